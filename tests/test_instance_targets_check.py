"""CPU: the range checks of the instance-target kernels (pq3d_amd/csrc/instance_targets_check.h, shared by the kernels and by
tests/instance_targets_check_main.cpp) compiled as a stand-alone host program and run: extreme int64 ids are rejected, every
accepted one indexes inside an exactly sized table.  (The same program built with -fsanitize=address,undefined turns a wrong
check into a reported out-of-bounds access.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_range_checks_as_a_host_program(tmp_path):
    exe = tmp_path / "instance_targets_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "instance_targets_check_main.cpp"),
                           "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().strip() == "ok"
