"""CPU: the scene table of the ragged-batch kernels (pq3d_amd/csrc/ragged.h: host fill, unrolled lookup, binary search; shared by
the kernels and by tests/ragged_check_main.cpp) compiled as a stand-alone host program and run.  (The same program built with
-fsanitize=address,undefined turns a read past an offsets array into a reported out-of-bounds access.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scene_table_as_a_host_program(tmp_path):
    exe = tmp_path / "ragged_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "ragged_check_main.cpp"),
                           "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().strip() == "ok"
