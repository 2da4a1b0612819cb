"""CPU: the C-ABI library loads, exports every symbol include/pq3d_hip.h declares, the ctypes structs agree with
the header's layout, the host modules mirror the reference's state_dict, and the product path fails loudly
(no CPU / oracle fallback)."""
import ctypes
import os
import re
import subprocess

import pytest

from pq3d_amd import _lib, build
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pq3d_hip.h")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pq3d_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(lib):
    declared = header_functions()
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/pq3d_hip.h but not exported"
    assert sorted(_lib.EXPORTS) == declared, "ctypes binding and header disagree on the entry-point set"
    assert lib.pq3d_version() >= 1


def header_text():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def ctypes_structs():
    """{normalised name: class} of every ctypes.Structure the binding defines ('pq3d_adamw_hp' and AdamWHp -> 'adamwhp')."""
    return {n.lower(): c for n, c in vars(_lib).items() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c.__module__ == _lib.__name__}


def header_structs():
    """{normalised name: typedef name} of every struct the header defines."""
    return {t[len("pq3d_"):].replace("_", ""): t for t in re.findall(r"}\s*(pq3d_\w+)\s*;", header_text())}


def test_struct_layouts_match_header(tmp_path):
    """Every Structure of the binding against the header's struct of the same name: sizeof, and offsetof / sizeof of every field,
    from a C program generated from the ctypes classes and compiled against the header."""
    ours, theirs = ctypes_structs(), header_structs()
    assert sorted(ours) == sorted(theirs) and len(ours) >= 18, "ctypes binding and header disagree on the set of structs"
    lines, want = [], []
    for key in sorted(ours):
        cls, ctype = ours[key], theirs[key]
        lines.append(f'  printf("{ctype} %zu\\n", sizeof({ctype}));')
        want.append(f"{ctype} {ctypes.sizeof(cls)}")
        for name, *_ in cls._fields_:
            lines.append(f'  printf("{ctype}.{name} %zu %zu\\n", offsetof({ctype}, {name}), sizeof((({ctype}*)0)->{name}));')
            want.append(f"{ctype}.{name} {getattr(cls, name).offset} {getattr(cls, name).size}")
    csrc = tmp_path / "layout.c"
    csrc.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pq3d_hip.h"\nint main(void) {\n' + "\n".join(lines) +
                    "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(csrc), "-o", str(exe)])
    got = subprocess.check_output([str(exe)]).decode().splitlines()
    assert len(got) == len(want) > 400
    assert [g for g, w in zip(got, want) if g != w] == [], "header layout (listed) differs from the ctypes Structure"


def test_header_constants_match_compiler(tmp_path):
    """Every non-guard PQ3D_* macro of the header, as gcc evaluates it, against _lib.H: the same names, the same values."""
    names = [n for n in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(PQ3D_\w+)", header_text(), flags=re.M) if n != "PQ3D_HIP_H"]
    assert len(names) == len(set(names)) >= 56
    csrc = tmp_path / "constants.c"
    csrc.write_text('#include <stdio.h>\n#include "pq3d_hip.h"\nint main(void) {\n' +
                    "\n".join(f'  printf("{n} %lld\\n", (long long)({n}));' for n in names) + "\n  return 0;\n}\n")
    exe = tmp_path / "constants"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(csrc), "-o", str(exe)])
    got = {n: int(v) for n, v in (line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())}
    assert sorted(got) == sorted(names)
    assert got == _lib.H._asdict()


def test_header_reader_refuses_what_it_cannot_read():
    for bad in ("1.5f", "(PQ3D_X + 1)", "(1", "1)", "1 + 1", "PQ3D_X"):
        with pytest.raises(_lib.Pq3dError, match=r"\bPQ3D_BAD\b"):
            _lib.header_constants(f"#define PQ3D_OK 3\n#define PQ3D_BAD {bad}\n")
    with pytest.raises(_lib.Pq3dError, match=r"\bPQ3D_BAD\b"):
        _lib.header_constants("#define PQ3D_BAD(x) 3\n")
    guard_only = "/* #define PQ3D_A 1 */\n#ifndef PQ3D_X_H\n#define PQ3D_X_H   // #define PQ3D_B 2\n#include <stdint.h>\n#endif\n"
    assert _lib.header_constants(guard_only)._asdict() == {}
    text = "#define PQ3D_A ( -0x10 << 2 ) /* a comment\n over two lines */\n  # define PQ3D_B 7 // #define PQ3D_C 1\n#define OTHER x\n"
    assert _lib.header_constants(text)._asdict() == {"PQ3D_A": -64, "PQ3D_B": 7}
    with pytest.raises(AttributeError):
        _lib.H.PQ3D_F32 = 1


def test_no_hand_copies_of_header_constants():
    """No line of the package assigns a numeric literal and names a header macro in a trailing comment."""
    pat = re.compile(r"=\s*[-(0-9][^#\n]*#\s*PQ3D_[A-Z0-9_]+")
    assert pat.search("CHUNK = 1024      # PQ3D_OBJECT_CHUNK") and pat.search("MAX_CELLS = (1 << 24)   # PQ3D_DBSCAN_MAX_CELLS: cells")
    assert not pat.search('    fast = os.environ.get("PQ3D_CHAIN") != "0"      # PQ3D_CHAIN=0: per-sublayer launches')
    pkg = os.path.join(ROOT, "pq3d_amd")
    found = [f"{f}: {line.strip()}" for f in sorted(os.listdir(pkg)) if f.endswith(".py")
             for line in open(os.path.join(pkg, f)) if pat.search(line)]
    assert found == []


def test_error_word_decoder():
    table = {1: "first", 2: "second", 4: "third", 8: "fourth"}
    _lib.raise_error_word("who", 0, table)
    for word, text in ((1 | 4, "who: first; third"), (1 | 8, "who: first; fourth"), (2, "who: second"), (15, "who: first; second; third; fourth")):
        with pytest.raises(ValueError) as e:
            _lib.raise_error_word("who", word, table)
        assert str(e.value) == text and type(e.value) is ValueError


def _c_param(decl: str):
    """One parameter of a header prototype -> ('ptr', typedef name or None) | ('int' | 'float', bytes)."""
    words = re.findall(r"\w+", decl.replace("*", " "))[:-1]     # the last word is the parameter's name
    base = [w for w in words if w != "const"]
    if "*" in decl:
        return ("ptr", base[0] if decl.count("*") == 1 and base[0].startswith("pq3d_") else None)
    return {"int": ("int", 4), "int32_t": ("int", 4), "uint32_t": ("int", 4), "int64_t": ("int", 8), "float": ("float", 4),
            "double": ("float", 8)}[" ".join(base)]


def _ctypes_param(t):
    if t is ctypes.c_void_p or t is ctypes.c_char_p:
        return ("ptr", None)
    if isinstance(getattr(t, "_type_", None), type):             # POINTER(x)
        to = t._type_
        return ("ptr", header_structs()[to.__name__.lower()] if issubclass(to, ctypes.Structure) else None)
    assert issubclass(t, ctypes._SimpleCData), t
    return ("float" if t._type_ in "fd" else "int", ctypes.sizeof(t))


def test_prototypes_match_header(lib):
    """Every prototype of the header against the argtypes / restype the binding gives ctypes: number of arguments, pointer or
    scalar (and, for a descriptor, which struct), scalar width, float or integer, and the width of the return value."""
    protos = re.findall(r"\b(const char\s*\*|int64_t|int32_t|int)\s+(pq3d_\w+)\s*\(([^)]*)\)\s*;", header_text())
    assert sorted(n for _r, n, _a in protos) == header_functions() == sorted(_lib.EXPORTS) and len(protos) >= 120
    assert _lib._RET64 <= set(_lib._SIGS)
    for ret, name, params in protos:
        fn = getattr(lib, name)
        want_ret = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64}.get(ret, ctypes.c_char_p)
        assert fn.restype is want_ret and (name in _lib._RET64) == (ret == "int64_t"), f"{name}: return type"
        params = [] if params.strip() == "void" else [_c_param(p) for p in params.split(",")]
        if name not in _lib._SIGS:
            assert name in ("pq3d_last_error", "pq3d_version") and not params and not fn.argtypes, name
            continue
        assert fn.argtypes == _lib._SIGS[name]
        assert [_ctypes_param(t) for t in _lib._SIGS[name]] == params, f"{name}: argument list differs from the header"


def test_call_reports_argument_errors(lib):
    """_lib.call: descriptor by reference, explicit stream, and the library's error text under the entry point's name."""
    d = _lib.GemmDesc()
    d.groups, d.batch, d.M, d.N, d.K = 999, 1, 4, 4, 4
    with pytest.raises(_lib.Pq3dError, match=r"^pq3d_gemm failed \(rc=-1\): .*groups"):
        _lib.call("pq3d_gemm", d, stream=0)
    with pytest.raises(_lib.Pq3dError, match="not a launch entry point"):
        _lib.call("pq3d_segment_plan_bytes", 1, 1, stream=0)


def test_call_rejects_cpu_tensors_before_the_library(lib, monkeypatch):
    import torch
    fn, ptrs, by_ref = _lib._ENTRY.get("pq3d_colsum") or _lib._entry("pq3d_colsum")
    entered = []
    monkeypatch.setitem(_lib._ENTRY, "pq3d_colsum", (lambda *a: entered.append(a) or 0, ptrs, by_ref))
    x, out = torch.zeros(4, 4), torch.zeros(4)
    for args in ((x, _lib.F32, 4, 4, 4, None), (None, _lib.F32, 4, 4, 4, out)):
        with pytest.raises(_lib.Pq3dError, match="device tensors"):
            _lib.call("pq3d_colsum", *args, stream=0)
    assert not entered
    _lib.call("pq3d_colsum", None, _lib.F32, 4, 4, 4, None, stream=0)     # (the spy does see a call that passes)
    assert len(entered) == 1 and entered[0][-1] == 0


def test_argument_errors_are_reported(lib):
    d = _lib.GemmDesc()
    d.groups, d.batch, d.M, d.N, d.K = 999, 1, 4, 4, 4
    rc = lib.pq3d_gemm(ctypes.byref(d), None)
    assert rc == -1 and b"groups" in lib.pq3d_last_error()
    a = _lib.AttnDesc()
    a.B, a.H, a.Lq, a.Lk, a.dh = 1, 1, 4, 4, 48
    assert lib.pq3d_attn_fwd(ctypes.byref(a), None) == -1 and b"head dim" in lib.pq3d_last_error()


def test_comm_entry_points_without_a_gpu(lib):
    """SURVEY 8b's gradient-exchange exports (csrc/comm.hip): the host-only parts answer without a GPU -- the wire form's scratch size,
    argument errors before any RCCL call, and (librccl is bound with dlopen at first use) the rendezvous id."""
    assert lib.pq3d_allreduce_wire_scratch_bytes(8, 1000) == (3 * 8 + 1) * 128 * 2
    assert lib.pq3d_allreduce_wire_scratch_bytes(1, 0) == 0 and lib.pq3d_allreduce_wire_scratch_bytes(0, 5) == -1
    junk = ctypes.create_string_buffer(64)
    assert lib.pq3d_allreduce_grads(junk, None, 8, 0, 1, None) == -1 and b"not a communicator" in lib.pq3d_last_error()
    assert lib.pq3d_comm_destroy(junk) == -1
    h = ctypes.c_void_p()
    assert lib.pq3d_comm_init(2, 2, junk, ctypes.byref(h)) == -1 and b"rank" in lib.pq3d_last_error() and not h.value
    a, b = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
    rc = lib.pq3d_comm_unique_id(a)
    if rc == 0:      # (a host without librccl reports an error text instead)
        assert lib.pq3d_comm_unique_id(b) == 0 and a.raw != b.raw and any(a.raw)
    else:
        assert b"rccl" in lib.pq3d_last_error().lower()


def test_state_dict_keys_match_reference():
    """Every parameter name/shape of the reference (recorded as grad/<name> in the fixtures) exists in our modules."""
    for name in ("F2_c1_mask", "F4_c2_slice", "F5_dimloc6", "F5_offline_mask"):
        z, args = util.load_fixture(name)
        _cfg, model, _sd, _dd = util.model_case(args)
        ref = sorted(k[5:-4] for k in z.files if k.startswith("grad/") and k.endswith("/sum"))
        ours = dict(model.named_parameters())
        assert sorted(ours) == ref, "parameter names differ from the reference's state_dict"
        for n in ref:
            assert tuple(ours[n].shape) == tuple(z[f"grad/{n}/shape"]), n
        assert "coord_encoder.pos_enc.gauss_B" in model.state_dict() or args.get("dim_loc", 3) > 3
        groups = model.get_opt_params()
        assert sum(len(g["params"]) for g in groups) == len(ours)


def test_no_cpu_fallback():
    """CPU tensors must raise (the product path never silently computes on the host or through the oracle)."""
    _z, args = util.load_fixture("F1_c1")
    _cfg, model, _sd, dd = util.model_case(args)
    with pytest.raises(_lib.Pq3dError):
        model(dd)
    for f in os.listdir(os.path.join(ROOT, "pq3d_amd")):
        if f.endswith(".py"):
            text = open(os.path.join(ROOT, "pq3d_amd", f)).read()
            assert "import oracle" not in text and "from oracle" not in text, f"{f} imports the oracle"
