"""lig_rows_diagnose_attached without a GPU: the Python method exists and its ctypes signature is the header's declaration, the entry is
exported, the argument checks that come before any trace or device is looked at answer, and no struct of the ABI changed size."""
import ctypes as C
import inspect
import os
import re

import pytest

import hip_lib

ROOT = hip_lib.ROOT


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def declaration(name):
    """the parameter list of `name` in include/lig_hip.h -> [(type, parameter name)], comments removed"""
    hdr = open(os.path.join(ROOT, "include", "lig_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, "%s is not declared" % name
    out = []
    for p in m.group(1).split(","):
        ty, pname = re.match(r"\s*(.*?)\s*(\w+)\s*$", p, flags=re.S).groups()
        out.append((re.sub(r"\s+", " ", ty).replace(" *", "*"), pname))
    return out


def test_signature_matches_the_header(amd):
    L = amd.load_library()
    decl = declaration("lig_rows_diagnose_attached")
    assert decl == [("lig_trace*", "trace"), ("lig_diag_linear*", "lin_out"), ("uint64_t", "lin_cap"), ("lig_diag_quad*", "quad_out"),
                    ("uint64_t", "quad_cap"), ("lig_diag_info*", "info")]
    # lig_rows_diagnose without its system: the same parameters in the same order
    assert decl == [p for p in declaration("lig_rows_diagnose") if p[1] != "sys"]
    ctype = {"lig_trace*": C.c_void_p, "lig_diag_linear*": C.c_void_p, "lig_diag_quad*": C.c_void_p, "uint64_t": C.c_uint64,
             "lig_diag_info*": C.POINTER(amd.DiagInfo)}
    assert list(L.lig_rows_diagnose_attached.argtypes) == [ctype[ty] for ty, _ in decl]
    assert L.lig_rows_diagnose_attached.restype is C.c_int
    assert "lig_rows_diagnose_attached" in amd.EXPORTS


def test_python_method(amd):
    sig = inspect.signature(amd.Context.rows_diagnose_attached)
    assert list(sig.parameters) == ["self", "trace", "lin_cap", "quad_cap"]
    assert (sig.parameters["lin_cap"].default, sig.parameters["quad_cap"].default) == (1024, 1024)
    ref = inspect.signature(amd.Context.rows_diagnose)
    assert [p for p in ref.parameters if p != "system"] == list(sig.parameters)


def test_argument_errors_before_any_trace_is_looked_at(amd):
    L = amd.load_library()
    info = amd.DiagInfo()
    info.struct_bytes = C.sizeof(amd.DiagInfo)
    assert L.lig_rows_diagnose_attached(None, None, 0, None, 0, C.byref(info)) == -1
    assert L.lig_rows_diagnose_attached(None, None, 0, None, 0, None) == -1
    short = amd.DiagInfo()
    short.struct_bytes = C.sizeof(amd.DiagInfo) - 8
    assert L.lig_rows_diagnose_attached(None, None, 0, None, 0, C.byref(short)) == -1
    # (a NULL array with a cap > 0 and the state errors on a REAL trace: tests/test_gpu_diagnose_attached.py)


def test_abi_sizes_are_unchanged(amd):
    L = amd.load_library()
    sizes = (C.c_uint32 * 6)()
    L.lig_abi_sizes(sizes)
    # lig_batch_op, lig_synth_job, lig_proof_info, lig_verify_info, lig_rows_job, lig_comm
    assert list(sizes) == [32, 192, 184, 56, 168, 64]
    assert C.sizeof(amd.DiagInfo) == 48 and amd.DIAG_LINEAR.itemsize == 40 and amd.DIAG_QUAD.itemsize == 48
