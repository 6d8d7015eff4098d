"""CPU-only: the prepared-linear-system entries (lig_linear_prepare & co.) at the boundary -- declared in include/lig_hip.h, exported
by the library, marshalled by the Python binding.  The binding is exercised on a recording stub in place of the loaded library (no
device call is made), and on the real library through argument checks that return before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hip_lib

ROOT = hip_lib.ROOT
ENTRIES = ["lig_linear_prepare", "lig_linear_program_release", "lig_rows_attach_linear", "lig_rows_verify_attach_linear",
           "lig_rows_set_linear_values", "lig_rows_verify_set_linear_values", "lig_linear_program_form"]
P = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


@pytest.fixture(scope="module")
def amd():
    mod = hip_lib.load()
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


def test_header_declares_and_library_exports_the_seven_entries(amd):
    hdr = open(os.path.join(ROOT, "include", "lig_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(amd.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), "not declared: %s" % name
        assert hasattr(lib, name), "not exported: %s" % name
        assert name in amd.EXPORTS
    assert "typedef struct lig_linear_program lig_linear_program;" in code
    # the sharded entry is out of scope, and the header says so
    doc = hdr[hdr.index("prepared linear systems"):hdr.index("typedef struct lig_linear_program")]
    assert "lig_shard_rows_set_linear" in doc
    L = amd.load_library()
    assert L.lig_linear_program_release.restype is None
    assert len(L.lig_linear_prepare.argtypes) == 5 and len(L.lig_linear_program_form.argtypes) == 7


class Stub:
    """stands where the loaded library stands in a Context: records every call, answers 0, hands out program handle 0xABC0"""

    SNAP = {"lig_linear_prepare": [(2, 3, 1)], "lig_rows_set_linear_values": [(1, 2, 32)], "lig_rows_verify_set_linear_values": [(1, 2, 32)],
            "lig_linear_program_form": [(2, None, 32), (3, 4, 32)]}

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            # (pointer, count, bytes per item) arguments are read NOW, into bytes: the binding's arrays live only as long as the call
            args = list(args)
            for ptr, cnt, size in self.SNAP.get(name, ()):
                p = value(args[ptr])
                args[ptr] = C.string_at(p, (args[cnt] if cnt is not None else 1) * size) if p else None
            args = tuple(args)
            self.calls.append((name, args))
            if name == "lig_linear_prepare":
                args[4]._obj.value = 0xABC0
            if name == "lig_linear_program_bytes":
                args[1]._obj.value, args[2]._obj.value = 1000, 200
            return 0
        return fn

    def named(self, name):
        return [a for n, a in self.calls if n == name]


def stub_context(amd):
    c = amd.Context.__new__(amd.Context)
    c.L, c.h, c.l, c.k, c.n, c._bufs = Stub(), C.c_void_p(0x1000), 320, 512, 2048, []
    return c


def value(p):
    return p.value if hasattr(p, "value") else p


def test_binding_marshals_the_arguments(amd):
    c = stub_context(amd)
    try:
        sysb = amd.LinearSystem.make([0, 1, 2], [0, 5], [amd.COEF_ONE, 0], [1], [1], [7, P - 1])
        kinds = [0, 0x80, 3]
        prog = c.linear_prepare(sysb, kinds)
        (h, sp, kp, rows, out), = c.L.named("lig_linear_prepare")
        assert value(h) == 0x1000 and rows == 3 and kp == bytes(kinds) and sp._obj is sysb
        assert isinstance(prog, amd.LinearProgram) and value(prog.h) == 0xABC0 and prog.bytes() == (1000, 200)
        assert c.linear_prepare(sysb, kinds, rows=2).h.value == 0xABC0 and c.L.named("lig_linear_prepare")[1][3] == 2
        with pytest.raises(ValueError):
            c.linear_prepare(sysb, kinds, rows=4)
        tr, vt = C.c_void_p(0x2000), C.c_void_p(0x3000)
        c.rows_attach_linear(tr, prog)
        c.rows_attach_linear(tr, None)
        c.rows_verify_attach_linear(vt, prog)
        assert [(value(a), value(b)) for a, b in c.L.named("lig_rows_attach_linear")] == [(0x2000, 0xABC0), (0x2000, None)]
        assert [(value(a), value(b)) for a, b in c.L.named("lig_rows_verify_attach_linear")] == [(0x3000, 0xABC0)]
        # values: integers, limbs, None
        tab = [0, 1, P - 1, 1 << 255]
        c.rows_set_linear_values(tr, tab)
        c.rows_set_linear_values(tr, amd.coef_table(tab))
        c.rows_set_linear_values(tr, None)
        c.rows_verify_set_linear_values(vt, tab)
        calls = c.L.named("lig_rows_set_linear_values")
        want = b"".join(v.to_bytes(32, "little") for v in tab)
        for t, p, ncoef in calls[:2]:
            assert value(t) == 0x2000 and ncoef == 4 and p == want
        assert calls[2][1] is None and calls[2][2] == 0
        (t, p, ncoef), = c.L.named("lig_rows_verify_set_linear_values")
        assert value(t) == 0x3000 and ncoef == 4 and p == want
        # the stand-alone form
        key = bytes(range(32))
        assert c.linear_program_form(prog, key, C.c_void_p(0x4000)) == bytes(32)
        c.linear_program_form(prog, key, C.c_void_p(0x4000), coefs=tab)
        f0, f1 = c.L.named("lig_linear_program_form")
        assert value(f0[0]) == 0x1000 and value(f0[1]) == 0xABC0 and f0[2] == key and f0[3] is None and f0[4] == 0
        assert value(f0[5]) == 0x4000 and f0[6] is not None
        assert f1[3] == want and f1[4] == 4
        # a released program is refused by the binding, before any call
        prog.release()
        n = len(c.L.calls)
        for call in (lambda: c.rows_attach_linear(tr, prog), lambda: c.rows_verify_attach_linear(vt, prog),
                     lambda: c.linear_program_form(prog, key, C.c_void_p(0x4000)), prog.bytes):
            with pytest.raises(amd.LigError, match="released"):
                call()
        assert len(c.L.calls) == n
    finally:
        c.h = None


def test_linear_program_releases_exactly_once(amd):
    c = stub_context(amd)
    try:
        sysb = amd.LinearSystem.make([0, 1], [0], [amd.COEF_ONE])
        released = lambda: [value(a[0]) for a in c.L.named("lig_linear_program_release")]
        with c.linear_prepare(sysb, [0]) as prog:
            assert released() == [] and prog.h
        assert released() == [0xABC0] and prog.h is None
        prog.release()
        del prog
        assert released() == [0xABC0]
        prog = c.linear_prepare(sysb, [0])
        prog.release()
        prog.release()
        with prog:
            pass
        assert released() == [0xABC0] * 2
        with pytest.raises(RuntimeError):
            with c.linear_prepare(sysb, [0]) as prog:
                raise RuntimeError("the body failed")
        assert released() == [0xABC0] * 3
        c.linear_prepare(sysb, [0])                   # dropped without release(): the finaliser does it, once
        import gc
        gc.collect()
        assert released() == [0xABC0] * 4
    finally:
        c.h = None


def test_the_library_checks_arguments_before_any_device_call(amd):
    """null handles: every entry answers LIG_E_ARG (-1) without touching a device; release(NULL) is a no-op"""
    L = amd.load_library()
    out = C.c_void_p()
    sysb = amd.LinearSystem.make([0, 1], [0], [amd.COEF_ONE])
    kinds = np.zeros(1, dtype=np.uint8)
    buf = np.zeros(32, dtype=np.uint8)
    assert L.lig_linear_prepare(None, C.byref(sysb), kinds.ctypes.data, 1, C.byref(out)) == -1
    assert L.lig_rows_attach_linear(None, None) == -1
    assert L.lig_rows_verify_attach_linear(None, None) == -1
    assert L.lig_rows_set_linear_values(None, buf.ctypes.data, 1) == -1
    assert L.lig_rows_verify_set_linear_values(None, buf.ctypes.data, 1) == -1
    assert L.lig_linear_program_form(None, None, buf.ctypes.data, None, 0, None, buf.ctypes.data) == -1
    assert L.lig_linear_program_bytes(None, None, None) == -1
    L.lig_linear_program_release(None)
