"""lig_rows_diagnose without a GPU: the argument checks that come before any trace or device is looked at, and the Python yardstick
of the GPU tests (tests/diagnose_ref.py) against linear_ref.holds on satisfied and corrupted matrices."""
import ctypes as C

import numpy as np
import pytest

import diagnose_ref as dr
import hip_lib
import linear_ref as lr


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def test_null_trace_and_short_info_are_argument_errors(amd):
    L = amd.load_library()
    info = amd.DiagInfo()
    info.struct_bytes = C.sizeof(amd.DiagInfo)
    assert C.sizeof(amd.DiagInfo) == 48 and amd.DIAG_LINEAR.itemsize == 40 and amd.DIAG_QUAD.itemsize == 48
    assert L.lig_rows_diagnose(None, None, None, 0, None, 0, C.byref(info)) == -1
    assert L.lig_rows_diagnose(None, None, None, 0, None, 0, None) == -1
    short = amd.DiagInfo()
    short.struct_bytes = C.sizeof(amd.DiagInfo) - 8
    assert L.lig_rows_diagnose(None, None, None, 0, None, 0, C.byref(short)) == -1
    # (a short struct_bytes and a NULL array with a nonzero cap on a REAL trace: tests/test_gpu_diagnose.py)


def test_reference_agrees_with_linear_ref_holds():
    l, k, n = 320, 512, 2048
    kinds, rows, _ = lr.build_trace(l, k, n, 3 * l + 17, l + 9)
    system = lr.make_system(kinds, rows, l, 2000, 0, seed=3, hot_terms=50)
    assert lr.holds(system, rows, l) and dr.linear_violations(system, rows, l) == []
    assert dr.quad_violations(kinds, rows, l) == []
    eq = lr.make_equality_system(kinds, l, 0)
    assert lr.holds(eq, rows, l) and dr.holds(eq, rows, l)
    bad = rows.copy()
    s = system.single_slot                       # constraint 0: w[s] = b
    bad[s // l, s % l, 0] ^= 1
    assert not lr.holds(system, bad, l)
    viol = dr.linear_violations(system, bad, l)
    assert viol and viol[0][0] == 0 and viol[0][1] in (1, dr.P - 1)
    # every violated constraint touches the changed slot
    for c, _ in viol:
        assert s in system.slots[system.term_begin[c]:system.term_begin[c + 1]]
    a, b = lr.equal_pairs(kinds, l)[4]
    bad = rows.copy()
    bad[b // l, b % l, 0] ^= 1
    assert not lr.holds(eq, bad, l)
    assert [c for c, _ in dr.linear_violations(eq, bad, l)] == [4]


def test_reference_quadratic_terms_and_residuals():
    l = 4
    kinds = np.array([0, 1, 2, 3, 5, 6, 7, 8, 9, 10], dtype=np.uint8)
    assert dr.quad_terms(kinds) == [(1, 2, 3), (4, 4, 4), (5, dr.NO_ROW, 6), (7, 8, 9)]
    assert dr.quad_terms(kinds | 0x80) == dr.quad_terms(kinds)
    rows = np.zeros((10, 8, 8), dtype=np.uint32)
    rows[1, :l, 0], rows[2, :l, 0], rows[3, :l, 0] = [2, 3, 4, 5], [7, 7, 7, 7], [14, 21, 29, 35]       # column 2: 28 expected
    rows[4, :l, 0] = [0, 1, 2, 1]                                                                        # a 2 in a bit row
    rows[5, :l, 0], rows[6, :l, 0] = [9, 9, 9, 9], [9, 9, 9, 8]
    want = [(1, 2, 3, 2, dr.P - 1), (4, 4, 4, 2, 2), (5, dr.NO_ROW, 6, 3, 1)]
    assert dr.quad_violations(kinds, rows, l) == want
    assert dr.quad_records(want)[1] == (4, 4, 4, 2, (2).to_bytes(32, "little"))
