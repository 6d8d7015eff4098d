"""Derived product rows on the host side (no GPU): an ELEM_PRODUCT row (lig_rows_job.elem_bytes = LIG_ELEM_PRODUCT, the z row of
a quadratic triple that the library forms on the device) contributes nothing to the packed byte array, its neighbours keep their
layout, and narrowest_widths marks exactly the QZ rows when asked to."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hip_lib                     # noqa: E402

amd = hip_lib.load()
K = 512
LIMIT = {amd.ELEM_BIT: 2, 1: 1 << 8, 2: 1 << 16, 4: 1 << 32, 8: 1 << 64, 32: 1 << 250, 0: 1 << 250}


def rows_of(values, k=K):
    R = len(values)
    out = np.zeros((R, k, 8), dtype=np.uint32)
    for r in range(R):
        for i, v in enumerate(values[r]):
            for j in range(8):
                out[r, i, j] = (v >> (32 * j)) & 0xFFFFFFFF
    return out


def packed_len(w, l, k=K):
    if w == amd.ELEM_PRODUCT:
        return 0
    if w in (0, 32):
        return k * 32
    n = (l + 7) // 8 if w == amd.ELEM_BIT else l * w
    return (n + 3) // 4 * 4


def test_the_constant_is_the_header_value():
    assert amd.ELEM_PRODUCT == 0x82 and amd.ELEM_PRODUCT != amd.ELEM_BIT


@pytest.mark.parametrize("l", [45, 317, 320])
def test_product_rows_take_no_bytes_and_leave_their_neighbours_where_the_parent_format_puts_them(l):
    """the packed bytes with ELEM_PRODUCT rows == the packed bytes of the same matrix with those rows REMOVED, for operand rows of
    every width (odd l: the 4-byte round-up of the row in front of a derived row and the start of the row behind it)"""
    rng = np.random.default_rng(l)
    D = amd.ELEM_PRODUCT
    widths = [1, amd.ELEM_BIT, amd.ELEM_BIT, D, 2, 1, D, 32, 8, D, 4, 4, D, 2, 8, 0, D, amd.ELEM_BIT]
    vals = [[int.from_bytes(rng.bytes(32), "little") % LIMIT.get(w, 1 << 250) for _ in range(l)] for w in widths]
    rows = rows_of(vals)
    rows[:, l:, 0] = 99                                                # full rows carry their pads
    got = amd.pack_rows(rows, widths, l)
    keep = [r for r, w in enumerate(widths) if w != D]
    want = amd.pack_rows(rows[keep], [widths[r] for r in keep], l)
    assert got.tobytes() == want.tobytes()
    assert len(got) == sum(packed_len(w, l) for w in widths)
    off = 0
    for r, w in enumerate(widths):                                     # every shipped row starts 4-byte aligned at the sum in front of it
        assert off % 4 == 0
        n = packed_len(w, l)
        if w in (0, 32):
            assert bytes(got[off:off + n]) == rows[r].tobytes()
        elif w in (1, 2, 4, 8):
            assert [int.from_bytes(bytes(got[off + i * w:off + (i + 1) * w]), "little") for i in range(l)] == vals[r]
        off += n
    assert off == len(got)


def test_a_product_row_is_not_looked_at():
    """whatever the caller left in the z row (a wrong product, a value that fits no narrow width) does not reach the bytes"""
    l = 9
    rows = rows_of([[3] * l, [5] * l, [1 << 200] * l])
    a = amd.pack_rows(rows, [1, 1, amd.ELEM_PRODUCT], l)
    rows[2] = 0
    assert a.tobytes() == amd.pack_rows(rows, [1, 1, amd.ELEM_PRODUCT], l).tobytes() == amd.pack_rows(rows[:2], [1, 1], l).tobytes()


def test_narrowest_widths_marks_exactly_the_qz_rows_when_asked():
    l = 12
    P = amd.ROW_DRAW_PAD
    kinds = np.array([0, 1, 2, 3, 0, 8, 9, 10, 1, 2, 3, 4, 5, 6, 7, 1, 2, 3], dtype=np.uint8)     # BQZ (10) is not a QZ row
    rng = np.random.default_rng(3)
    tops = [1, 255, 1 << 20, 1 << 70, 1 << 40, 3, 3, 9, 1, 1, 1, 2, 1, 7, 7, 1 << 100, 1 << 100, 1 << 200]
    rows = rows_of([[int(rng.integers(0, 2)) for _ in range(l - 1)] + [t] for t in tops])
    plain = amd.narrowest_widths(rows, kinds, l)
    assert list(plain) == [amd.ELEM_BIT, 1, 4, 32, 8, 32, 32, 32, amd.ELEM_BIT, amd.ELEM_BIT, amd.ELEM_BIT, 32, 32, 32, 32, 32, 32, 32]
    assert list(amd.narrowest_widths(rows, kinds, l, derive_products=False)) == list(plain)
    for kk in (kinds, kinds | P):
        got = amd.narrowest_widths(rows, kk, l, derive_products=True)
        assert [r for r in range(len(kinds)) if got[r] == amd.ELEM_PRODUCT] == [3, 10, 17]
        assert all(got[r] == plain[r] for r in range(len(kinds)) if r not in (3, 10, 17))
    packed = amd.pack_rows(rows, amd.narrowest_widths(rows, kinds, l, derive_products=True), l)
    assert len(packed) == len(amd.pack_rows(rows, plain, l)) - sum(packed_len(int(plain[r]), l) for r in (3, 10, 17))
