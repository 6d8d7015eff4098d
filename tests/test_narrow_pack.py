"""The narrow row format on the host side (no GPU): pack_rows lays out every width of lig_rows_job.elem_bytes -- bits, 1-, 2-, 4-,
8-byte integers, full rows -- as include/lig_hip.h describes it, and narrowest_widths picks the smallest width a row fits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hip_lib                     # noqa: E402

amd = hip_lib.load()
K = 64


def rows_of(values, k=K):
    """python ints (R x l) -> (R, k, 8) uint32 limbs, zeros past the data slots"""
    R, l = len(values), len(values[0])
    out = np.zeros((R, k, 8), dtype=np.uint32)
    for r in range(R):
        for i, v in enumerate(values[r]):
            for j in range(8):
                out[r, i, j] = (v >> (32 * j)) & 0xFFFFFFFF
    return out


def packed_len(w, l, k=K):
    if w in (0, 32):
        return k * 32
    n = (l + 7) // 8 if w == amd.ELEM_BIT else l * w
    return (n + 3) // 4 * 4


@pytest.mark.parametrize("l", [1, 7, 8, 9, 31, 32, 33, 45, 48])
def test_bit_rows_are_lsb_first_and_padded_to_four_bytes(l):
    rng = np.random.default_rng(l)
    bits = [int(b) for b in rng.integers(0, 2, l)]
    p = amd.pack_rows(rows_of([bits]), [amd.ELEM_BIT], l)
    assert len(p) == packed_len(amd.ELEM_BIT, l) and len(p) % 4 == 0
    for i, b in enumerate(bits):
        assert (p[i // 8] >> (i % 8)) & 1 == b
    assert not p[(l + 7) // 8:].any()                                  # the round-up is zero
    assert bytes(p[:(l + 7) // 8]) == np.packbits(np.array(bits, dtype=np.uint8), bitorder="little").tobytes()
    if l % 8:
        assert p[l // 8] >> (l % 8) == 0                               # bits past l in the last byte are zero


@pytest.mark.parametrize("w", [1, 2])
@pytest.mark.parametrize("l", [1, 3, 5, 317, 320])
def test_byte_and_u16_rows_are_little_endian_and_padded(w, l):
    rng = np.random.default_rng(w * 1000 + l)
    vals = [int(v) for v in rng.integers(0, 1 << (8 * w), l)]
    p = amd.pack_rows(rows_of([vals], k=512), [w], l)
    assert len(p) == packed_len(w, l, 512) and len(p) % 4 == 0
    assert bytes(p[:l * w]) == b"".join(v.to_bytes(w, "little") for v in vals)
    assert not p[l * w:].any()


def test_mixed_widths_in_one_buffer_keep_every_row_four_byte_aligned():
    l = 317
    rng = np.random.default_rng(5)
    widths = [amd.ELEM_BIT, 1, 2, 4, 8, 32, 1, amd.ELEM_BIT, 0, 2]
    limit = {amd.ELEM_BIT: 2, 1: 1 << 8, 2: 1 << 16, 4: 1 << 32, 8: 1 << 64, 32: 1 << 250, 0: 1 << 250}
    vals = [[int.from_bytes(rng.bytes(32), "little") % limit[w] for _ in range(l)] for w in widths]
    rows = rows_of(vals, k=512)
    p = amd.pack_rows(rows, widths, l)
    off = 0
    for r, w in enumerate(widths):
        assert off % 4 == 0
        n = packed_len(w, l, 512)
        seg = bytes(p[off:off + n])
        if w in (0, 32):
            assert seg == rows[r].tobytes()
        elif w == amd.ELEM_BIT:
            got = np.unpackbits(np.frombuffer(seg, dtype=np.uint8), bitorder="little")[:l]
            assert [int(x) for x in got] == vals[r]
        else:
            assert [int.from_bytes(seg[i * w:(i + 1) * w], "little") for i in range(l)] == vals[r]
        off += n
    assert off == len(p)


def test_four_eight_and_full_rows_keep_their_layout():
    """an independent restatement of the layout before the narrower widths existed: a 4 / 8-byte row is its l slots as
    little-endian integers of that width, back to back; a full row is its k x 32 bytes"""
    l = 45
    rng = np.random.default_rng(9)
    widths = [4, 8, 32, 4, 0, 8]
    vals = [[int(v) for v in rng.integers(0, 1 << 32, l)], [int.from_bytes(rng.bytes(8), "little") for _ in range(l)],
            [int.from_bytes(rng.bytes(31), "little") for _ in range(l)], [int(v) for v in rng.integers(0, 1 << 32, l)],
            [int.from_bytes(rng.bytes(31), "little") for _ in range(l)], [int.from_bytes(rng.bytes(8), "little") for _ in range(l)]]
    rows = rows_of(vals)
    rows[2, l:, 0] = 77                                                 # full rows carry their pads
    want = b""
    for r, w in enumerate(widths):
        if w in (0, 32):
            want += b"".join(int(x).to_bytes(4, "little") for x in rows[r].reshape(-1))
        else:
            want += b"".join(v.to_bytes(w, "little") for v in vals[r])
    assert amd.pack_rows(rows, widths, l).tobytes() == want


def test_pack_rows_refuses_values_that_do_not_fit():
    l = 8
    with pytest.raises(AssertionError):
        amd.pack_rows(rows_of([[2] + [0] * 7]), [amd.ELEM_BIT], l)
    with pytest.raises(AssertionError):
        amd.pack_rows(rows_of([[256] + [0] * 7]), [1], l)
    with pytest.raises(AssertionError):
        amd.pack_rows(rows_of([[1 << 16] + [0] * 7]), [2], l)
    with pytest.raises(ValueError):
        amd.pack_rows(rows_of([[0] * 8]), [3], l)


@pytest.mark.parametrize("top,want", [(0, "bit"), (1, "bit"), (2, 1), (255, 1), (256, 2), (65535, 2), (65536, 4),
                                      ((1 << 32) - 1, 4), (1 << 32, 8), ((1 << 64) - 1, 8), (1 << 64, 32)])
def test_narrowest_width_at_the_boundaries(top, want):
    l = 12
    want = amd.ELEM_BIT if want == "bit" else want
    kinds = np.array([0, 1, 2, 3], dtype=np.uint8)
    rows = rows_of([[0, 1] * 5 + [0, top]] * 4)
    assert list(amd.narrowest_widths(rows, kinds, l)) == [want] * 4
    assert list(amd.narrowest_widths(rows, kinds | amd.ROW_DRAW_PAD, l)) == [want] * 4
    packed = amd.pack_rows(rows, amd.narrowest_widths(rows, kinds, l), l)             # and the rows fit what was chosen
    assert len(packed) == 4 * packed_len(want, l)


def test_narrowest_width_ignores_pads_and_keeps_other_kinds_full():
    l = 12
    rows = rows_of([[1] * l] * 4)
    rows[:, l:, :] = 0xFFFFFFFF                                         # pad slots do not count
    kinds = np.array([0, 4, 5, 6], dtype=np.uint8)                      # LINEAR, INIT, BIT, EQX
    assert list(amd.narrowest_widths(rows, kinds, l)) == [amd.ELEM_BIT, 32, 32, 32]
