"""Mixed witness rows on the host side (no GPU): pack_rows_mixed lays out lig_rows_job.wide_per_row as include/lig_hip.h describes
it -- the narrow row, then 36-byte records {uint32 column, 8 uint32 limbs} -- and mixed_widths picks, per row, the base width whose
narrow row plus records is the fewest bytes.  The byte arithmetic of the two recorded i32_add traces (tests/golden) is asserted."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hip_lib                     # noqa: E402

amd = hip_lib.load()
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
K = 64


def rows_of(values, k=K):
    """python ints (R x l) -> (R, k, 8) uint32 limbs, zeros past the data slots"""
    out = np.zeros((len(values), k, 8), dtype=np.uint32)
    for r, row in enumerate(values):
        for i, v in enumerate(row):
            for j in range(8):
                out[r, i, j] = (v >> (32 * j)) & 0xFFFFFFFF
    return out


def u32(*words):
    return b"".join(int(w).to_bytes(4, "little") for w in words)


def test_a_hand_written_two_row_example():
    """l = 5.  Row 0: bits 1,0,*,1,* with p - 1 in slot 2 and 2^64 in slot 4 -> one dword of bits (0b01001, the two wide slots 0),
    then the records (2, p - 1), (4, 2^64).  Row 1: bytes 7,*,255,0,9 with 256 in slot 1 -> 5 bytes rounded up to 8, then (1, 256)."""
    l = 5
    rows = rows_of([[1, 0, P - 1, 1, 1 << 64], [7, 256, 255, 0, 9]])
    got = amd.pack_rows_mixed(rows, [amd.ELEM_BIT, 1], [2, 1], l).tobytes()
    pm1 = [((P - 1) >> (32 * j)) & 0xFFFFFFFF for j in range(8)]
    want = (u32(0b01001) + u32(2, *pm1) + u32(4, 0, 0, 1, 0, 0, 0, 0, 0)
            + bytes([7, 0, 255, 0, 9, 0, 0, 0]) + u32(1, 256, 0, 0, 0, 0, 0, 0, 0))
    assert got == want
    assert len(got) == 4 + 2 * 36 + 8 + 36


def test_without_records_it_is_pack_rows():
    l = 45
    rng = np.random.default_rng(3)
    widths = [amd.ELEM_BIT, 1, 2, 4, 8, 32, 0, amd.ELEM_PRODUCT]
    limit = {amd.ELEM_BIT: 2, 1: 1 << 8, 2: 1 << 16, 4: 1 << 32, 8: 1 << 64, 32: 1 << 250, 0: 1 << 250, amd.ELEM_PRODUCT: 2}
    rows = rows_of([[int.from_bytes(rng.bytes(32), "little") % limit[w] for _ in range(l)] for w in widths])
    assert amd.pack_rows_mixed(rows, widths, [0] * len(widths), l).tobytes() == amd.pack_rows(rows, widths, l).tobytes()


def test_pack_rows_mixed_refuses_counts_that_are_not_the_rows():
    l = 8
    with pytest.raises(ValueError):
        amd.pack_rows_mixed(rows_of([[2, 3] + [0] * 6]), [amd.ELEM_BIT], [1], l)       # two slots do not fit
    with pytest.raises(ValueError):
        amd.pack_rows_mixed(rows_of([[1 << 70] + [0] * 7]), [32], [1], l)               # records on a full row


def bit_length(limbs):
    return sum(int(limbs[j]) << (32 * j) for j in range(8)).bit_length()


def brute_force(rows, kinds, l, k):
    """the definition, slot by slot with python ints: min over the five bases of narrow bytes + 36 per misfit, narrower on a tie,
    full width only where it is not more bytes"""
    widths, wide = [], []
    for r, kd in enumerate(kinds):
        if (kd & 0x7F) > 3:
            widths.append(32); wide.append(0)
            continue
        bl = [bit_length(rows[r, i]) for i in range(l)]
        best = None
        for b, fit, nb in ((amd.ELEM_BIT, 1, (l + 31) // 32 * 4), (1, 8, (l + 3) // 4 * 4), (2, 16, (2 * l + 3) // 4 * 4), (4, 32, 4 * l), (8, 64, 8 * l)):
            c = sum(1 for x in bl if x > fit)
            if best is None or nb + 36 * c < best[0]:
                best = (nb + 36 * c, b, c)
        if 32 * k <= best[0]:
            widths.append(32); wide.append(0)
        else:
            widths.append(best[1]); wide.append(best[2])
    return widths, wide


def mixed_len(widths, wide, l, k):
    return sum(amd.narrow_row_bytes(w, l, k) + 36 * int(c) for w, c in zip(widths, wide))


@pytest.mark.parametrize("seed", range(6))
def test_mixed_widths_is_the_brute_force_minimum_on_random_rows(seed):
    rng = np.random.default_rng(seed)
    l, k = int(rng.integers(2, 60)), K
    kinds = np.array([0, 1, 2, 3, 4, 5, 0, 0, 0, 0, 0, 0, 0, 0], dtype=np.uint8)
    vals = []
    for r in range(len(kinds)):
        base_bits = int(rng.choice([1, 8, 16, 32, 64, 250]))
        n_wide = int(rng.choice([0, 0, 1, 2, l // 2, l]))
        row = [int.from_bytes(rng.bytes(32), "little") % (1 << base_bits) for _ in range(l)]
        for i in rng.permutation(l)[:n_wide]:
            row[int(i)] = int.from_bytes(rng.bytes(32), "little") % (1 << int(rng.choice([9, 17, 33, 65, 250])))
        vals.append(row)
    rows = rows_of(vals, k)
    rows[:, l:] = 0xFFFFFFFF                                            # pad slots do not count
    widths, wide = amd.mixed_widths(rows, kinds | amd.ROW_DRAW_PAD, l)
    bw, bc = brute_force(rows, kinds, l, k)
    assert [int(w) for w in widths] == bw and [int(c) for c in wide] == bc
    packed = amd.pack_rows_mixed(rows, widths, wide, l)                 # and the rows fit what was chosen
    assert len(packed) == mixed_len(widths, wide, l, k)
    dw, dc = amd.mixed_widths(rows, kinds, l, derive_products=True)
    assert int(dw[3]) == amd.ELEM_PRODUCT and int(dc[3]) == 0 and [int(w) for w in dw[:3]] == bw[:3]


def test_a_tie_takes_the_narrower_base_and_a_full_row_wins_only_where_it_is_not_more_bytes():
    # l = 36: one slot of 2 bits in a bit row: bit base 8 + 36 = 44 bytes, byte base 36 -- byte.  l = 44: 8 + 36 = 44 = 44: the tie -> bits
    for l, want in ((36, (1, 0)), (44, (amd.ELEM_BIT, 1))):
        rows = rows_of([[2] + [1] * (l - 1)])
        w, c = amd.mixed_widths(rows, np.array([0], dtype=np.uint8), l)
        assert (int(w[0]), int(c[0])) == want
    # every slot 250 bits wide, k = l + 1: 8-byte base 8 l + 36 l > 32 k -> the full row; one slot above 8 bytes is an ordinary record
    l = 40
    wide_row = [(1 << 249) + i for i in range(l)]
    w, c = amd.mixed_widths(rows_of([wide_row, [1 << 200] + [1] * (l - 1)], k=l + 1), np.array([0, 0], dtype=np.uint8), l)
    assert [(int(a), int(b)) for a, b in zip(w, c)] == [(32, 0), (amd.ELEM_BIT, 1)]


@pytest.mark.parametrize("name,l,k", [("ref_rows_i32_add_8000.npz", 8000, 8192), ("ref_rows_i32_add_320.npz", 320, 512)])
def test_the_recorded_i32_add_rows(name, l, k):
    """the only real rows there are: the linear row of i32_add is bits with 40 machine words among them"""
    z = np.load(os.path.join(GOLD, name))
    kinds, rows = z["kinds"], z["vals"]
    widths, wide = amd.mixed_widths(rows, kinds, l)
    bw, bc = brute_force(rows, kinds, l, k)
    assert [int(w) for w in widths] == bw and [int(c) for c in wide] == bc
    lin = int(np.nonzero(kinds == 0)[0][0])
    bl = [bit_length(rows[lin, i]) for i in range(l)]
    assert sum(1 for x in bl if x <= 1) == l - 40 and sum(1 for x in bl if x > 32) == 4 and max(bl) <= 64
    # l = 8000: bits + 40 records = 1000 + 1440 = 2440 bytes, the cheapest.  l = 320: bits + 40 records = 40 + 1440 = 1480 bytes, but
    # 4-byte slots + the 4 records above 4 bytes = 1280 + 144 = 1424: at this small l the word base wins
    assert (int(widths[lin]), int(wide[lin])) == ((amd.ELEM_BIT, 40) if l == 8000 else (4, 4))
    assert all(int(w) == amd.ELEM_BIT and int(c) == 0 for r, (w, c) in enumerate(zip(widths, wide)) if r != lin)
    packed = amd.pack_rows_mixed(rows, widths, wide, l)
    narrowest = amd.pack_rows(rows, amd.narrowest_widths(rows, kinds, l), l)
    if l == 8000:
        assert amd.narrow_row_bytes(amd.ELEM_BIT, l, k) + 36 * 40 == 2440
        assert len(packed) == 2440 + 3 * 1000 == 5440
        assert len(narrowest) == 64000 + 3 * 1000 == 67000
    else:
        assert len(packed) == (4 * 320 + 36 * 4) + 12 * 40 == 1904
        assert len(narrowest) == 8 * 320 + 12 * 40 == 3040


def test_the_link_bytes_of_the_timing_tool_follow_from_the_arithmetic():
    """tools/time_mixed_rows.py ships a 2^24-constraint trace of rows with the i32_add profile both ways: what it packs is what the
    format's arithmetic says -- 64 000 bytes per row as narrowest_widths ships it, 2440 as a mixed row"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("time_mixed_rows", os.path.join(os.path.dirname(GOLD), "..", "tools", "time_mixed_rows.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert (tool.expected_link_bytes("a", 1), tool.expected_link_bytes("b", 1)) == (64000, 2440)
    assert (tool.expected_link_bytes("a", 2098), tool.expected_link_bytes("b", 2098)) == (134272000, 5119120)
    data = tool.profile_rows(3, np.random.default_rng(1))
    for leg, w in (("a", 8), ("b", amd.ELEM_BIT)):
        packed, widths, wide = tool.pack_trace(amd, leg, 7, data)
        assert len(packed) == tool.expected_link_bytes(leg, 7) and list(widths) == [w] * 7
        assert wide is None if leg == "a" else list(wide) == [40] * 7
