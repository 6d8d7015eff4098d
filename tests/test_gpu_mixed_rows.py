"""GPU: mixed witness rows (lig_rows_job.wide_per_row) -- narrow rows followed by 36-byte records {uint32 column, 8 uint32 limbs}
of the few slots that do not fit the row's width -- through the single-GPU rows entry, the sharded rows entry and lig_rows_diagnose.
Every expected byte comes from the oracle's prover over the same rows (ol.prove_rows), from the full-width rows entry, or from the
recorded fixtures under tests/golden; the packed bytes are laid out by a packer written out in this file, with garbage wherever the
format says the library does not look."""
import hashlib
import json
import os
import textwrap

import numpy as np
import pytest

import diagnose_ref as dr
import hip_lib
import multirank as mr
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu
GEN = 47
P = ol.P
K, N = 512, 2048
BASES = ("bit", 1, 2, 4, 8)
FIT = {"bit": 1, 1: 8, 2: 16, 4: 32, 8: 64}
LINEAR, QX, QY, QZ = 0, 1, 2, 3


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def limbs(vals):
    """python ints -> (len, 8) uint32"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint32).reshape(-1, 8).copy()


def width_of(amd, base):
    return amd.ELEM_BIT if base == "bit" else base


def narrow_values(base, l, rng):
    """l python ints that fit `base`, the largest such value among them"""
    top = (1 << FIT[base]) - 1
    v = [int(x) % (top + 1) for x in rng.integers(0, 1 << 63, l)] if base != 8 else [int.from_bytes(rng.bytes(8), "little") for _ in range(l)]
    v[1 % l] = top
    return v


def wide_values(base, c):
    """c values that need a record on a row of width `base`: just above the width, 2^64, p - 1, in turn"""
    return [(1 << FIT[base], 1 << 64, P - 1)[j % 3] for j in range(c)]


def columns(c, l, shift=0):
    """c ascending columns < l: column 0 and column l - 1 among them from c = 2 on; c = 1: column 0, or l - 1 with shift"""
    if c == 0:
        return []
    if c == 1:
        return [l - 1 if shift else 0]
    if c == l:
        return list(range(l))
    inner = sorted(set((17 + 31 * j + shift) % (l - 2) + 1 for j in range(c - 2)))
    assert len(inner) == c - 2
    return [0] + inner + [l - 1]


def mixed_row(base, c, l, rng, shift=0):
    """l python ints: a row of width `base` with c wider slots"""
    v = narrow_values(base, l, rng)
    for col, w in zip(columns(c, l, shift), wide_values(base, c)):
        v[col] = w
    return v


def pack(amd, rows, widths, wide, l, garbage=True):
    """the packed bytes of lig_hip.h, written out: per row the narrow part (bits LSB first / little-endian integers, rounded up to 4
    bytes), then the records of the slots that do not fit, ascending.  garbage: the narrow part holds ones under every record column,
    the round-up bytes and the bits past l of a bit row are set -- the library ignores all of them.  A full row is its k x 32 bytes"""
    out = []
    for r, w in enumerate(widths):
        w, c = int(w), int(wide[r])
        if w == amd.ELEM_PRODUCT:
            continue
        if w == 32:
            out.append(np.ascontiguousarray(rows[r], dtype=np.uint32).tobytes())
            continue
        base = "bit" if w == amd.ELEM_BIT else w
        vals = ol.from_limbs(rows[r, :l])
        cols = [i for i, v in enumerate(vals) if v.bit_length() > FIT[base]]
        assert len(cols) == c, (r, len(cols), c)
        for i in cols:
            vals[i] = (1 << FIT[base]) - 1 if garbage else 0
        if base == "bit":
            b = bytearray(np.packbits(np.array(vals, dtype=np.uint8), bitorder="little").tobytes())
            if garbage and l % 8:
                b[-1] |= (0xFF << (l % 8)) & 0xFF
        else:
            b = bytearray(b"".join(v.to_bytes(w, "little") for v in vals))
        b += bytes([0xA5 if garbage else 0]) * (-len(b) % 4)
        assert len(b) == amd.narrow_row_bytes(w, l, rows.shape[1])
        for i in cols:
            b += int(i).to_bytes(4, "little") + np.ascontiguousarray(rows[r, i], dtype=np.uint32).tobytes()
        out.append(bytes(b))
    return np.frombuffer(b"".join(out), dtype=np.uint8).copy()


def oracle_frame(l, R):
    """the oracle's pads and masks for R rows that each own k - l stream elements (an all-linear job of as many rows gives them)"""
    job = ol.make_job(l, K, N, 192, R * l, 0, generated_at=GEN, threads=8)
    rows, mc, ml, mq = ol.form_rows(job)
    return rows.copy(), (mc, ml, mq)


def flagged(amd, kinds, rows, l):
    """(kinds | ROW_DRAW_PAD, the rows with garbage in the pad slots the library draws)"""
    kk = np.asarray(kinds, dtype=np.uint8).copy()
    kk[kk <= 3] |= amd.ROW_DRAW_PAD
    msgs = rows.copy()
    msgs[:, l:] = 0x5A5A5A5A
    return kk, msgs


def rands_for(R, seed):
    rng = np.random.default_rng(seed)
    rands = rng.integers(0, 1 << 32, (R, K, 8), dtype=np.uint64).astype(np.uint32)
    rands[:, :, 7] &= 0x0FFFFFFF
    return rands


def prove_full(c, kk, msgs, rands, **kw):
    tr, keep = c.rows_begin(kk, msgs, generated_at=GEN, **kw)
    root, seed1 = c.rows_commit(tr)
    proof, _ = c.rows_prove(tr, rands, None)
    c.trace_destroy(tr)
    return root, seed1, proof


def every_width_trace(amd, l, shift):
    """20 linear rows -- every base width x {0, 1, 3, l} records -- and a triple whose x, y and z rows are all mixed -> kinds, rows
    (data slots only: the frame comes later), widths, counts.  shift: other columns, other narrow values, the same counts"""
    rng = np.random.default_rng(100 + shift)
    kinds, vals, widths, wide = [], [], [], []
    for base in BASES:
        for c in (0, 1, 3, l):
            kinds.append(LINEAR); widths.append(width_of(amd, base)); wide.append(c)
            vals.append(mixed_row(base, c, l, rng, shift))
    x, y = mixed_row("bit", 3, l, rng, shift), mixed_row(2, 1, l, rng, shift)
    z = [a * b % P for a, b in zip(x, y)]
    zc = sum(1 for v in z if v.bit_length() > 64)
    kinds += [QX, QY, QZ]; widths += [amd.ELEM_BIT, 2, 8]; wide += [3, 1, zc]
    vals += [x, y, z]
    return np.array(kinds, dtype=np.uint8), vals, np.array(widths, dtype=np.uint8), np.array(wide, dtype=np.uint32)


@pytest.mark.parametrize("l", [320, 317])
def test_every_base_width_with_0_1_3_and_l_records_equals_oracle_and_full_width(amd, l):
    """host rows, device rows, and lig_rows_restart from the other side with a second trace of the same counts but other columns and
    values: root, stage-1 seed and envelope of the oracle's prover and of the full-width entry.  l = 317: bit and byte rows need the
    round-up before their first record"""
    frame, masks = oracle_frame(l, 23)
    traces = []
    for shift in (0, 5):
        kinds, vals, widths, wide = every_width_trace(amd, l, shift)
        rows = frame.copy()
        for r, v in enumerate(vals):
            rows[r, :l] = limbs(v)
        traces.append((kinds, rows, widths, wide))
    (kinds, rows_a, widths, wide), (_, rows_b, widths_b, wide_b) = traces
    assert list(widths) == list(widths_b) and list(wide) == list(wide_b)           # one shape
    assert not np.array_equal(rows_a[:, :l], rows_b[:, :l])
    R = len(kinds)
    rands = rands_for(R, 1)
    want = [ol.prove_rows(l, K, N, 192, kinds, rows, *masks, rands, None, generated_at=GEN, threads=8) for rows in (rows_a, rows_b)]
    assert want[0]["proof"] != want[1]["proof"]
    kk, msgs_a = flagged(amd, kinds, rows_a, l)
    _, msgs_b = flagged(amd, kinds, rows_b, l)
    packed = [pack(amd, m, widths, wide, l) for m in (msgs_a, msgs_b)]
    for m, p in zip((msgs_a, msgs_b), packed):                                      # the binding's packer lays out the same bytes, garbage aside
        assert amd.pack_rows_mixed(m, widths, wide, l).tobytes() == pack(amd, m, widths, wide, l, garbage=False).tobytes()
        assert len(p) == sum(amd.narrow_row_bytes(w, l, K) + 36 * int(c) for w, c in zip(widths, wide))
    c = amd.Context(l, K, N)
    try:
        for i, m in enumerate((msgs_a, msgs_b)):
            root, seed1, full = prove_full(c, kk, m, rands)
            assert (root, seed1, full) == (want[i]["root"], want[i]["stage1_seed"], want[i]["proof"])
        dev = [c.upload(p) for p in packed]
        for where in ("host", "device"):
            if where == "device":
                tr, keep = c.rows_begin(kk, dev[0], on_device=True, generated_at=GEN, elem_bytes=widths, wide_per_row=wide)
            else:
                tr, keep = c.rows_begin(kk, packed[0], generated_at=GEN, elem_bytes=widths, wide_per_row=wide)
            assert c.rows_commit(tr) == (want[0]["root"], want[0]["stage1_seed"]), where
            # the second trace arrives from the other side while the first is proved
            if where == "device":
                c.rows_restart(tr, packed[1].ctypes.data, on_device=False)
            else:
                c.rows_restart(tr, dev[1], on_device=True)
            proof, _ = c.rows_prove(tr, rands, None)
            assert proof == want[0]["proof"], where
            assert c.rows_commit(tr) == (want[1]["root"], want[1]["stage1_seed"]), where
            proof, _ = c.rows_prove(tr, rands, None)
            assert proof == want[1]["proof"], where
            # and the first again from the same side
            c.rows_restart(tr, dev[0] if where == "device" else packed[0].ctypes.data, on_device=where == "device")
            assert c.rows_commit(tr) == (want[0]["root"], want[0]["stage1_seed"]), where
            proof, _ = c.rows_prove(tr, rands, None)
            assert proof == want[0]["proof"], where
            c.trace_destroy(tr)
    finally:
        c.close()


def stage1_chunks(R, big=512, head=128, tail=96):
    """the library's stage-1 chunk schedule at its defaults (chunk_schedule in prover_common.hpp)"""
    out, b = [], 0
    if head and R > head + tail:
        out.append((0, head))
        b = head
    stop = R - tail if tail and R > b + tail else R
    while b < stop:
        e = min(stop, b + big)
        out.append((b, e))
        b = e
    if b < R:
        out.append((b, R))
    return out


def test_mixed_rows_on_both_sides_of_every_stage1_chunk_boundary(amd):
    """530 rows, host rows through the default upload path: the last row of every stage-1 chunk and the first row of the next are
    mixed, so the records of the one end an upload chunk and the narrow part of the other begins one"""
    l, R = 320, 530
    chunks = stage1_chunks(R)
    assert len(chunks) == 3
    edge = sorted(set([e - 1 for _, e in chunks[:-1]] + [b for b, _ in chunks[1:]]))
    assert edge == [127, 128, 433, 434]
    rng = np.random.default_rng(2)
    rows, masks = oracle_frame(l, R)
    kinds = np.zeros(R, dtype=np.uint8)
    widths = np.full(R, amd.ELEM_BIT, dtype=np.uint8)
    wide = np.zeros(R, dtype=np.uint32)
    for r in range(R):
        base, c = "bit", 0
        if r in edge:
            base, c = BASES[edge.index(r) % len(BASES)], (3, l, 1, 40)[edge.index(r)]
        elif r % 7 == 3:
            base = 1
        widths[r], wide[r] = width_of(amd, base), c
        rows[r, :l] = limbs(mixed_row(base, c, l, rng, shift=r) if c not in (40,) else
                            [v if i % 8 else (1 << 40) + i for i, v in enumerate(narrow_values(base, l, rng))])
    rands = rands_for(R, 3)
    want = ol.prove_rows(l, K, N, 192, kinds, rows, *masks, rands, None, generated_at=GEN, threads=8)
    kk, msgs = flagged(amd, kinds, rows, l)
    packed = pack(amd, msgs, widths, wide, l)
    c = amd.Context(l, K, N)
    try:
        assert prove_full(c, kk, msgs, rands) == (want["root"], want["stage1_seed"], want["proof"])
        assert prove_full(c, kk, packed, rands, elem_bytes=widths, wide_per_row=wide) == (want["root"], want["stage1_seed"], want["proof"])
    finally:
        c.close()


@pytest.mark.parametrize("name,nbytes", [("i32_add_8000", 2440 + 3 * 1000), ("i32_add_320", (4 * 320 + 4 * 36) + 12 * 40)])
def test_the_recorded_i32_add_rows_ship_mixed(amd, name, nbytes):
    """the reference constraint backend's rows for i32_add, shipped as mixed_widths chooses: the fixture's own root and seed, the
    full-width entry's envelope, and the bytes of the arithmetic: l = 8000: the linear row as bits + 40 records = 2440 bytes next to
    three 1000-byte bit rows; l = 320: 4-byte slots + the 4 records above 4 bytes next to twelve 40-byte bit rows"""
    z = np.load(os.path.join(GOLD, "ref_rows_%s.npz" % name))
    m = json.loads(str(z["meta"]))
    l, k, n = m["l"], m["k"], m["n"]
    key = bytes.fromhex(m["encoding_seed"])
    kinds, vals, rands, constsum = z["kinds"], z["vals"], z["rands"], z["constsum"].tobytes()
    kk = kinds | amd.ROW_DRAW_PAD
    msgs = vals.copy()
    msgs[:, l:] = 0xDEADBEEF
    widths, wide = amd.mixed_widths(vals, kinds, l)
    assert int(wide.sum()) > 0
    packed = pack(amd, msgs, widths, wide, l)
    assert len(packed) == nbytes
    assert amd.pack_rows_mixed(msgs, widths, wide, l).tobytes() == pack(amd, msgs, widths, wide, l, garbage=False).tobytes()
    c = amd.Context(l, k, n)
    try:
        tr, keep = c.rows_begin(kk, msgs, encoding_seed=key, generated_at=m["generated_at"])
        c.rows_commit(tr)
        full, _ = c.rows_prove(tr, rands, constsum)
        c.trace_destroy(tr)
        assert hashlib.sha256(full).hexdigest() == m["oracle_proof_sha256"]
        tr, keep = c.rows_begin(kk, packed, encoding_seed=key, generated_at=m["generated_at"], elem_bytes=widths, wide_per_row=wide)
        root, seed1 = c.rows_commit(tr)
        assert root.hex() == m["oracle_root"] and seed1.hex() == m["oracle_stage1_seed"]
        proof, info = c.rows_prove(tr, rands, constsum)
        assert [info.valid_code, info.valid_linear, info.valid_quad] == [1, 1, 1]
        assert proof == full
        c.trace_destroy(tr)
    finally:
        c.close()


def derived_trace(amd, l):
    """triples whose z is derived (LIG_ELEM_PRODUCT) from mixed operands: x mixed, y mixed, both mixed -- a record in x over a bit
    of y, over a record of y, and p - 1 times p - 1 -- with linear rows between them -> kinds, values, widths, counts"""
    rng = np.random.default_rng(9)
    kinds, vals, widths, wide = [], [], [], []
    def triple(x, wx, y, wy):
        for kd, v, w in ((QX, x, wx), (QY, y, wy)):
            base = "bit" if w == amd.ELEM_BIT else w
            kinds.append(kd); vals.append(v); widths.append(w); wide.append(sum(1 for a in v if a.bit_length() > FIT[base]))
        kinds.append(QZ); vals.append([a * b % P for a, b in zip(x, y)]); widths.append(amd.ELEM_PRODUCT); wide.append(0)
    # x mixed (bits + records), y plain bits: a record of x over a 1 bit and over a 0 bit of y
    x, y = mixed_row("bit", 3, l, rng), narrow_values("bit", l, rng)
    y[0], y[l - 1] = 1, 0
    triple(x, amd.ELEM_BIT, y, amd.ELEM_BIT)
    kinds.append(LINEAR); vals.append(mixed_row(1, 3, l, rng)); widths.append(1); wide.append(3)
    # x plain 8 bytes (2^64 - 1 among them), y mixed bytes
    x, y = narrow_values(8, l, rng), mixed_row(1, 3, l, rng, shift=2)
    triple(x, 8, y, 1)
    # both mixed: p - 1 times p - 1 in column 5, a record of x against a narrow slot of y in column 6 and the reverse in column 7
    x, y = narrow_values(4, l, rng), narrow_values("bit", l, rng)
    x[5], y[5] = P - 1, P - 1
    x[6], y[6] = (1 << 200) + 3, 1
    x[7], y[7] = 0xFFFFFFFF, 1 << 64
    x[l - 1], y[l - 1] = P - 2, P - 1
    triple(x, 4, y, amd.ELEM_BIT)
    # every slot of both operands a record
    triple(mixed_row(2, l, l, rng), 2, mixed_row("bit", l, l, rng), amd.ELEM_BIT)
    return np.array(kinds, dtype=np.uint8), vals, np.array(widths, dtype=np.uint8), np.array(wide, dtype=np.uint32)


@pytest.mark.parametrize("l", [320, 317])
def test_derived_products_of_mixed_operands(amd, l):
    """the QZ rows are LIG_ELEM_PRODUCT and are not shipped: the envelope of the full-width entry and of the oracle over rows whose z
    was computed in Python integers"""
    kinds, vals, widths, wide = derived_trace(amd, l)
    R = len(kinds)
    rows, masks = oracle_frame(l, R)
    for r, v in enumerate(vals):
        rows[r, :l] = limbs(v)
    rands = rands_for(R, 4)
    want = ol.prove_rows(l, K, N, 192, kinds, rows, *masks, rands, None, generated_at=GEN, threads=8)
    kk, msgs = flagged(amd, kinds, rows, l)
    blind = msgs.copy()
    blind[kinds == QZ] = 0xDEADBEEF                                             # nothing of the expected product reaches the library
    packed = pack(amd, blind, widths, wide, l)
    c = amd.Context(l, K, N)
    try:
        assert prove_full(c, kk, msgs, rands) == (want["root"], want["stage1_seed"], want["proof"])
        assert prove_full(c, kk, packed, rands, elem_bytes=widths, wide_per_row=wide) == (want["root"], want["stage1_seed"], want["proof"])
        assert prove_full(c, kk, c.upload(packed), rands, on_device=True, elem_bytes=widths, wide_per_row=wide) == (want["root"], want["stage1_seed"], want["proof"])
    finally:
        c.close()


def test_diagnose_names_the_constraint_of_a_changed_record(amd):
    """lig_rows_diagnose reads the expanded matrix: one record value of a shipped z row changed -> exactly that (triple, column)"""
    l = 320
    kinds, vals, widths, wide = every_width_trace(amd, l, 0)
    R = len(kinds)
    rows, _ = oracle_frame(l, R)
    for r, v in enumerate(vals):
        rows[r, :l] = limbs(v)
    assert dr.quad_violations(kinds, rows, l) == []
    zrow = R - 1
    col = [i for i, v in enumerate(vals[zrow]) if v.bit_length() > 64][-1]
    rows[zrow, col, 5] ^= 1 << 3                                                # inside a record of the z row
    want = dr.quad_violations(kinds, rows, l)
    assert [(x, y, z, i) for x, y, z, i, _ in want] == [(R - 3, R - 2, R - 1, col)]
    kk, msgs = flagged(amd, kinds, rows, l)
    c = amd.Context(l, K, N)
    try:
        tr, keep = c.rows_begin(kk, pack(amd, msgs, widths, wide, l), generated_at=GEN, elem_bytes=widths, wide_per_row=wide)
        c.rows_commit(tr)
        info, lin, quad = c.rows_diagnose(tr, None)
        assert (info.n_quad_bad, info.n_quad_reported) == (1, 1)
        assert dr.got_quad(quad) == dr.quad_records(want)
        c.trace_destroy(tr)
    finally:
        c.close()


def small_mixed_trace(amd, l):
    """three linear rows: bits with 3 records, bytes, 4-byte words with 2 records -> kinds, rows (oracle frame), masks, widths, counts"""
    rng = np.random.default_rng(6)
    rows, masks = oracle_frame(l, 3)
    widths, wide = np.array([amd.ELEM_BIT, 1, 4], dtype=np.uint8), np.array([3, 0, 2], dtype=np.uint32)
    for r, (base, c) in enumerate((("bit", 3), (1, 0), (4, 2))):
        rows[r, :l] = limbs(mixed_row(base, c, l, rng))
    return np.zeros(3, dtype=np.uint8), rows, masks, widths, wide


def record_offsets(amd, widths, wide, l):
    """byte offset of the column word of every record: {row: [offsets]}"""
    out, off = {}, 0
    for r, (w, c) in enumerate(zip(widths, wide)):
        off += amd.narrow_row_bytes(w, l, K)
        out[r] = [off + 36 * j for j in range(int(c))]
        off += 36 * int(c)
    return out


def set_column(packed, off, col):
    bad = packed.copy()
    bad[off:off + 4] = np.frombuffer(int(col).to_bytes(4, "little"), dtype=np.uint8)
    return bad


def test_records_that_leave_the_row_or_the_order_are_refused(amd):
    """host rows: a column >= l, columns out of order -> LIG_E_ARG from lig_rows_begin and lig_rows_restart, before anything is copied.
    Device rows: a column >= l is not written (the kernel's guard) and lig_rows_commit returns LIG_E_ARG; the trace stays usable"""
    l = 317
    kinds, rows, masks, widths, wide = small_mixed_trace(amd, l)
    rands = rands_for(3, 7)
    want = ol.prove_rows(l, K, N, 192, kinds, rows, *masks, rands, None, generated_at=GEN, threads=8)
    kk, msgs = flagged(amd, kinds, rows, l)
    good = pack(amd, msgs, widths, wide, l)
    offs = record_offsets(amd, widths, wide, l)
    cols0 = columns(3, l)
    bad = {"column == l": set_column(good, offs[0][2], l), "column 2^32 - 1": set_column(good, offs[2][1], 0xFFFFFFFF),
           "descending": set_column(good, offs[0][1], l - 1), "twice the same": set_column(good, offs[0][1], cols0[0])}
    c = amd.Context(l, K, N)
    try:
        tr, keep = c.rows_begin(kk, good, generated_at=GEN, elem_bytes=widths, wide_per_row=wide)
        for why, p in bad.items():
            with pytest.raises(amd.LigError, match=r"\(-1\).*wide slot"):
                c.rows_begin(kk, p, generated_at=GEN, elem_bytes=widths, wide_per_row=wide)
            with pytest.raises(amd.LigError, match=r"\(-1\).*wide slot"):
                c.rows_restart(tr, p.ctypes.data, on_device=False)
        assert c.rows_commit(tr) == (want["root"], want["stage1_seed"])          # the refused restarts have not touched the loaded rows
        proof, _ = c.rows_prove(tr, rands, None)
        assert proof == want["proof"]
        c.trace_destroy(tr)
        # counts where the format does not allow them: decided before anything is launched, device rows included
        d_good = c.upload(good)
        for w2, c2 in (([amd.ELEM_BIT, 32, 4], [3, 1, 2]), ([amd.ELEM_BIT, 1, 4], [l + 1, 0, 2])):
            with pytest.raises(amd.LigError, match=r"\(-1\).*wide_per_row"):
                c.rows_begin(kk, d_good, on_device=True, generated_at=GEN, elem_bytes=np.array(w2, dtype=np.uint8), wide_per_row=np.array(c2, dtype=np.uint32))
        with pytest.raises(amd.LigError, match=r"\(-1\).*wide_per_row"):
            c.rows_begin(kk, msgs, generated_at=GEN, wide_per_row=wide)           # without elem_bytes
        # device rows: the refusal comes from the commit; good rows then prove on the same trace
        for why in ("column == l", "column 2^32 - 1"):
            tr, keep = c.rows_begin(kk, c.upload(bad[why]), on_device=True, generated_at=GEN, elem_bytes=widths, wide_per_row=wide)
            with pytest.raises(amd.LigError, match=r"\(-1\).*wide slot"):
                c.rows_commit(tr)
            c.rows_restart(tr, d_good, on_device=True)
            assert c.rows_commit(tr) == (want["root"], want["stage1_seed"]), why
            proof, _ = c.rows_prove(tr, rands, None)
            assert proof == want["proof"], why
            c.trace_destroy(tr)
    finally:
        c.close()


def test_sharded_entry_refuses_bad_records_before_any_collective(amd):
    """one rank, in-process communicator: bad host records at begin and at restart, a device record with a column >= l at begin"""
    l = 317
    kinds, rows, masks, widths, wide = small_mixed_trace(amd, l)
    rands = rands_for(3, 7)
    want = ol.prove_rows(l, K, N, 192, kinds, rows, *masks, rands, None, generated_at=GEN, threads=8)
    kk, msgs = flagged(amd, kinds, rows, l)
    good = pack(amd, msgs, widths, wide, l)
    offs = record_offsets(amd, widths, wide, l)
    bad = [set_column(good, offs[0][2], l), set_column(good, offs[2][0], l - 1)]     # column == l; out of order
    c = amd.Context(l, K, N)
    comm = c.ipc_comm("/lig_mx_" + mr.fresh_tag(), 0, 1)
    try:
        for p in bad:
            with pytest.raises(amd.LigError, match=r"\(-1\).*wide slot"):
                c.shard_rows_begin(kk, p, 0, 1, comm, generated_at=GEN, elem_bytes=widths, wide_per_row=wide)
        with pytest.raises(amd.LigError, match=r"\(-1\).*wide slot"):
            c.shard_rows_begin(kk, c.upload(bad[0]), 0, 1, comm, on_device=True, generated_at=GEN, elem_bytes=widths, wide_per_row=wide)
        sh = c.shard_rows_begin(kk, good, 0, 1, comm, generated_at=GEN, elem_bytes=widths, wide_per_row=wide)
        for p in bad:
            with pytest.raises(amd.LigError, match=r"\(-1\).*wide slot"):
                c.shard_rows_restart(sh, p)
        c.shard_rows_restart(sh, good)
        assert c.shard_rows_commit(sh) == (want["root"], want["stage1_seed"])
        proof, _ = c.shard_rows_prove(sh, rands, None)
        assert proof == want["proof"]
        c.shard_destroy(sh)
    finally:
        c.ipc_comm_destroy(comm)
        c.close()


MIXED_SHARD_WORKER = textwrap.dedent('''
    import hashlib, importlib.util, json, os, sys
    import numpy as np
    root, l, mode = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    sys.path.insert(0, os.path.join(root, "tests"))
    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, "ligero-prover_amd", rel))
        m = importlib.util.module_from_spec(spec); sys.modules[name] = m; spec.loader.exec_module(m); return m
    pkg = load("ligero_prover_amd", "__init__.py")
    dist = load("lig_dist", "dist.py")
    import oracle_lib as ol
    import test_gpu_mixed_rows as tm
    g = dist.Group("gloo")
    ctx = pkg.Context(l, tm.K, tm.N, device=0)
    # every rank plays the same deterministic guest (all rows, kinds, counts, randomness rows) and keeps its slice
    kinds, widths, wide, traces, masks, rands = tm.sharded_traces(pkg, l)
    rounds, b = pkg.shard_rows_plan(kinds, g.world)
    mine = pkg.local_rows_of(b, g.rank, g.world)
    kk = kinds | pkg.ROW_DRAW_PAD
    packed = [tm.pack(pkg, tm.flagged(pkg, kinds, rows, l)[1][mine], widths[mine], wide[mine], l) for rows in traces]
    comm = g.make_comm(pkg, ctx)
    dev = [ctx.upload(p) if p.size else ctx.malloc(32) for p in packed]
    src = dev if mode == "device" else packed
    sh = ctx.shard_rows_begin(kk, src[0], g.rank, g.world, comm, on_device=mode == "device", generated_at=tm.GEN, elem_bytes=widths, wide_per_row=wide)
    out = []
    for rep in (0, 1, 0):                            # lig_shard_rows_restart: other columns and values under the same counts, and back
        if out:
            ctx.shard_rows_restart(sh, src[rep], on_device=mode == "device")
        ctx.shard_rows_commit(sh)
        proof, info = ctx.shard_rows_prove(sh, rands[mine], None)
        out.append(proof)
    ctx.shard_destroy(sh)
    ref = oref = None
    if g.rank == 0:                                  # the unsharded rows entry at full width, and the oracle's prover
        ref, oref = [], []
        for rows in traces:
            tr, keep = ctx.rows_begin(kk, tm.flagged(pkg, kinds, rows, l)[1], generated_at=tm.GEN)
            ctx.rows_commit(tr)
            ref.append(ctx.rows_prove(tr, rands, None)[0])
            ctx.trace_destroy(tr)
            oref.append(ol.prove_rows(l, tm.K, tm.N, 192, kinds, rows, *masks, rands, None, generated_at=tm.GEN, threads=4)["proof"])
    digs = [g.gather_digests(hashlib.sha256(p).digest()) for p in out]
    print(json.dumps({"rank": g.rank, "local_rows": len(mine), "local_records": int(wide[mine].sum()), "differ": out[0] != out[1], "back": out[0] == out[2],
                      "all_equal": all(len(set(d)) == 1 for d in digs),
                      "equals_rows_prove": None if ref is None else [ref[0] == out[0], ref[1] == out[1]],
                      "equals_oracle": None if oref is None else [oref[0] == out[0], oref[1] == out[1]]}))
    g.close(); ctx.close()
''')


def sharded_traces(amd, l):
    """the rows of test 1 three times over (69 rows: enough for every rank of two to hold mixed rows, a derived triple among them)
    -> kinds, widths, counts, [rows of trace A, rows of trace B], masks, rands"""
    parts = [every_width_trace(amd, l, s) for s in (0, 5)]
    kinds, _, widths, wide = parts[0]
    reps = 3
    frame, masks = oracle_frame(l, reps * len(kinds))
    traces = []
    for _, vals, _, _ in parts:
        rows = frame.copy()
        for rep in range(reps):
            for r, v in enumerate(vals):
                rows[rep * len(kinds) + r, :l] = limbs(v)
        traces.append(rows)
    return np.tile(kinds, reps), np.tile(widths, reps), np.tile(wide, reps), traces, masks, rands_for(reps * len(kinds), 8)


@pytest.mark.parametrize("world,l,mode", [(1, 317, "host"), (2, 320, "host"), (2, 317, "device")])
def test_sharded_mixed_rows_equal_rows_prove_and_oracle(tmp_path, world, l, mode):
    """lig_shard_rows_* with wide_per_row: each rank passes the counts of all rows and its own rows packed back to back; every rank's
    envelope == lig_rows_prove of the whole trace at full width == the oracle's, also after lig_shard_rows_restart"""
    script = tmp_path / "mixed_shard_worker.py"
    script.write_text(MIXED_SHARD_WORKER)
    outs = mr.run_ranks(mr.python_argv(script, ROOT, l, mode), world, mr.rendezvous_env(world, "ipc"), timeout=300)
    outs = sorted((mr.last_json(o) for o, _ in outs), key=lambda d: d["rank"])
    assert all(o["differ"] and o["back"] and o["all_equal"] and o["local_records"] > 0 for o in outs), outs
    assert outs[0]["equals_rows_prove"] == [True, True] and outs[0]["equals_oracle"] == [True, True], outs


# ---- the row-batching shim (include/lig_hip_row_batcher.hpp) with hip_proof_meta::wide_slots
def build_mixed_batcher():
    import subprocess
    mod = hip_lib.load()
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    odir = os.path.join(ROOT, "oracle")
    ol.build()
    src, exe = os.path.join(ROOT, "tests", "cpp", "mixed_batcher_prog.cpp"), os.path.join(ROOT, "tests", "cpp", "mixed_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def test_row_batcher_ships_mixed_rows_on_one_gpu():
    """wide_slots next to narrow_rows + narrowest: fewer bytes than narrowest alone on a trace whose bit rows hold a few machine
    words, the same (the oracle's) envelope, also on the restarted trace; with wide_slots off -- and with it on but narrowest off --
    the shipped bytes are today's.  Both byte counts equal the arithmetic of the format worked out in the program"""
    import subprocess
    p = subprocess.run([build_mixed_batcher()], capture_output=True, timeout=300)
    assert p.returncode == 0, (p.stdout.decode()[-3000:], p.stderr.decode()[-3000:])
    out = mr.last_json(p.stdout.decode())
    assert out["equals_oracle"] is True and out["mixed_rows"] > 0, out
    assert out["shipped_narrowest"] == out["want_narrowest"] and out["shipped_mixed"] == out["want_mixed"] == out["shipped_mixed_again"], out
    assert out["shipped_mixed"] * 4 < out["shipped_narrowest"], out
    assert out["shipped_without_narrowest"] > out["shipped_narrowest"], out


def test_row_batcher_ships_mixed_rows_on_every_rank_of_a_sharded_trace():
    exe = build_mixed_batcher()
    name = "/lig_mb_" + mr.fresh_tag()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = mr.run_ranks(lambda r: [exe, str(r), "2", name], 2, env, timeout=300)
    outs = [mr.last_json(o) for o, _ in outs]
    for o in outs:
        assert o["equals_oracle"] is True and o["local_rows"] and o["mixed_rows"], outs
        assert o["shipped_narrowest"] == o["want_narrowest"] and o["shipped_mixed"] == o["want_mixed"] == o["shipped_mixed_again"], outs
        assert o["shipped_mixed"] < o["shipped_narrowest"], outs


def test_a_job_that_does_not_announce_the_member_is_read_as_before(amd):
    """a caller compiled before wide_per_row existed passes a struct that ends at elem_bytes, with reserved = 0: what lies behind it
    is not read.  A narrow job with reserved = 0 and an unreadable pointer in the member's place proves the oracle's envelope"""
    import ctypes as C
    l = 317
    kinds, rows, masks, widths, wide = small_mixed_trace(amd, l)
    rows[:, :l, 1:] = 0
    rows[:, :l, 0] &= 1                                                          # plain bit rows
    rands = rands_for(3, 7)
    want = ol.prove_rows(l, K, N, 192, kinds, rows, *masks, rands, None, generated_at=GEN, threads=8)
    kk, msgs = flagged(amd, kinds, rows, l)
    widths = np.full(3, amd.ELEM_BIT, dtype=np.uint8)
    packed = amd.pack_rows(msgs, widths, l)
    c = amd.Context(l, K, N)
    try:
        job = amd.RowsJob()
        job.rows, job.kinds, job.msgs, job.msgs_on_device = 3, kk.ctypes.data, packed.ctypes.data, 0
        for i in range(32):
            job.encoding_seed[i] = i
        job.generated_at = GEN
        job.version = b"1.5.0"
        job.set_public_args(None)
        job.elem_bytes = widths.ctypes.data
        job.reserved = 0
        job.wide_per_row = 0x10                                                  # stack garbage of an old caller: never dereferenced
        tr = C.c_void_p()
        c.check(c.L.lig_rows_begin(c.h, C.byref(job), C.byref(tr)))
        assert c.rows_commit(tr) == (want["root"], want["stage1_seed"])
        proof, _ = c.rows_prove(tr, rands, None)
        assert proof == want["proof"]
        c.trace_destroy(tr)
    finally:
        c.close()
