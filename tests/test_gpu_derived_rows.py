"""GPU: derived product rows (lig_rows_job.elem_bytes = LIG_ELEM_PRODUCT).  The z row of a quadratic triple is not shipped: the
library forms x[i] * y[i] mod p on the device from the PACKED x and y rows and draws the row's pads.  Every expected byte comes
from the oracle's prover (ol.prove_rows) and from the full-width rows entry over rows whose z was computed in Python integers --
never from the derived path itself.  Single-GPU entry, sharded entry, the row-batching shim, and the refusals of both entries."""
import hashlib
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import hip_lib
import multirank as mr
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GEN = 43
P = ol.P
# operand classes of a triple (x, y): what each row is shipped as
PAIRS = (("bit", "bit"), (4, 4), (8, 8), (8, 32), ("bit", 32), (32, 32), (1, 2), (32, 8), (2, "bit"), (32, 4))


def stage1_chunks(R, big=512, head=128, tail=96):
    """the library's stage-1 chunk schedule at its defaults (chunk_schedule in prover_common.hpp: LIG_CHUNK, LIG_S1_HEAD,
    LIG_S1_TAIL): a 128-row head chunk and a 96-row tail chunk around 512-row chunks, the head only when R > head + tail"""
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


def layout(R, forced):
    """kinds of R rows: a triple starts at every row of `forced`; in between linear rows and triples alternate"""
    kinds, r, triple = [], 0, False
    forced = sorted(forced)
    while r < R:
        nxt = min([f for f in forced if f >= r], default=R)
        if r == nxt and r + 3 <= R:
            kinds += [1, 2, 3]
            r += 3
            continue
        if triple and r + 3 <= nxt:
            kinds += [1, 2, 3]
            r += 3
        else:
            kinds += [0]
            r += 1
        triple = not triple
    return np.array(kinds, dtype=np.uint8)


def limbs(vals):
    """python ints -> (len, 8) uint32"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint32).reshape(-1, 8).copy()


def operand(cls, l, rng):
    """(l, 8) uint32: data slots whose narrowest width is exactly `cls`"""
    out = np.zeros((l, 8), dtype=np.uint32)
    if cls == "bit":
        out[:, 0] = rng.integers(0, 2, l)
        out[0, 0] = 1
    elif cls in (1, 2, 4):
        out[:, 0] = rng.integers(0, 1 << (8 * cls), l, dtype=np.uint64)
        out[0, 0] = (1 << (8 * cls)) - 1
    elif cls == 8:
        out[:, :2] = rng.integers(0, 1 << 32, (l, 2), dtype=np.uint64)
        out[0, :2] = 0xFFFFFFFF                                        # x = y = 2^64 - 1 in an 8 x 8 triple: the largest plain product
        out[1 % l, :2] = (0, 1)
    else:
        out[:] = rng.integers(1, 1 << 32, (l, 8), dtype=np.uint64)     # all eight limbs populated
        out[:, 7] = (out[:, 7] & 0x0FFFFFFF) | 0x08000000              # 2^251 <= v < 2^252 < p: canonical
    return out


def build_trace(l, k, n, kinds, seed=11, lin_classes=("bit", 1, 2, 4, 8, 32)):
    """-> (rows, masks, rands, pairs): the oracle's pads and masks (every LINEAR / QX / QY / QZ row owns the next k - l stream elements
    whatever its kind: an all-linear job of as many rows gives them), data slots of the given kinds; z = x * y mod p in Python ints"""
    R = len(kinds)
    job = ol.make_job(l, k, n, 192, R * l, 0, generated_at=GEN, threads=8)
    rows, mc, ml, mq = ol.form_rows(job)
    rows = rows.copy()
    rng = np.random.default_rng(seed)
    pairs, j, t = {}, 0, 0
    for r in range(R):
        if kinds[r] == 0:
            rows[r, :l] = operand(lin_classes[j % len(lin_classes)], l, rng)
            j += 1
        elif kinds[r] == 1:
            cx, cy = PAIRS[t % len(PAIRS)]
            t += 1
            x, y = ol.from_limbs(operand(cx, l, rng)), ol.from_limbs(operand(cy, l, rng))
            if (cx, cy) == (32, 32):
                x[0], y[0] = P - 1, P - 1
                x[1 % l], y[1 % l] = P - 1, 2
                x[2 % l] = 0
                y[3 % l] = 0
            z = [a * b % P for a, b in zip(x, y)]
            for d, v in enumerate((x, y, z)):
                rows[r + d, :l] = limbs(v)
            pairs[r] = (cx, cy)
    rands = rng.integers(0, 1 << 32, (R, k, 8), dtype=np.uint64).astype(np.uint32)
    rands[:, :, 7] &= 0x0FFFFFFF
    return rows, (mc, ml, mq), rands, pairs


def ship(amd, kinds, rows, l):
    """-> (kinds | ROW_DRAW_PAD, widths with every QZ row derived, packed bytes, the full-width matrix with garbage in the pad slots
    of flagged rows): the z rows are WIPED before packing, so nothing of the expected product can reach the library"""
    kk = kinds.copy()
    kk[kinds <= 3] |= amd.ROW_DRAW_PAD
    widths = amd.narrowest_widths(rows, kinds, l, derive_products=True)
    wide = rows.copy()
    wide[kinds <= 3, l:] = 0x5A5A5A5A
    blind = wide.copy()
    blind[kinds == 3] = 0xDEADBEEF
    packed = amd.pack_rows(blind, widths, l)
    return kk, widths, wide, packed


def packed_bytes(amd, widths, l, k):
    n = 0
    for w in widths:
        w = int(w)
        n += 0 if w == amd.ELEM_PRODUCT else k * 32 if w == 32 else ((l + 31) // 32 * 4 if w == amd.ELEM_BIT else (l * w + 3) // 4 * 4)
    return n


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def run_every_path(amd, l, k, n, kinds, rows, masks, rands):
    R = len(kinds)
    want = ol.prove_rows(l, k, n, 192, kinds, rows, *masks, rands, None, generated_at=GEN, threads=8)
    assert want["valid"][2] == 1                                           # the Python z rows are the products: the oracle's own quadratic check
    kk, widths, wide, packed = ship(amd, kinds, rows, l)
    assert [r for r in range(R) if widths[r] == amd.ELEM_PRODUCT] == [r for r in range(R) if kinds[r] == 3]
    assert len(packed) == packed_bytes(amd, widths, l, k)                  # msgs is exactly as long as the packed layout says
    c = amd.Context(l, k, n)
    try:
        tr, keep = c.rows_begin(kk, wide, generated_at=GEN)                # the full-width entry on the rows with the Python z
        root_full, _ = c.rows_commit(tr)
        full, _ = c.rows_prove(tr, rands, None)
        c.trace_destroy(tr)
        assert root_full == want["root"] and full == want["proof"]
        d_packed = c.upload(packed)
        for where in ("host", "device"):
            if where == "device":
                tr, keep = c.rows_begin(kk, d_packed, on_device=True, generated_at=GEN, elem_bytes=widths)
            else:
                tr, keep = c.rows_begin(kk, packed, generated_at=GEN, elem_bytes=widths)
            root, seed1 = c.rows_commit(tr)
            assert root == want["root"] and seed1 == want["stage1_seed"], where
            # the restart between commit and prove: the next trace arrives from the other side while this one is proved
            if where == "device":
                c.rows_restart(tr, packed.ctypes.data, on_device=False)
            else:
                c.rows_restart(tr, d_packed, on_device=True)
            proof, info = c.rows_prove(tr, rands, None)
            assert proof == want["proof"], where
            assert info.valid_quad == 1
            assert c.rows_commit(tr) == (root, seed1)
            proof2, _ = c.rows_prove(tr, rands, None)
            assert proof2 == proof, where
            # and once more from the same side
            c.rows_restart(tr, d_packed if where == "device" else packed.ctypes.data, on_device=where == "device")
            assert c.rows_commit(tr) == (root, seed1)
            proof3, _ = c.rows_prove(tr, rands, None)
            assert proof3 == proof, where
            c.trace_destroy(tr)
    finally:
        c.close()


@pytest.mark.parametrize("place", ["x_last_of_chunk", "z_first_of_chunk"])
@pytest.mark.parametrize("l,k,n", [(320, 512, 2048), (317, 512, 2048)])
def test_derived_rows_across_stage1_chunks_equal_oracle_and_full_width(amd, l, k, n, place):
    """135 rows.  The stage-1 chunks are cut by row count: [0, 39), [39, 135) at this size (the 96-row tail rule; the 128-row head
    chunk only exists above 224 rows), and row 128 would be the cut with a head chunk.  One trace has a triple whose x row is the
    last row in front of each cut, the other a triple whose z row is the first row behind it -- the two cannot share a trace at
    one cut.  Operand classes within each trace: bit x bit, 4 x 4, 8 x 8 with (2^64 - 1)^2, 8 x 32, bit x 32, 32 x 32 with
    (p-1)(p-1), (p-1) * 2, zero operands, all limbs populated, and more."""
    R = 135
    chunks = stage1_chunks(R)
    assert chunks == [(0, 39), (39, 135)]
    cuts = [chunks[0][1], 128]
    forced = [c - 1 for c in cuts] if place == "x_last_of_chunk" else [c - 2 for c in cuts]
    kinds = layout(R, forced)
    assert len(kinds) == R
    for c in cuts:
        if place == "x_last_of_chunk":
            assert list(kinds[c - 1:c + 2]) == [1, 2, 3]                   # x is the last row of the chunk, y and z open the next
        else:
            assert list(kinds[c - 2:c + 1]) == [1, 2, 3]                   # z is the first row of the next chunk
    rows, masks, rands, pairs = build_trace(l, k, n, kinds)
    assert set(pairs.values()) >= {("bit", "bit"), (4, 4), (8, 8), (8, 32), ("bit", 32), (32, 32)}
    run_every_path(amd, l, k, n, kinds, rows, masks, rands)


def test_derived_rows_in_a_full_512_row_chunk_at_the_large_geometry(amd):
    """736 rows at (8000, 8192, 32768): chunks [0, 128), [128, 640), [640, 736).  A triple straddles each cut -- x | y z at 128,
    x y | z at 640 -- and the full 512-row chunk holds derived rows of every operand class"""
    l, k, n, R = 8000, 8192, 32768, 736
    assert stage1_chunks(R) == [(0, 128), (128, 640), (640, 736)]
    forced = [127, 638] + list(range(200, 200 + 3 * 9, 3))
    kinds = np.zeros(R, dtype=np.uint8)
    for f in forced:
        kinds[f:f + 3] = (1, 2, 3)
    assert list(kinds[127:130]) == [1, 2, 3] and list(kinds[638:641]) == [1, 2, 3]
    assert sum(1 for r in range(128, 640) if kinds[r] == 3) >= 10
    rows, masks, rands, pairs = build_trace(l, k, n, kinds, lin_classes=("bit", 8, 1, 32, 4, 2, "bit", "bit"))
    assert set(pairs.values()) >= set(PAIRS[:6])
    run_every_path(amd, l, k, n, kinds, rows, masks, rands)


def _begin_one(amd, c, kinds, widths, comm=None, on_device=False):
    l, k = 320, 512
    rows = np.zeros((len(kinds), k, 8), dtype=np.uint32)
    rows[:, :l, 0] = 1
    packed = amd.pack_rows(rows, widths, l)
    if not packed.size:
        packed = np.zeros(4, dtype=np.uint8)
    msgs = c.upload(packed) if on_device else packed
    eb = np.array(widths, dtype=np.uint8)
    if comm is None:
        tr, keep = c.rows_begin(np.array(kinds, dtype=np.uint8), msgs, on_device=on_device, generated_at=GEN, elem_bytes=eb)
        c.trace_destroy(tr)
    else:
        sh = c.shard_rows_begin(np.array(kinds, dtype=np.uint8), msgs, 0, 1, comm, on_device=on_device, generated_at=GEN, elem_bytes=eb)
        c.shard_destroy(sh)


def refusal_cases(amd):
    D, B, F = amd.ELEM_PRODUCT, amd.ELEM_BIT, amd.ROW_DRAW_PAD
    LIN, QX, QY, QZ, INIT, BIT, BQX, BQY, BQZ = 0, 1, 2, 3, 4, 5, 8, 9, 10
    accepted = [([QX | F, QY | F, QZ | F], [B, 4, D]),                    # narrow operands
                ([QX | F, QY | F, QZ | F], [32, 32, D]),                   # full-width operands, flagged
                ([QX, QY, QZ | F], [32, 0, D]),                            # ... carrying their own pads
                ([LIN | F, QX | F, QY, QZ | F, LIN], [1, 8, 32, D, 32])]
    refused = [([LIN | F, LIN | F], [D, 32]),                              # on LINEAR
               ([QX | F, QY | F, QZ | F], [D, 1, 1]),                      # on QX
               ([QX | F, QY | F, QZ | F], [1, D, 1]),                      # on QY
               ([QX | F, QY | F, QZ | F], [D, D, D]),
               ([QX | F, QY | F, QZ], [1, 1, D]),                          # QZ without LIG_ROW_DRAW_PAD
               ([QX, QY, QZ], [32, 32, D]),
               ([BQX, BQY, BQZ], [32, 32, D]),                             # batch triples are device variables
               ([LIN | F, INIT | F], [32, D]),
               ([LIN | F, BIT], [32, D])]
    return accepted, refused


def test_product_rows_are_refused_where_the_format_does_not_allow_them(amd):
    c = amd.Context(320, 512, 2048)
    try:
        accepted, refused = refusal_cases(amd)
        for kinds, widths in accepted:
            _begin_one(amd, c, kinds, widths)
            _begin_one(amd, c, kinds, widths, on_device=True)
        for kinds, widths in refused:
            with pytest.raises(amd.LigError):
                _begin_one(amd, c, kinds, widths)
    finally:
        c.close()


def test_sharded_entry_refuses_product_rows_where_the_format_does_not_allow_them(amd):
    c = amd.Context(320, 512, 2048)
    comm = c.ipc_comm("/lig_dr_" + mr.fresh_tag(), 0, 1)
    try:
        accepted, refused = refusal_cases(amd)
        for kinds, widths in accepted:
            _begin_one(amd, c, kinds, widths, comm=comm)
            _begin_one(amd, c, kinds, widths, comm=comm, on_device=True)
        for kinds, widths in refused:
            with pytest.raises(amd.LigError):
                _begin_one(amd, c, kinds, widths, comm=comm)
    finally:
        c.ipc_comm_destroy(comm)
        c.close()


DERIVED_SHARD_WORKER = textwrap.dedent('''
    import hashlib, importlib.util, json, os, sys
    import numpy as np
    root, mode = sys.argv[1], sys.argv[2]
    sys.path.insert(0, os.path.join(root, "tests"))
    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, "ligero-prover_amd", rel))
        m = importlib.util.module_from_spec(spec); sys.modules[name] = m; spec.loader.exec_module(m); return m
    pkg = load("ligero_prover_amd", "__init__.py")
    dist = load("lig_dist", "dist.py")
    import oracle_lib as ol
    import test_gpu_derived_rows as td
    l, k, n = 320, 512, 2048
    g = dist.Group("gloo")
    ctx = pkg.Context(l, k, n, device=0)
    # every rank plays the same deterministic guest and keeps its slice.  1100 rows: three 512-row global chunks at W = 2 (two
    # rounds), chunks of ~275 rows at W = 4; triples of every operand class all over, so every rank has a mix of them
    kinds = td.layout(1100, [])
    rows, masks, rands, pairs = td.build_trace(l, k, n, kinds)
    kk, widths, wide, _ = td.ship(pkg, kinds, rows, l)
    rounds, b = pkg.shard_rows_plan(kinds, g.world)
    mine = pkg.local_rows_of(b, g.rank, g.world)
    blind = wide[mine].copy()
    blind[kinds[mine] == 3] = 0xDEADBEEF                 # nothing of the expected z rows reaches the library
    packed = pkg.pack_rows(blind, widths[mine], l)
    assert len(packed) == td.packed_bytes(pkg, widths[mine], l, k)
    lr = rands[mine]
    comm = g.make_comm(pkg, ctx)
    if mode == "device":
        d_packed = ctx.upload(packed)
        sh = ctx.shard_rows_begin(kk, d_packed, g.rank, g.world, comm, on_device=True, generated_at=td.GEN, elem_bytes=widths)
    else:
        sh = ctx.shard_rows_begin(kk, packed, g.rank, g.world, comm, generated_at=td.GEN, elem_bytes=widths)
    out = []
    for rep in range(2):                                 # the second pass: lig_shard_rows_restart with the same packed rows
        if rep:
            if mode == "device":
                ctx.shard_rows_restart(sh, d_packed, on_device=True)
            else:
                ctx.shard_rows_restart(sh, packed)
        ctx.shard_rows_commit(sh)
        proof, info = ctx.shard_rows_prove(sh, lr, None)
        out.append(proof)
    ctx.shard_destroy(sh)
    ref = oref = None
    if g.rank == 0:                                      # the unsharded rows entry at full width with the Python z, and the oracle's prover
        tr, keep = ctx.rows_begin(kk, wide, generated_at=td.GEN)
        ctx.rows_commit(tr)
        ref, _ = ctx.rows_prove(tr, rands, None)
        ctx.trace_destroy(tr)
        oref = ol.prove_rows(l, k, n, 192, kinds, rows, *masks, rands, None, generated_at=td.GEN, threads=4)["proof"]
    digs = g.gather_digests(hashlib.sha256(out[0]).digest())
    mine_pairs = sorted(set(str(pairs[r]) for r in mine if r in pairs))
    print(json.dumps({"rank": g.rank, "local_rows": len(mine), "rounds": rounds, "pairs": mine_pairs, "derived": int((widths[mine] == pkg.ELEM_PRODUCT).sum()),
                      "again": out[0] == out[1], "all_equal": len(set(digs)) == 1,
                      "equals_rows_prove": None if ref is None else ref == out[0], "equals_oracle": None if oref is None else oref == out[0]}))
    g.close(); ctx.close()
''')


@pytest.mark.parametrize("world,mode,comm", [(2, "host", None), (4, "host", "ipc"), (2, "device", "ipc")])
def test_sharded_derived_rows_equal_rows_prove_and_oracle(tmp_path, world, mode, comm):
    """lig_shard_rows_* with derived rows: a rank's msgs holds nothing for them; every rank's envelope == lig_rows_prove of the
    whole trace at full width == the oracle's, operand widths mixed across the ranks, and lig_shard_rows_restart gives it again"""
    script = tmp_path / "derived_shard_worker.py"
    script.write_text(DERIVED_SHARD_WORKER)
    outs = mr.run_ranks(mr.python_argv(script, ROOT, mode), world, mr.rendezvous_env(world, comm), timeout=300)
    outs = sorted((mr.last_json(o) for o, _ in outs), key=lambda d: d["rank"])
    assert all(o["again"] and o["all_equal"] for o in outs), outs
    assert outs[0]["equals_rows_prove"] is True and outs[0]["equals_oracle"] is True, outs
    assert all(o["derived"] > 0 and len(o["pairs"]) >= 4 for o in outs), outs
    assert len(set(tuple(o["pairs"]) for o in outs)) > 1 or all(len(o["pairs"]) == len(PAIRS) for o in outs), outs


# ---- the row-batching shim (include/lig_hip_row_batcher.hpp) with hip_proof_meta::derive_products
def build_derived_batcher():
    mod = hip_lib.load()
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    odir = os.path.join(ROOT, "oracle")
    ol.build()
    src, exe = os.path.join(ROOT, "tests", "cpp", "derived_batcher_prog.cpp"), os.path.join(ROOT, "tests", "cpp", "derived_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def check_batcher(o):
    assert o["equals_oracle"] is True and o["derived_rows"] > 0, o
    assert o["shipped_bytes"] == o["computed_bytes"] and o["shipped_bytes"] < o["underived_bytes"], o
    assert o["linear_honest_valid"] is True and o["linear_equals_oracle"] is True, o
    assert o["linear_false_valid_linear"] == 0, o


def test_row_batcher_derives_the_z_rows_on_one_gpu():
    """derive_products: the QZ row of every recorded triple is not shipped, shipped_bytes() is the computed figure, the envelope
    is the oracle's; with set_linear_system a guest whose z statement is false gets valid_linear == 0"""
    p = subprocess.run([build_derived_batcher()], capture_output=True, timeout=300)
    assert p.returncode == 0, (p.stdout.decode()[-3000:], p.stderr.decode()[-3000:])
    check_batcher(mr.last_json(p.stdout.decode()))


def test_row_batcher_derives_the_z_rows_on_every_rank_of_a_sharded_trace():
    exe = build_derived_batcher()
    name = "/lig_db_" + mr.fresh_tag()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = mr.run_ranks(lambda r: [exe, str(r), "2", name], 2, env, timeout=300)
    outs = [mr.last_json(o) for o, _ in outs]
    for o in outs:
        assert o["local_rows"], o
        check_batcher(o)
