"""GPU: witness rows in every width of the narrow row format (lig_rows_job.elem_bytes: bits, 1-, 2-, 4-, 8-byte integers, full
rows) through the single-GPU rows entry, the sharded rows entry and the row-batching shim.  The rows are the oracle's
(lo_form_rows: pads, masks) with their data slots overwritten by values that need exactly each width; every envelope must be
byte-identical to the oracle's prover over the same rows and to the full-width rows entry."""
import ctypes as C
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
GEN = 41
CLASSES = ("bit", 1, 2, 4, 8, 32)


def _limbs(vals):
    """python ints -> (len, 8) uint32"""
    return ol.to_limbs(vals)


def data_for(cls, l, rng):
    """(l, 8) uint32: data slots whose narrowest width is exactly `cls`, boundary values included"""
    if cls == "bit":
        v = rng.integers(0, 2, l).astype(np.uint32)
        v[0] = 1
        out = np.zeros((l, 8), dtype=np.uint32)
        out[:, 0] = v
        return out
    if cls in (1, 2, 4):
        top = (1 << (8 * cls)) - 1
        low = 2 if cls == 1 else (top + 1) >> (4 * cls)           # the smallest value that does not fit the next narrower width
        out = np.zeros((l, 8), dtype=np.uint32)
        out[:, 0] = rng.integers(0, top + 1, l, dtype=np.uint64).astype(np.uint32)
        out[0, 0], out[1 % l, 0] = top, low
        return out
    if cls == 8:
        out = np.zeros((l, 8), dtype=np.uint32)
        out[:, :2] = rng.integers(0, 1 << 32, (l, 2), dtype=np.uint64).astype(np.uint32)
        out[0, :2] = 0xFFFFFFFF
        out[1 % l, :2] = (0, 1)                                    # 2^32
        return out
    out = rng.integers(0, 1 << 32, (l, 8), dtype=np.uint64).astype(np.uint32)
    out[:, 7] &= 0x0FFFFFFF                                        # < 2^252 < p: canonical
    out[0] = _limbs([1 << 64])[0]
    out[1 % l] = _limbs([ol.P - 1])[0]
    return out


def build_trace(l, k, n, n_lin, n_quad, seed=7):
    """-> (kinds, rows, masks, rands): the oracle's rows with data slots of every width (linear rows cycle through CLASSES,
    x / y rows are bits and z = x * y); rands: fixed canonical randomness rows"""
    job = ol.make_job(l, k, n, 192, n_lin, n_quad, generated_at=GEN, threads=8)
    rows, mc, ml, mq = ol.form_rows(job)
    kinds = ol.row_kinds(job).copy()
    rows = rows.copy()
    rng = np.random.default_rng(seed)
    j = 0
    for r in range(len(kinds)):
        if kinds[r] == 0:
            rows[r, :l] = data_for(CLASSES[j % len(CLASSES)], l, rng)
            j += 1
        elif kinds[r] == 1:
            x, y = rng.integers(0, 2, l).astype(np.uint32), rng.integers(0, 2, l).astype(np.uint32)
            for d, v in enumerate((x, y, x * y)):
                rows[r + d, :l] = 0
                rows[r + d, :l, 0] = v
    rands = rng.integers(0, 1 << 32, (len(kinds), k, 8), dtype=np.uint64).astype(np.uint32)
    rands[:, :, 7] &= 0x0FFFFFFF
    return kinds, rows, (mc, ml, mq), rands


def ship(amd, kinds, rows, l, garbage=True):
    """-> (kinds | ROW_DRAW_PAD, narrowest widths, packed bytes): pad slots of flagged rows, the round-up bytes of the packed
    rows and, in a bit row with l % 8 != 0, the bits past l of its last data byte hold garbage (the library draws the first and
    ignores the others)"""
    kk = kinds.copy()
    kk[kinds <= 3] |= amd.ROW_DRAW_PAD
    widths = amd.narrowest_widths(rows, kinds, l)
    wide = rows.copy()
    if garbage:
        wide[kinds <= 3, l:] = 0x5A5A5A5A
    packed = amd.pack_rows(wide, widths, l)
    if garbage:
        off = 0
        for w in widths:
            w = int(w)
            data = wide.shape[1] * 32 if w == 32 else ((l + 7) // 8 if w == amd.ELEM_BIT else l * w)
            full = data if w == 32 else (data + 3) // 4 * 4
            packed[off + data:off + full] = 0xA5
            if w == amd.ELEM_BIT and l % 8:
                packed[off + l // 8] |= (0xFF << (l % 8)) & 0xFF
            off += full
        assert off == len(packed)
    return kk, widths, wide, packed


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


@pytest.mark.parametrize("l,k,n,n_lin,n_quad", [
    (320, 512, 2048, 320 * 30 + 7, 320 * 2 + 5),
    (317, 512, 2048, 317 * 30 + 5, 317 * 2 + 3),             # odd l: byte, u16 and bit rows all need the round-up
    (8000, 8192, 32768, 8000 * 520 + 3, 8000 * 2 + 1),       # > one 512-row chunk at the 2^24 geometry
])
def test_narrow_rows_of_every_width_equal_oracle_and_full_width(amd, l, k, n, n_lin, n_quad):
    """host rows, device rows, and lig_rows_restart from the other side, with every width in one matrix: the envelope of the
    oracle's prover over the same rows, and of the full-width rows entry"""
    kinds, rows, masks, rands = build_trace(l, k, n, n_lin, n_quad)
    R = len(kinds)
    want = ol.prove_rows(l, k, n, 192, kinds, rows, *masks, rands, None, generated_at=GEN, threads=8)
    kk, widths, wide, packed = ship(amd, kinds, rows, l)
    assert set(int(w) for w in widths[kinds == 0]) == {amd.ELEM_BIT, 1, 2, 4, 8, 32}
    assert set(int(w) for w in widths[(kinds >= 1) & (kinds <= 3)]) == {amd.ELEM_BIT}
    assert len(packed) < wide.nbytes
    if R > 512:
        assert len(set(int(w) for w in widths[:512])) == 6 and len(set(int(w) for w in widths[512:])) > 1
    c = amd.Context(l, k, n)
    try:
        tr, keep = c.rows_begin(kk, wide, generated_at=GEN)                    # the full-width entry on the same rows
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
            # the next trace arrives from the other side while this one is proved
            if where == "device":
                c.rows_restart(tr, packed.ctypes.data, on_device=False)
            else:
                c.rows_restart(tr, d_packed, on_device=True)
            proof, _ = c.rows_prove(tr, rands, None)
            assert proof == want["proof"], where
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


def test_narrow_widths_are_refused_where_the_format_does_not_allow_them(amd):
    l, k, n = 320, 512, 2048
    rows = np.zeros((2, k, 8), dtype=np.uint32)
    rows[:, :l, 0] = 1
    c = amd.Context(l, k, n)
    try:
        def begin(kinds, widths):
            packed = amd.pack_rows(rows, [w if w in (amd.ELEM_BIT, 1, 2, 4, 8, 32) else 32 for w in widths], l)
            tr, keep = c.rows_begin(np.array(kinds, dtype=np.uint8), packed, generated_at=GEN, elem_bytes=np.array(widths, dtype=np.uint8))
            c.trace_destroy(tr)
        P, LIN, INIT, BIT = amd.ROW_DRAW_PAD, 0, 4, 5
        begin([LIN | P, LIN | P], [amd.ELEM_BIT, 1])                         # accepted
        begin([LIN | P, LIN | P], [2, 32])
        for kinds, widths in [([LIN, LIN | P], [amd.ELEM_BIT, 32]),           # no LIG_ROW_DRAW_PAD
                              ([LIN | P, LIN], [32, 1]),
                              ([LIN | P, INIT | P], [32, amd.ELEM_BIT]),      # a bit row of kind INIT
                              ([LIN | P, BIT], [32, amd.ELEM_BIT]),           # ... of kind BIT
                              ([LIN | P, LIN | P], [3, 32]),                  # widths that do not exist
                              ([LIN | P, LIN | P], [16, 32]),
                              ([LIN | P, LIN | P], [0x82, 32])]:
            with pytest.raises(amd.LigError):
                begin(kinds, widths)
    finally:
        c.close()


def test_sharded_entry_refuses_narrow_widths_where_the_format_does_not_allow_them(amd):
    """lig_shard_rows_begin checks elem_bytes as lig_rows_begin does (one rank, in-process communicator)"""
    l, k, n = 320, 512, 2048
    rows = np.zeros((2, k, 8), dtype=np.uint32)
    rows[:, :l, 0] = 1
    c = amd.Context(l, k, n)
    comm = c.ipc_comm("/lig_nr_" + mr.fresh_tag(), 0, 1)
    try:
        def begin(kinds, widths, on_device=False):
            packed = amd.pack_rows(rows, [w if w in (amd.ELEM_BIT, 1, 2, 4, 8, 32) else 32 for w in widths], l)
            msgs = c.upload(packed) if on_device else packed
            sh = c.shard_rows_begin(np.array(kinds, dtype=np.uint8), msgs, 0, 1, comm, on_device=on_device, generated_at=GEN,
                                    elem_bytes=np.array(widths, dtype=np.uint8))
            c.shard_destroy(sh)
        P, LIN, INIT, BIT = amd.ROW_DRAW_PAD, 0, 4, 5
        begin([LIN | P, LIN | P], [amd.ELEM_BIT, 1])                         # accepted, host and device rows
        begin([LIN | P, LIN | P], [2, 32], on_device=True)
        for kinds, widths in [([LIN, LIN | P], [amd.ELEM_BIT, 32]),           # no LIG_ROW_DRAW_PAD
                              ([LIN | P, INIT | P], [32, amd.ELEM_BIT]),      # a bit row of kind INIT
                              ([LIN | P, BIT], [32, amd.ELEM_BIT]),           # ... of kind BIT
                              ([LIN | P, LIN | P], [3, 32]),                  # widths that do not exist
                              ([LIN | P, LIN | P], [16, 32]),
                              ([LIN | P, LIN | P], [0x82, 32])]:
            with pytest.raises(amd.LigError):
                begin(kinds, widths)
    finally:
        c.ipc_comm_destroy(comm)
        c.close()


NARROW_SHARD_WORKER = textwrap.dedent('''
    import ctypes as C, hashlib, importlib.util, json, os, sys
    import numpy as np
    root, l, k, n, n_lin, n_quad, mode = sys.argv[1], *map(int, sys.argv[2:7]), sys.argv[7]
    sys.path.insert(0, os.path.join(root, "tests"))
    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, "ligero-prover_amd", rel))
        m = importlib.util.module_from_spec(spec); sys.modules[name] = m; spec.loader.exec_module(m); return m
    pkg = load("ligero_prover_amd", "__init__.py")
    dist = load("lig_dist", "dist.py")
    import oracle_lib as ol
    import test_gpu_narrow_rows as tn
    g = dist.Group("gloo")
    ctx = pkg.Context(l, k, n, device=0)
    # every rank plays the same deterministic guest (all rows, all kinds, the randomness rows) and keeps its slice
    kinds, rows, masks, rands = tn.build_trace(l, k, n, n_lin, n_quad)
    kk, widths, wide, _ = tn.ship(pkg, kinds, rows, l)
    rounds, b = pkg.shard_rows_plan(kinds, g.world)
    mine = pkg.local_rows_of(b, g.rank, g.world)
    local = wide[mine] if len(mine) else np.zeros((0, k, 8), dtype=np.uint32)
    packed = pkg.pack_rows(local, widths[mine], l) if len(mine) else np.zeros(0, dtype=np.uint8)
    lr = rands[mine] if len(mine) else np.zeros((0, k, 8), dtype=np.uint32)
    comm = g.make_comm(pkg, ctx)
    if mode == "device":
        d_packed = ctx.upload(packed) if packed.size else ctx.malloc(32)
        sh = ctx.shard_rows_begin(kk, d_packed, g.rank, g.world, comm, on_device=True, generated_at=tn.GEN, elem_bytes=widths)
    else:
        sh = ctx.shard_rows_begin(kk, packed, g.rank, g.world, comm, generated_at=tn.GEN, elem_bytes=widths)
    out = []
    for rep in range(2):                             # the second pass: lig_shard_rows_restart with the same packed rows
        if rep:
            if mode == "device":
                ctx.shard_rows_restart(sh, d_packed, on_device=True)
            else:
                ctx.shard_rows_restart(sh, packed)
        root_, seed1 = ctx.shard_rows_commit(sh)
        proof, info = ctx.shard_rows_prove(sh, lr, None)
        out.append(proof)
    ctx.shard_destroy(sh)
    ref = oref = None
    if g.rank == 0:                                  # the unsharded rows entry at full width, and the oracle's prover
        tr, keep = ctx.rows_begin(kk, wide, generated_at=tn.GEN)
        ctx.rows_commit(tr)
        ref, _ = ctx.rows_prove(tr, rands, None)
        ctx.trace_destroy(tr)
        oref = ol.prove_rows(l, k, n, 192, kinds, rows, *masks, rands, None, generated_at=tn.GEN, threads=4)["proof"]
    digs = g.gather_digests(hashlib.sha256(out[0]).digest())
    print(json.dumps({"rank": g.rank, "local_rows": len(mine), "rounds": rounds, "widths": sorted(set(int(w) for w in widths[mine])),
                      "again": out[0] == out[1], "all_equal": len(set(digs)) == 1,
                      "equals_rows_prove": None if ref is None else ref == out[0], "equals_oracle": None if oref is None else oref == out[0]}))
    g.close(); ctx.close()
''')


@pytest.mark.parametrize("world,n_lin,n_quad,mode,comm", [
    (2, 320 * 40 + 9, 320 * 3 + 1, "host", None),               # mixed widths over gloo callbacks
    (4, 320 * 4300 + 1, 330, "host", "ipc"),                     # three exchange rounds on 4 ranks
    (4, 320 * 2 + 5, 0, "host", "ipc"),                          # 3 rows on 4 ranks: a rank without rows
    (8, 320 * 9000 + 11, 330, "host", "ipc"),                    # the node's shape: 8 ranks, three rounds
    (2, 320 * 1500 + 7, 330, "device", "ipc"),                   # packed rows resident on the device, two rounds
])
def test_sharded_narrow_rows_equal_rows_prove_and_oracle(tmp_path, world, n_lin, n_quad, mode, comm):
    """lig_shard_rows_* with elem_bytes: each rank passes the widths of all rows and its own rows packed back to back; every rank's
    envelope == lig_rows_prove of the whole trace at full width == the oracle's, and lig_shard_rows_restart gives it again"""
    script = tmp_path / "narrow_shard_worker.py"
    script.write_text(NARROW_SHARD_WORKER)
    outs = mr.run_ranks(mr.python_argv(script, ROOT, 320, 512, 2048, n_lin, n_quad, mode), world, mr.rendezvous_env(world, comm), timeout=300)
    outs = sorted((mr.last_json(o) for o, _ in outs), key=lambda d: d["rank"])
    assert all(o["again"] and o["all_equal"] for o in outs), outs
    assert outs[0]["equals_rows_prove"] is True and outs[0]["equals_oracle"] is True, outs
    if n_lin == 320 * 2 + 5:
        assert min(o["local_rows"] for o in outs) == 0
    else:
        assert all(len(o["widths"]) > 1 for o in outs if o["local_rows"]), outs
    if n_lin > 320 * 1000:
        assert outs[0]["rounds"] >= 2


# ---- the row-batching shim (include/lig_hip_row_batcher.hpp) with hip_proof_meta::narrowest
def build_narrow_batcher():
    mod = hip_lib.load()
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    odir = os.path.join(ROOT, "oracle")
    ol.build()
    src, exe = os.path.join(ROOT, "tests", "cpp", "narrow_batcher_prog.cpp"), os.path.join(ROOT, "tests", "cpp", "narrow_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def test_row_batcher_ships_each_row_in_its_narrowest_width_on_one_gpu():
    """narrow_rows = narrowest = true: bit and byte witness rows leave the shim as LIG_ELEM_BIT / 1-byte rows (1 / 8 of a byte per
    data slot against 32 bytes per slot at full width) and the envelope is the oracle's"""
    p = subprocess.run([build_narrow_batcher()], capture_output=True, timeout=300)
    assert p.returncode == 0, (p.stdout.decode()[-3000:], p.stderr.decode()[-3000:])
    out = mr.last_json(p.stdout.decode())
    assert out["equals_oracle"] is True, out
    assert out["shipped_bytes"] * 32 < out["full_bytes"], out


def test_row_batcher_ships_narrowest_rows_on_every_rank_of_a_sharded_trace():
    exe = build_narrow_batcher()
    name = "/lig_nb_" + mr.fresh_tag()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = mr.run_ranks(lambda r: [exe, str(r), "2", name], 2, env, timeout=300)
    outs = [mr.last_json(o) for o, _ in outs]
    assert all(o["equals_oracle"] is True and o["local_rows"] and o["shipped_bytes"] * 32 < o["full_bytes"] for o in outs), outs
