#!/usr/bin/env python3
"""Mixed witness rows (lig_rows_job.wide_per_row): what shipping a bit row with a few machine words as bits + records buys.

A trace of linear rows at the default bench geometry (l = 8000, k = 8192, n = 32768; 2098 rows = 2^24 constraints), every row with
the profile of the recorded i32_add linear row: 0.5 % of the data slots (40 of 8000) are machine words -- 36 of 4 bytes, 4 of 8 --
among bits.  Rows in pinned HOST memory, the library draws every pad and samples the dense randomness rows on the device.
Two legs, alternating in ONE command (a, b, a, b, ...):
    a   narrowest_widths, as before the format: the OR of the slots decides, every row travels 8 bytes per slot (64 000 bytes)
    b   mixed_widths: a bit row + 40 records of 36 bytes (2440 bytes)
The upload of every trace is inside the timed region (commit -> restart of the next trace -> prove, --inflight proofs in flight on
as many contexts, as tools/time_derived_rows.py).  Per leg: ms per proof of every round, their median, bytes over the link per
trace (they follow from the arithmetic: expected_link_bytes), the proof's sha256 (equal across the legs: same rows).

    python tools/time_mixed_rows.py [--rows 2098] [--legs a,b] [--reps 5] [--steps 4] [--warmup 1] [--inflight 2] [--json out.json]"""
import argparse
import ctypes as C
import hashlib
import importlib.util
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_, K_, N_ = 8000, 8192, 32768
WORDS4, WORDS8 = 36, 4                     # per row: slots that need 4 bytes, slots that need 8 (the i32_add linear row at l = 8000)


def load_pkg():
    if "ligero_prover_amd" in sys.modules:
        return sys.modules["ligero_prover_amd"]
    spec = importlib.util.spec_from_file_location("ligero_prover_amd", os.path.join(ROOT, "ligero-prover_amd", "__init__.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["ligero_prover_amd"] = m
    spec.loader.exec_module(m)
    return m


def profile_rows(distinct, rng, l=L_, k=K_):
    """(distinct, k, 8) uint32: bits, with WORDS4 slots of 17..32 bits and WORDS8 slots of 33..64 bits at random columns"""
    rows = np.zeros((distinct, k, 8), dtype=np.uint32)
    rows[:, :l, 0] = rng.integers(0, 2, (distinct, l))
    for d in range(distinct):
        cols = rng.permutation(l)[:WORDS4 + WORDS8]
        rows[d, cols[:WORDS4], 0] = rng.integers(1 << 16, 1 << 32, WORDS4, dtype=np.uint64)
        rows[d, cols[WORDS4:], 0] = rng.integers(0, 1 << 32, WORDS8, dtype=np.uint64)
        rows[d, cols[WORDS4:], 1] = rng.integers(1, 1 << 32, WORDS8, dtype=np.uint64)
    return rows


def expected_link_bytes(leg, rows, l=L_):
    """the arithmetic of the two formats for this profile: 8 bytes per slot | ceil(l / 32) dwords of bits + 36 bytes per word slot"""
    return rows * (8 * l if leg == "a" else (l + 31) // 32 * 4 + 36 * (WORDS4 + WORDS8))


def pack_trace(pkg, leg, rows, data, l=L_):
    """-> (packed bytes of the whole trace, widths, wide_per_row or None): row r carries the data of distinct row r % distinct"""
    distinct = len(data)
    kinds = np.zeros(distinct, dtype=np.uint8)
    if leg == "a":
        w, c = pkg.narrowest_widths(data, kinds, l), None
        per = [pkg.pack_rows(data[d:d + 1], w[d:d + 1], l) for d in range(distinct)]
    else:
        w, c = pkg.mixed_widths(data, kinds, l)
        per = [pkg.pack_rows_mixed(data[d:d + 1], w[d:d + 1], c[d:d + 1], l) for d in range(distinct)]
    idx = np.arange(rows) % distinct
    packed = np.concatenate([per[i] for i in idx]) if rows else np.zeros(0, dtype=np.uint8)
    return packed, np.ascontiguousarray(w[idx]), None if c is None else np.ascontiguousarray(c[idx])


def run_leg(pkg, torch, ctxs, a, kinds, per_row, packed, widths, wide):
    host = torch.empty(len(packed), dtype=torch.uint8, pin_memory=True)
    host.copy_(torch.from_numpy(packed))
    R = len(kinds)
    traces = []
    for c in ctxs:
        job = pkg.RowsJob()
        job.rows, job.kinds, job.msgs, job.msgs_on_device = R, kinds.ctypes.data, host.data_ptr(), 0
        for i in range(32):
            job.encoding_seed[i] = i
            job.program_hash[i] = 0
        job.version = b"1.5.0"
        job.set_public_args(None)
        job.dense_rands_per_row = per_row.ctypes.data
        job.elem_bytes = widths.ctypes.data
        if wide is not None:
            job.wide_per_row = wide.ctypes.data
            job.reserved = pkg.ROWS_JOB_WIDE
        t = C.c_void_p()
        c.check(c.L.lig_rows_begin(c.h, C.byref(job), C.byref(t)))
        traces.append([t, True])

    def loop(i, steps, last):
        c, t = ctxs[i], traces[i][0]
        out = None
        for s in range(steps):
            if not traces[i][1]:
                c.check(c.L.lig_rows_restart(t, C.c_void_p(host.data_ptr()), 0))
            c.rows_commit(t)
            traces[i][1] = s + 1 < steps or not last
            if traces[i][1]:                                                         # the next trace goes up under this proof
                c.check(c.L.lig_rows_restart(t, C.c_void_p(host.data_ptr()), 0))
            out, info = c.rows_prove(t, None, None, copy=False)
            if not (info.valid_code and info.valid_linear and info.valid_quad):
                raise SystemExit("prover self-check failed")
        return C.string_at(*out)

    with ThreadPoolExecutor(max_workers=a.inflight) as pool:
        list(pool.map(lambda i: loop(i, a.warmup, False), range(a.inflight)))
        t0 = time.perf_counter()
        proofs = list(pool.map(lambda i: loop(i, a.steps, True), range(a.inflight)))
        dt = time.perf_counter() - t0
    for c, (t, _) in zip(ctxs, traces):
        c.trace_destroy(t)
    del host
    if len(set(proofs)) != 1:
        raise SystemExit("the proofs in flight differ")
    return 1e3 * dt / (a.inflight * a.steps), hashlib.sha256(proofs[0]).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2098, help="linear rows of the trace (2098 x 8000 slots = 2^24 constraints)")
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--distinct", type=int, default=8, help="distinct rows of data, tiled over the trace")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    legs = a.legs.split(",")
    R = a.rows
    kinds = np.full(R, pkg.ROW_KINDS["LINEAR"] | pkg.ROW_DRAW_PAD, dtype=np.uint8)
    per_row = np.full(R, L_, dtype=np.uint32)
    data = profile_rows(a.distinct, np.random.default_rng(13))
    packed = {leg: pack_trace(pkg, leg, R, data) for leg in legs}
    for leg in legs:
        assert len(packed[leg][0]) == expected_link_bytes(leg, R), (leg, len(packed[leg][0]))
    ctxs = [pkg.Context(L_, K_, N_, device=a.device) for _ in range(a.inflight)]
    ms, sha = {leg: [] for leg in legs}, {}
    for rep in range(a.reps):
        for leg in legs:                                                               # alternating: a, b, a, b, ...
            t, h = run_leg(pkg, torch, ctxs, a, kinds, per_row, *packed[leg])
            ms[leg].append(t)
            sha[leg] = h
            print("leg %s round %d  %7.2f ms/proof  %11d link bytes/trace  sha256 %s" % (leg, rep, t, len(packed[leg][0]), h[:16]), flush=True)
    for c in ctxs:
        c.close()
    results = [{"leg": leg, "ms_per_proof": ms[leg], "median_ms": statistics.median(ms[leg]), "spread_ms": max(ms[leg]) - min(ms[leg]),
                "link_bytes_per_trace": len(packed[leg][0]), "proof_sha256": sha[leg]} for leg in legs]
    same = len(set(sha.values())) == 1
    out = {"tool": "time_mixed_rows", "rows": R, "slots": R * L_, "word_slots_per_row": WORDS4 + WORDS8, "inflight": a.inflight, "steps": a.steps,
           "reps": a.reps, "same_proof_across_legs": same, "results": results}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
