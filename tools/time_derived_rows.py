#!/usr/bin/env python3
"""Derived product rows (lig_rows_job.elem_bytes = LIG_ELEM_PRODUCT): what not shipping the z row of a quadratic triple buys.

A trace of quadratic triples at the default bench geometry (l = 8000, k = 8192, n = 32768; 699 triples = 2097 rows, 2^24
geometry), rows in pinned HOST memory, the library draws every pad and samples the dense randomness rows on the device.  Two
operand classes:
    word   x and y are 8-byte words; z = x * y is 128 bits wide and fits no narrow width
    field  x and y are full field elements; z = x * y mod p
Two legs, alternating in ONE command (a, b, a, b, ...):
    a   the best format without derivation: x and y in their narrowest width, z shipped at 32 bytes per slot
    b   z derived on the device (LIG_ELEM_PRODUCT): nothing shipped for it
Two proofs in flight on two contexts (commit -> restart of the next trace -> prove, as tools/time_narrow_rows.py), the upload of
every trace inside the timed region.  Per class and leg: ms per proof of every repetition, their median, bytes over the link per
trace, the proof's sha256 (equal across the legs: same rows).

    python tools/time_derived_rows.py [--classes word,field] [--legs a,b] [--reps 3] [--steps 4] [--warmup 1] [--json out.json]

`--legs a` runs on a library without the format (LIG_HIP_LIB=<the parent's build>): the did-not-move check of the existing path.
The kernels' own times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool (--legs b --reps 1):
k_expand_product beside k_expand_narrow -> profiles/r10_derived_product_rows.md."""
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
P = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
ELEM_PRODUCT = 0x82


def load_pkg():
    spec = importlib.util.spec_from_file_location("ligero_prover_amd", os.path.join(ROOT, "ligero-prover_amd", "__init__.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["ligero_prover_amd"] = m
    spec.loader.exec_module(m)
    return m


def limbs(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint32).reshape(-1, 8)


def triples_of(cls, distinct, rng):
    """-> (x, y, z) as (distinct, l, w) uint32 limb arrays, w = 2 for 8-byte words and 8 for field elements and every z"""
    if cls == "word":
        x = rng.integers(0, 1 << 64, (distinct, L_), dtype=np.uint64)
        y = rng.integers(0, 1 << 64, (distinct, L_), dtype=np.uint64)
        z = limbs([int(a) * int(b) for a, b in zip(x.reshape(-1), y.reshape(-1))]).reshape(distinct, L_, 8)
        return x.view(np.uint32).reshape(distinct, L_, 2), y.view(np.uint32).reshape(distinct, L_, 2), z
    raw = rng.integers(0, 1 << 32, (2, distinct * L_, 8), dtype=np.uint64).astype(np.uint32)
    raw[:, :, 7] &= 0x0FFFFFFF                                             # < 2^252 < p: canonical
    xi = [int.from_bytes(raw[0, i].tobytes(), "little") for i in range(distinct * L_)]
    yi = [int.from_bytes(raw[1, i].tobytes(), "little") for i in range(distinct * L_)]
    z = limbs([a * b % P for a, b in zip(xi, yi)]).reshape(distinct, L_, 8)
    return raw[0].reshape(distinct, L_, 8), raw[1].reshape(distinct, L_, 8), z


def pack_trace(cls, leg, triples, x, y, z):
    """-> (uint8 array: the packed rows of the trace, widths): triple t carries the data of distinct triple t % distinct"""
    distinct = x.shape[0]
    wide = cls == "field"

    def row(a):                                                            # (l, w) limbs -> the bytes of one packed row
        if a.shape[1] == 8:                                                # a full row: k slots, the library draws the pads
            full = np.zeros((K_, 8), dtype=np.uint32)
            full[:L_] = a
            return full.reshape(-1).view(np.uint8)
        return np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    per = [np.concatenate([row(x[d]), row(y[d])] + ([row(z[d])] if leg == "a" else [])) for d in range(distinct)]
    packed = np.concatenate([per[t % distinct] for t in range(triples)])
    wxy = 32 if wide else 8
    widths = np.tile(np.array([wxy, wxy, 32 if leg == "a" else ELEM_PRODUCT], dtype=np.uint8), triples)
    return packed, widths


def expected_link_bytes(cls, leg, triples):
    xy = K_ * 32 if cls == "field" else L_ * 8
    return triples * (2 * xy + (K_ * 32 if leg == "a" else 0))


def run_leg(pkg, torch, ctxs, a, kinds, per_row, packed, widths):
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
    ap.add_argument("--classes", default="word,field")
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--triples", type=int, default=699)
    ap.add_argument("--distinct", type=int, default=4, help="distinct triples of data, tiled over the trace")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    legs = a.legs.split(",")
    R = 3 * a.triples
    F = pkg.ROW_DRAW_PAD
    kinds = np.tile(np.array([1 | F, 2 | F, 3 | F], dtype=np.uint8), a.triples)
    per_row = np.full(R, L_, dtype=np.uint32)
    ctxs = [pkg.Context(L_, K_, N_, device=a.device) for _ in range(a.inflight)]
    results = []
    for cls in a.classes.split(","):
        x, y, z = triples_of(cls, a.distinct, np.random.default_rng(10))
        data = {leg: pack_trace(cls, leg, a.triples, x, y, z) for leg in legs}
        ms = {leg: [] for leg in legs}
        sha = {}
        for rep in range(a.reps):
            for leg in legs:                                                           # alternating: a, b, a, b, ...
                packed, widths = data[leg]
                assert len(packed) == expected_link_bytes(cls, leg, a.triples)
                t, h = run_leg(pkg, torch, ctxs, a, kinds, per_row, packed, widths)
                ms[leg].append(t)
                sha[leg] = h
                print("class %-5s leg %s rep %d  %7.2f ms/proof  %11d link bytes/trace  sha256 %s" % (cls, leg, rep, t, len(packed), h[:16]), flush=True)
        for leg in legs:
            results.append({"class": cls, "leg": leg, "ms_per_proof": ms[leg], "median_ms": statistics.median(ms[leg]),
                            "spread_ms": max(ms[leg]) - min(ms[leg]), "link_bytes_per_trace": len(data[leg][0]), "proof_sha256": sha[leg]})
    for c in ctxs:
        c.close()
    same = all(len(set(r["proof_sha256"] for r in results if r["class"] == cls)) == 1 for cls in a.classes.split(","))
    out = {"tool": "time_derived_rows", "triples": a.triples, "rows": R, "slots": a.triples * L_, "inflight": a.inflight, "steps": a.steps,
           "reps": a.reps, "same_proof_across_legs": same, "results": results}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
