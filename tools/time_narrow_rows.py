#!/usr/bin/env python3
"""Caller-rows entry with the witness in pinned HOST memory, shipped in each width of the narrow row format (lig_rows_job.elem_bytes).

The 2^24-constraint trace of the default bench geometry (l = 8000, k = 8192, n = 32768) whose witness slots are all bits, so the SAME
values travel as full rows (32), 8-, 4-, 2-, 1-byte integers and packed bits; the library draws every pad and samples the dense
randomness rows on the device.  Two proofs in flight on two contexts (commit -> restart of the next trace -> prove, as bench.py's
RowsFromHostWorkload does), the upload of every trace inside the timed region.  Per width: constraints/s, bytes over the link per
trace, and the proof's sha256 (equal across widths: same values).

    python tools/time_narrow_rows.py [--widths 32,8,4,2,1,bit] [--steps 4] [--warmup 1] [--inflight 2] [--json out.json]

The expansion kernel's own time per 512-row chunk comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool
(--widths 8), with this build and with the parent's (LIG_HIP_LIB=...): profiles/r07_narrow_rows.md."""
import argparse
import ctypes as C
import hashlib
import importlib.util
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_, K_, N_ = 8000, 8192, 32768


def load_pkg():
    spec = importlib.util.spec_from_file_location("ligero_prover_amd", os.path.join(ROOT, "ligero-prover_amd", "__init__.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["ligero_prover_amd"] = m
    spec.loader.exec_module(m)
    return m


def packed_bytes(pkg, bits, w):
    """bits (R, l) uint8 -> the packed rows of width w (every row a multiple of 4 bytes at l = 8000)"""
    R, l = bits.shape
    if w == 32:
        full = np.zeros((R, K_, 8), dtype=np.uint32)
        full[:, :l, 0] = bits
        return full.reshape(-1).view(np.uint8)
    if w == pkg.ELEM_BIT:
        out = np.packbits(bits, axis=1, bitorder="little")
    elif w == 8:
        out = np.zeros((R, l, 2), dtype=np.uint32)
        out[:, :, 0] = bits
    else:
        out = bits.astype("<u%d" % w)
    out = np.ascontiguousarray(out).reshape(R, -1).view(np.uint8)
    assert out.shape[1] % 4 == 0
    return out.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="32,8,4,2,1,bit")
    ap.add_argument("--constraints", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    R = -(-a.constraints // L_)
    per_row = np.full(R, L_, dtype=np.uint32)
    if a.constraints % L_:
        per_row[-1] = a.constraints % L_
    bits = np.random.default_rng(24).integers(0, 2, (R, L_), dtype=np.uint8)
    bits[-1, per_row[-1]:] = 0
    kinds = np.full(R, pkg.ROW_KINDS["LINEAR"] | pkg.ROW_DRAW_PAD, dtype=np.uint8)
    ctxs = [pkg.Context(L_, K_, N_, device=a.device) for _ in range(a.inflight)]
    results = []
    for name in a.widths.split(","):
        w = pkg.ELEM_BIT if name == "bit" else int(name)
        packed = packed_bytes(pkg, bits, w)
        link = len(packed)
        host = torch.empty(len(packed), dtype=torch.uint8, pin_memory=True)
        host.copy_(torch.from_numpy(packed))
        del packed
        widths = np.full(R, w, dtype=np.uint8)
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
                out, info = c.rows_prove(t, None, None, copy=False)          # (address, length) of the trace-owned envelope
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
        r = {"width": name, "constraints_per_s": a.constraints * a.inflight * a.steps / dt, "ms_per_trace": 1e3 * dt / (a.inflight * a.steps),
             "link_bytes_per_trace": link,
             "proof_sha256": hashlib.sha256(proofs[0]).hexdigest(), "inflight_equal": len(set(proofs)) == 1}
        results.append(r)
        print("width %-4s %.4e constraints/s  %7.2f ms/trace  %11d link bytes/trace  sha256 %s" % (
            name, r["constraints_per_s"], r["ms_per_trace"], r["link_bytes_per_trace"], r["proof_sha256"][:16]), flush=True)
    for c in ctxs:
        c.close()
    same = len(set(r["proof_sha256"] for r in results)) == 1 and all(r["inflight_equal"] for r in results)
    print(json.dumps({"tool": "time_narrow_rows", "constraints": a.constraints, "rows": R, "inflight": a.inflight, "steps": a.steps,
                      "same_proof_across_widths": same, "results": results}))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"constraints": a.constraints, "rows": R, "inflight": a.inflight, "steps": a.steps, "same_proof_across_widths": same,
                       "results": results}, f, indent=1)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
