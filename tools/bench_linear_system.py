#!/usr/bin/env python3
"""What the sparse linear system (lig_rows_set_linear) buys on the rows entry, in ONE command on one box.

Shape: the 2^24-constraint trace of bench.py (k = 8192, l = 8000, linear rows from pinned host memory), timing discipline of its
rows-from-host leg (bench.py: RowsFromHostWorkload, which this tool drives): warm-up, >= 20 steps, two traces in flight, whole
steps timed up to a device synchronise.  Legs (a) and (b) ALTERNATE `--rounds` times:

  (a) the existing path: witness rows AND dense randomness rows from pinned host memory (bench.py --full: incl_h2d.caller_rands)
  (b) the sparse path per proof, structure resident: witness rows from pinned host memory, lig_rows_prove(rands = NULL)
  (c) lig_rows_set_linear once (upload + regroup by slot), in ms
  (d) --form-only N: N x lig_linear_form and nothing else -- run it under `rocprofv3 --kernel-trace --stats -- python ...`, a run of
      its own, to read the form kernels alone; the bytes they move are printed here

The system: ONE single-term constraint per witness slot, coefficient +1, constraint c = slot c -- the statement of the synthetic
stream (w_s = b_s), whose randomness rows are exactly the dense rows of (a); so (a) and (b) must produce the SAME proof bytes (checked).
The table is empty: the public constant -sum_s b_s r_s would need b (2^24 elements) as table entries, so (b) hands over the
constant as a given value (the one leg (a) reports), which lig_rows_prove uses as given.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workload classes and the shape; importing it runs nothing)


class SparseWorkload(bench.RowsFromHostWorkload):
    """leg (b): RowsFromHostWorkload without randomness rows -- every trace carries the linear system instead"""
    name = "rows_from_host_sparse"

    def __init__(self, ctx, constraints, pkg, inflight, device, const_sum):
        import numpy as np
        self._np = np
        self.const_sum = np.frombuffer(bytes(const_sum), dtype=np.uint8).copy()
        self.set_linear_ms = []
        super().__init__(ctx, constraints, pkg, inflight, device)

    def _begin(self, c, kinds):
        np = self._np
        self.caller_rands = True                                   # (for the base class: a job without dense_rands_per_row)
        t, keep = super()._begin(c, kinds)
        self.caller_rands = False
        if not hasattr(self, "system"):
            n = self.constraints_per_trace
            rows_of = np.repeat(np.arange(len(self.per_row), dtype=np.uint64), self.per_row)
            cols = np.arange(n, dtype=np.uint64) - np.repeat(np.cumsum(self.per_row, dtype=np.uint64) - self.per_row, self.per_row)
            slots = (rows_of * bench.L_ + cols).astype(np.uint32)
            self.system = self.pkg.LinearSystem.make(np.arange(n + 1, dtype=np.uint32), slots, np.full(n, self.pkg.COEF_ONE, dtype=np.uint32))
        t0 = time.perf_counter()
        c.rows_set_linear(t, self.system)
        self.set_linear_ms.append(1e3 * (time.perf_counter() - t0))
        return t, keep

    def _loop(self, i, steps):
        c, t = self.ctxs[i], self.traces[i]
        host = C.c_void_p(self.host.data_ptr())
        out = None
        for s_ in range(steps):
            if not self.loaded[i]:
                c.check(c.L.lig_rows_restart(t, host, 0))
            c.rows_commit(t)
            self.loaded[i] = s_ + 1 < steps
            if self.loaded[i]:
                c.check(c.L.lig_rows_restart(t, host, 0))
            (addr, length), info = c.rows_prove(t, None, self.const_sum, copy=False)
            if not (info.valid_code and info.valid_linear and info.valid_quad):
                raise SystemExit("prover self-check failed")
            out = (addr, length)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-constraints", type=int, default=24)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="(a), (b) alternations")
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--form-only", type=int, default=0, help="N x lig_linear_form only (for a rocprofv3 --kernel-trace --stats run)")
    a = ap.parse_args()
    import numpy as np
    import torch
    pkg = bench.load_pkg()
    n = 1 << a.log2_constraints
    ctx = pkg.Context(bench.L_, bench.K_, bench.N_, device=0)

    def timed(wl):
        wl.run(a.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wl.run(a.steps)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    if a.form_only:
        R = -(-n // bench.L_)
        kinds = np.zeros(R, dtype=np.uint8)
        slots = np.arange(n, dtype=np.uint32)                      # full rows: slot = row * l + column = constraint number
        system = pkg.LinearSystem.make(np.arange(n + 1, dtype=np.uint32), slots, np.full(n, pkg.COEF_ONE, dtype=np.uint32))
        out = ctx.malloc(R * bench.K_ * 32)
        for _ in range(a.form_only):
            ctx.linear_form(system, kinds, bytes(range(32)), out)
        print(json.dumps({"form_only": a.form_only, "constraints": n, "rows": R,
                          "k_lin_form_bytes": {"r_gather": 32 * n, "entries": 8 * n, "segment_bounds": 4 * R * bench.L_, "rn_written": 32 * R * bench.K_},
                          "k_rng_fill_bytes_written": 32 * n}))
        ctx.close()
        return

    res = {"constraints": n, "steps": a.steps, "warmup": a.warmup, "inflight": a.inflight, "a_ms_per_proof": [], "b_ms_per_proof": []}
    wa = bench.RowsFromHostWorkload(ctx, n, pkg, a.inflight, 0, caller_rands=True)
    wa.run(1)
    const_sum = None
    # the public constant of the statement, as leg (a) reports it (const_sum = NULL there: minus the sum of the inner products)
    c0, t0_ = wa.ctxs[0], wa.traces[0]
    c0.check(c0.L.lig_rows_restart(t0_, C.c_void_p(wa.host.data_ptr()), 0))
    c0.rows_commit(t0_)
    _, info = c0.rows_prove(t0_, wa.rands.data_ptr(), None, copy=False)
    const_sum = bytes(info.const_sum)
    wa.loaded[0] = False
    ctx_b = pkg.Context(bench.L_, bench.K_, bench.N_, device=0)
    wb = SparseWorkload(ctx_b, n, pkg, a.inflight, 0, const_sum)
    for _ in range(a.rounds):
        for wl, key in ((wa, "a_ms_per_proof"), (wb, "b_ms_per_proof")):
            dt = timed(wl)
            res[key].append(1e3 * dt / (a.steps * wl.inflight))
    res["a_constraints_per_s"] = n / (1e-3 * min(res["a_ms_per_proof"]))
    res["b_constraints_per_s"] = n / (1e-3 * min(res["b_ms_per_proof"]))
    res["b_over_a_time"] = min(res["b_ms_per_proof"]) / min(res["a_ms_per_proof"])
    res["c_set_linear_ms"] = wb.set_linear_ms
    res["same_proof_bytes"] = wa.proof_sha256() == wb.proof_sha256()
    res["a_h2d_bytes_per_proof"] = int(wa.host.numel() * 4 + wa.rands.numel() * 4)
    res["b_h2d_bytes_per_proof"] = int(wb.host.numel() * 4)
    print(json.dumps(res))
    wa.close()
    wb.close()
    ctx_b.close()
    ctx.close()
    if not res["same_proof_bytes"]:
        raise SystemExit("legs (a) and (b) produced different proofs")


if __name__ == "__main__":
    main()
