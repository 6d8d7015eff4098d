#!/usr/bin/env python3
"""What lig_rows_diagnose costs next to a proof, in ONE command on one box.  Records, asserts nothing about speed.

Shape: the 2^24 single-term-constraint trace of tools/bench_linear_system.py (k = 8192, l = 8000, linear rows; constraint c = slot c,
coefficient +1).  Here every constraint has a right-hand side, w_s = b_s, with the witnesses taken from a table of 251 values so that the
statement fits a small coefficient table.  Four legs ALTERNATE `--rounds` times (one warm-up round in front, not recorded):

  (a) lig_rows_diagnose on the committed trace, every constraint satisfied
  (b) the same with 1 % of the witness slots changed after the right-hand sides were fixed (reported: the first `--cap` of them)
  (c) one lig_rows_prove of the same trace (stages 2 + 3 with the system attached), for scale
  (d) as (a), with the constraints in a random order: constraint c names slot perm[c].  In (a) and (b) constraint c names slot c, so the
      "random" 32-byte witness gather of the evaluation pass is in fact a sequential read; (d) is the random-access case

(a), (b) and (d) are the whole blocking call: the host pass of lig_linear_check over the term list, the upload of the term list (12 bytes
per constraint for term_begin and the terms, 8 for the right-hand sides, from pageable memory here), the passes, the scan and the copy of
the records.  Two clocks are recorded per call: the library's own wall time (lig_diag_info.ms_total, taken at entry) and the wall time
around the ctypes call; the median of the rounds is reported.
Writes a markdown file (default profiles/r12_diagnose.md) and prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the shape and the package loader; importing it runs nothing)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-constraints", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_diagnose.md"))
    a = ap.parse_args()
    import numpy as np
    pkg = bench.load_pkg()
    l, k, n_enc = bench.L_, bench.K_, bench.N_
    n = 1 << a.log2_constraints
    R = -(-n // l)
    kinds = np.full(R, pkg.ROW_KINDS["LINEAR"] | pkg.ROW_DRAW_PAD, dtype=np.uint8)
    good = np.zeros((R, k, 8), dtype=np.uint32)
    good[:, :l, 0] = (np.arange(R * l, dtype=np.uint64) % 251 + 1).reshape(R, l)        # w[s] = table[s % 251]
    bad = good.copy()
    rng = np.random.default_rng(12)
    changed = np.sort(rng.choice(n, size=n // 100, replace=False))
    bad.reshape(R * k, 8)[(changed // l) * k + changed % l, 0] += 1000
    cons = np.arange(n, dtype=np.uint32)
    system = pkg.LinearSystem.make(np.arange(n + 1, dtype=np.uint32), cons, np.full(n, pkg.COEF_ONE, dtype=np.uint32), cons, cons % 251,
                                   list(range(1, 252)))
    perm = rng.permutation(n).astype(np.uint32)
    system_perm = pkg.LinearSystem.make(np.arange(n + 1, dtype=np.uint32), perm, np.full(n, pkg.COEF_ONE, dtype=np.uint32), cons, perm % 251,
                                        list(range(1, 252)))
    c = pkg.Context(l, k, n_enc, device=0)
    tr, keep = c.rows_begin(kinds, good, generated_at=1)
    c.rows_set_linear(tr, system)
    legs = {"a": [], "b": [], "c": [], "d": []}
    outer = {"a": [], "b": [], "d": []}

    def diagnose(leg, sysb):
        t0 = time.perf_counter()
        info, _, _ = c.rows_diagnose(tr, sysb, lin_cap=a.cap, quad_cap=0)
        dt = 1e3 * (time.perf_counter() - t0)
        counts[leg] = (int(info.n_linear_bad), int(info.n_linear_reported))
        if rnd:
            legs[leg].append(info.ms_total)
            outer[leg].append(dt)

    counts = {}
    loaded = True
    for rnd in range(a.rounds + 1):
        for leg, rows in (("a", good), ("b", bad)):
            if not loaded:
                c.rows_restart(tr, rows)
            loaded = False
            c.rows_commit(tr)
            diagnose(leg, system)
            if leg == "a":
                diagnose("d", system_perm)
            _, pinfo = c.rows_prove(tr, None, None, copy=False)
            if rnd:
                legs["c"].append(pinfo.ms_total - pinfo.ms_stage1)
    c.trace_destroy(tr)
    c.close()
    if counts["a"] != (0, 0) or counts["d"] != (0, 0) or counts["b"] != (len(changed), min(a.cap, len(changed))):
        raise SystemExit("diagnose counted %s, expected 0 and %d violated constraints" % (counts, len(changed)))
    med = {key: statistics.median(v) for key, v in legs.items()}
    med_outer = {key: statistics.median(v) for key, v in outer.items()}
    gather_bytes = 32 * n + 8 * n
    res = {"constraints": n, "rows": R, "rounds": a.rounds, "cap": a.cap, "changed_slots": int(len(changed)),
           "a_diagnose_satisfied_ms": legs["a"], "b_diagnose_1pct_bad_ms": legs["b"], "c_rows_prove_stage23_ms": legs["c"],
           "d_diagnose_random_order_ms": legs["d"], "around_the_call_ms": outer, "median_ms": med, "median_around_the_call_ms": med_outer,
           "term_list_upload_bytes": 12 * n + 4 + 8 * n, "gather_plus_term_bytes": gather_bytes}
    print(json.dumps(res))
    fmt = lambda v: ", ".join("%.2f" % x for x in v)      # noqa: E731
    with open(a.out, "w") as f:
        f.write("# lig_rows_diagnose next to a proof (tools/time_diagnose.py)\n\n")
        f.write("Trace: %d single-term constraints w_s = b_s (coefficient +1, one right-hand side each) over %d linear rows at l = %d, k = %d; "
                "%d rounds after one warm-up round, the legs alternating inside every round; times in ms: the library's own wall time of the "
                "blocking call (`lig_diag_info.ms_total`, taken at entry) and, second, the wall time around the ctypes call.  Nothing is "
                "asserted about speed.\n\n" % (n, R, l, k, a.rounds))
        f.write("| leg | what | median ms | median ms around the call | all rounds, ms |\n|---|---|---|---|---|\n")
        f.write("| (a) | `lig_rows_diagnose`, every constraint satisfied (counts 0 / 0); constraint c names slot c: a sequential witness read | %.2f | %.2f | %s |\n" %
                (med["a"], med_outer["a"], fmt(legs["a"])))
        f.write("| (b) | the same, %d slots (1 %%) changed: %d violated, the first %d reported | %.2f | %.2f | %s |\n" %
                (len(changed), counts["b"][0], counts["b"][1], med["b"], med_outer["b"], fmt(legs["b"])))
        f.write("| (c) | `lig_rows_prove` of the same trace (stages 2 + 3, system attached), for scale | %.2f | | %s |\n" % (med["c"], fmt(legs["c"])))
        f.write("| (d) | as (a), constraints in a random order (constraint c names slot perm[c]): the random 32-byte gather | %.2f | %.2f | %s |\n\n" %
                (med["d"], med_outer["d"], fmt(legs["d"])))
        f.write("Inside (a), (b) and (d): the host pass of `lig_linear_check` over the term list (one step per term, on one core), the upload "
                "of the caller's term list from pageable host memory (%d bytes: `term_begin`, the terms, the "
                "right-hand sides), the evaluation pass (a random 32-byte gather per term plus 8 bytes of term read: %d bytes), the scan of "
                "the flags and the copy of the records.\n" % (res["term_list_upload_bytes"], gather_bytes))
    return 0


if __name__ == "__main__":
    sys.exit(main())
