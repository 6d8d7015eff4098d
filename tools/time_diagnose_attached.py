#!/usr/bin/env python3
"""What lig_rows_diagnose_attached costs next to lig_rows_diagnose, in ONE command on one box.  Records, asserts nothing about speed.

Trace and protocol of tools/time_diagnose.py: the 2^24 single-term-constraint trace (k = 8192, l = 8000, linear rows; constraint c names
one slot with coefficient +1 and has a right-hand side, w_s = b_s, the witnesses taken from a table of 251 values), 1 % of the witness
slots changed after the right-hand sides were fixed.  Three legs ALTERNATE `--rounds` times on the committed trace (one warm-up round in
front, not recorded):

  (a) lig_rows_diagnose with the caller's term list: the host pass of lig_linear_check, the upload from pageable memory, the passes
  (b) lig_rows_diagnose_attached on the same trace, attached to a program prepared from the same system: no host pass, no upload; the
      slot-major index of the program is regrouped by constraint on the device (count, scan, scatter), then the same passes
  (c) as (b), with the constraints in a random order (constraint c names slot perm[c]): the scatter of the regrouping and the witness
      gather of the evaluation are then random accesses.  The trace is re-attached to the other program between the legs, off the clock.

Two clocks per call: the library's own wall time (lig_diag_info.ms_total, taken at entry) and the wall time around the ctypes call; the
median of the rounds is reported.  The records of (a) and (b) are compared byte for byte in every round, those of (c) with
lig_rows_diagnose given the permuted term list (warm-up round).
--parent-tree DIR: a built checkout of the parent commit.  Its tools/time_diagnose.py is run first, in a child process of its own (same
box, same session); its leg (b) is this file's leg (a) on a library without the new entry, and is recorded next to it.
Writes a markdown file (default profiles/r15_diagnose_attached.md) and prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the shape and the package loader; importing it runs nothing)


def parent_leg(tree, log2n, rounds, cap):
    """leg (b) of the parent's tools/time_diagnose.py -> its JSON line (None: no parent tree given)"""
    if not tree:
        return None
    tree = os.path.abspath(tree)
    out = os.path.join(tree, "parent_r12_diagnose.md")
    p = subprocess.run([sys.executable, os.path.join(tree, "tools", "time_diagnose.py"), "--log2-constraints", str(log2n), "--rounds", str(rounds),
                        "--cap", str(cap), "--out", out], cwd=tree, capture_output=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit("the parent's tools/time_diagnose.py failed: %s" % p.stderr.decode()[-2000:])
    return json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-constraints", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_diagnose_attached.md"))
    a = ap.parse_args()
    parent = parent_leg(a.parent_tree, a.log2_constraints, a.rounds, a.cap)
    print("parent leg: %s" % ("done" if parent else "none"), file=sys.stderr, flush=True)
    import numpy as np
    pkg = bench.load_pkg()
    l, k, n_enc = bench.L_, bench.K_, bench.N_
    n = 1 << a.log2_constraints
    R = -(-n // l)
    kinds = np.full(R, pkg.ROW_KINDS["LINEAR"] | pkg.ROW_DRAW_PAD, dtype=np.uint8)
    bad = np.zeros((R, k, 8), dtype=np.uint32)
    bad[:, :l, 0] = (np.arange(R * l, dtype=np.uint64) % 251 + 1).reshape(R, l)        # w[s] = table[s % 251]
    rng = np.random.default_rng(12)
    changed = np.sort(rng.choice(n, size=n // 100, replace=False))
    bad.reshape(R * k, 8)[(changed // l) * k + changed % l, 0] += 1000
    cons = np.arange(n, dtype=np.uint32)
    ones = np.full(n, pkg.COEF_ONE, dtype=np.uint32)
    system = pkg.LinearSystem.make(np.arange(n + 1, dtype=np.uint32), cons, ones, cons, cons % 251, list(range(1, 252)))
    perm = rng.permutation(n).astype(np.uint32)
    system_perm = pkg.LinearSystem.make(np.arange(n + 1, dtype=np.uint32), perm, ones, cons, perm % 251, list(range(1, 252)))
    c = pkg.Context(l, k, n_enc, device=0)
    prog, prog_perm = c.linear_prepare(system, kinds), c.linear_prepare(system_perm, kinds)
    tr, keep = c.rows_begin(kinds, bad, generated_at=1)
    c.rows_attach_linear(tr, prog)
    c.rows_commit(tr)
    legs = {"a": [], "b": [], "c": []}
    outer = {"a": [], "b": [], "c": []}
    counts, same = {}, {"ab": True, "c": None}

    def timed(leg, call):
        t0 = time.perf_counter()
        info, lin, _ = call()
        dt = 1e3 * (time.perf_counter() - t0)
        counts[leg] = (int(info.n_linear_bad), int(info.n_linear_reported))
        if rnd:
            legs[leg].append(info.ms_total)
            outer[leg].append(dt)
        return lin.tobytes()

    for rnd in range(a.rounds + 1):
        print("round %d of %d" % (rnd, a.rounds), file=sys.stderr, flush=True)
        got_a = timed("a", lambda: c.rows_diagnose(tr, system, lin_cap=a.cap, quad_cap=0))
        got_b = timed("b", lambda: c.rows_diagnose_attached(tr, lin_cap=a.cap, quad_cap=0))
        same["ab"] = same["ab"] and got_a == got_b
        c.rows_attach_linear(tr, prog_perm)
        got_c = timed("c", lambda: c.rows_diagnose_attached(tr, lin_cap=a.cap, quad_cap=0))
        if not rnd:
            same["c"] = got_c == c.rows_diagnose(tr, system_perm, lin_cap=a.cap, quad_cap=0)[1].tobytes()
        c.rows_attach_linear(tr, prog)
    c.trace_destroy(tr)
    prog.release()
    prog_perm.release()
    c.close()
    want = (len(changed), min(a.cap, len(changed)))
    if counts != {"a": want, "b": want, "c": want} or not same["ab"] or not same["c"]:
        raise SystemExit("diagnose counted %s (expected %s each), records equal: %s" % (counts, want, same))
    med = {key: statistics.median(v) for key, v in legs.items()}
    med_outer = {key: statistics.median(v) for key, v in outer.items()}
    passes = 32 * n + 2 * 4 * (n + 1)                        # residuals, flags, scan positions: both entries
    scratch_a = 4 * (n + 1) + 8 * n + 4 * n + 4 * n + 4 * n + 32 * 251 + passes
    scratch_b = 4 * (n + 1) + 4 * (n + 1) + 8 * n + 4 * n + 4 * (n // 2049 + 1) + 4 + passes
    res = {"constraints": n, "rows": R, "rounds": a.rounds, "cap": a.cap, "changed_slots": int(len(changed)),
           "a_diagnose_term_list_ms": legs["a"], "b_diagnose_attached_ms": legs["b"], "c_diagnose_attached_random_order_ms": legs["c"],
           "around_the_call_ms": outer, "median_ms": med, "median_around_the_call_ms": med_outer, "records_a_equal_b": same["ab"],
           "records_c_equal_term_list": same["c"], "scratch_bytes_a": scratch_a, "scratch_bytes_b": scratch_b,
           "term_list_upload_bytes": 12 * n + 4 + 8 * n}
    if parent:
        res["parent_a_ms"] = parent["b_diagnose_1pct_bad_ms"]
        res["parent_a_median_ms"] = parent["median_ms"]["b"]
        res["parent_a_median_around_the_call_ms"] = parent["median_around_the_call_ms"]["b"]
    print(json.dumps(res))
    fmt = lambda v: ", ".join("%.2f" % x for x in v)      # noqa: E731
    with open(a.out, "w") as f:
        f.write("# lig_rows_diagnose_attached next to lig_rows_diagnose (tools/time_diagnose_attached.py)\n\n")
        f.write("Trace: %d single-term constraints w_s = b_s (coefficient +1, one right-hand side each) over %d linear rows at l = %d, k = %d, "
                "%d slots (1 %%) changed after the right-hand sides were fixed: %d violated, the first %d reported.  %d rounds after one warm-up "
                "round, the legs alternating inside every round; times in ms: the library's own wall time of the blocking call "
                "(`lig_diag_info.ms_total`, taken at entry) and, second, the wall time around the ctypes call.  Nothing is asserted about "
                "speed.\n\n" % (n, R, l, k, len(changed), want[0], want[1], a.rounds))
        f.write("| leg | what | median ms | median ms around the call | all rounds, ms |\n|---|---|---|---|---|\n")
        f.write("| (a) | `lig_rows_diagnose` with the term list (host check, upload, passes); constraint c names slot c | %.2f | %.2f | %s |\n" %
                (med["a"], med_outer["a"], fmt(legs["a"])))
        f.write("| (b) | `lig_rows_diagnose_attached`, the same trace attached to a program prepared from the same system | %.2f | %.2f | %s |\n" %
                (med["b"], med_outer["b"], fmt(legs["b"])))
        f.write("| (c) | as (b), constraints in a random order (constraint c names slot perm[c]) | %.2f | %.2f | %s |\n" %
                (med["c"], med_outer["c"], fmt(legs["c"])))
        if parent:
            pa = res["parent_a_ms"]
            f.write("| (a), parent | leg (a) on a build of the parent commit (its `tools/time_diagnose.py`, leg (b) there), a process of its own, same "
                    "box and session | %.2f | %.2f | %s |\n" % (res["parent_a_median_ms"], res["parent_a_median_around_the_call_ms"], fmt(pa)))
        f.write("\nRecords of (a) and (b) byte for byte, every round: %s.  Records of (c) against `lig_rows_diagnose` with the permuted term "
                "list: %s.\n\n" % ("identical" if same["ab"] else "DIFFERENT", "identical" if same["c"] else "DIFFERENT"))
        if parent:
            lo, hi = min(pa), max(pa)
            f.write("Leg (a) is not meant to change: its median here is %.2f ms, the five rounds of the parent's own leg span %.2f .. %.2f ms "
                    "(%s that spread).\n\n" % (med["a"], lo, hi, "inside" if lo <= med["a"] <= hi else "OUTSIDE"))
        else:
            f.write("No build of the parent commit was measured in this run (`--parent-tree`).\n\n")
        f.write("Scratch of one call at this size: (a) %d bytes -- the uploaded system (`term_begin`, terms, right-hand sides, `rhs_index`, the "
                "table) plus residuals, flags and scan positions; (b) %d bytes -- `cbegin`, the cursor, the regrouped terms, `rhs_index`, the "
                "heavy list, plus the same residuals, flags and scan positions.  (a) also moves %d bytes of term list over the link from "
                "pageable memory; (b) moves none.\n" % (scratch_a, scratch_b, res["term_list_upload_bytes"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
