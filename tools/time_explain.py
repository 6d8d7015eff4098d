#!/usr/bin/env python3
"""What lig_rows_explain_attached and lig_rows_read_slots cost next to lig_rows_diagnose_attached, in ONE command on one box.  Records,
asserts nothing about speed.

Trace of tools/time_diagnose_attached.py: the 2^24 single-term-constraint trace (k = 8192, l = 8000, linear rows; constraint c names slot c
with coefficient +1 and has a right-hand side, w_s = b_s, the witnesses taken from a table of 251 values), 1 % of the witness slots changed
after the right-hand sides were fixed, attached to a program prepared from the system.  Six legs ALTERNATE `--rounds` times on the
committed trace (one warm-up round in front, not recorded):

  (d)   lig_rows_diagnose_attached, lin_cap = 65 536: names the violated constraints (count, scan, scatter over the program's entries, then
        the evaluation of every constraint)
  (e1)  lig_rows_explain_attached for the first violated constraint (d) reported, term_cap = 1
  (e2)  ... for the first 1024
  (e3)  ... for the first 65 536: one mark pass over the program's entries, a scan, a collect, the order of the m items on the host,
        fill and finish
  (e3w) as (e3) through Context.rows_explain_attached, which allocates fresh numpy output arrays per call (pages the copy touches first)
  (r)   lig_rows_read_slots of 65 536 random slots

The output arrays of (e1), (e2), (e3) and (r) are allocated and touched once, as a C caller keeps them.

Two clocks per call: the library's own wall time (ms_total, taken at entry; lig_rows_read_slots has none) and the wall time around the
ctypes call; the median of the rounds is reported.  Every round checks the answers against numpy: residual = the record of (d), value =
the committed witness, coef = 1, rhs = the table entry.
Writes a markdown file (default profiles/r16_explain.md) and prints one JSON line."""
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
    ap.add_argument("--asked", type=int, nargs=3, default=[1, 1024, 65536])
    ap.add_argument("--slots", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_explain.md"))
    a = ap.parse_args()
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
    lin_cap = max(a.asked)
    if lin_cap > len(changed):
        raise SystemExit("only %d constraints are violated at this size: --asked %s is too many" % (len(changed), a.asked))
    slots = rng.integers(0, R * l, a.slots).astype(np.uint32)
    want_slots = bad.reshape(R * k, 8)[(slots.astype(np.int64) // l) * k + slots % l]
    c = pkg.Context(l, k, n_enc, device=0)
    prog = c.linear_prepare(system, kinds)
    del system                                                   # the caller of lig_linear_prepare who released its term list
    tr, keep = c.rows_begin(kinds, bad, generated_at=1)
    c.rows_attach_linear(tr, prog)
    c.rows_commit(tr)
    names = ["d", "e1", "e2", "e3", "e3w", "r"]
    legs, outer = {key: [] for key in names}, {key: [] for key in names}
    ok = True
    # the output arrays of the explain legs and of (r): allocated and touched once, as a C caller keeps them
    import ctypes as C
    con_buf, terms_buf = np.zeros(lin_cap, dtype=pkg.EXPLAIN_CONSTRAINT), np.zeros(lin_cap, dtype=pkg.EXPLAIN_TERM)
    vals_buf = np.zeros((a.slots, 8), dtype=np.uint32)
    ptr = lambda arr: arr.ctypes.data_as(C.c_void_p)      # noqa: E731

    def explain(asked, m):
        info = pkg.ExplainInfo()
        info.struct_bytes = C.sizeof(pkg.ExplainInfo)
        c.check(c.L.lig_rows_explain_attached(tr, ptr(asked), m, ptr(con_buf), ptr(terms_buf), m, C.byref(info)))
        return info, con_buf[:m], terms_buf[:info.n_terms_reported]

    def read():
        c.check(c.L.lig_rows_read_slots(tr, ptr(slots), len(slots), ptr(vals_buf)))
        return vals_buf

    def timed(leg, call):
        t0 = time.perf_counter()
        out = call()
        dt = 1e3 * (time.perf_counter() - t0)
        if rnd:
            outer[leg].append(dt)
            if leg != "r":
                legs[leg].append(out[0].ms_total)
        return out

    for rnd in range(a.rounds + 1):
        print("round %d of %d" % (rnd, a.rounds), file=sys.stderr, flush=True)
        dinfo, lin, _ = timed("d", lambda: c.rows_diagnose_attached(tr, lin_cap=lin_cap, quad_cap=0))
        ok = ok and (int(dinfo.n_linear_bad), len(lin)) == (len(changed), lin_cap) and (lin["constraint"] == changed[:lin_cap]).all()
        for leg, m in zip(("e1", "e2", "e3"), a.asked):
            asked = np.ascontiguousarray(lin["constraint"][:m])
            info, con, terms = timed(leg, lambda: explain(asked, m))
            w = np.zeros((m, 8), dtype=np.uint32)
            w[:, 0] = asked.astype(np.uint64) % 251 + 1001        # the changed witness ...
            b = np.zeros((m, 8), dtype=np.uint32)
            b[:, 0] = asked.astype(np.uint64) % 251 + 1            # ... and the right-hand side it was changed against
            one = np.zeros((m, 8), dtype=np.uint32)
            one[:, 0] = 1
            ok = ok and (int(info.n_terms_total), int(info.n_terms_reported)) == (m, m)
            ok = ok and (con["constraint"] == asked).all() and (con["n_terms"] == 1).all() and (con["first_term"] == np.arange(m)).all()
            ok = ok and con["residual"].tobytes() == lin["residual"][:m].tobytes() and con["rhs"].tobytes() == b.tobytes()
            ok = ok and (terms["constraint"] == asked).all() and (terms["slot"] == asked).all() and (terms["coef_index"] == pkg.COEF_ONE).all()
            ok = ok and terms["coef"].tobytes() == one.tobytes() and terms["value"].tobytes() == w.tobytes()
        asked = np.ascontiguousarray(lin["constraint"][:a.asked[2]])
        winfo, wcon, wterms = timed("e3w", lambda: c.rows_explain_attached(tr, asked, term_cap=a.asked[2]))
        ok = ok and wcon.tobytes() == con.tobytes() and wterms.tobytes() == terms.tobytes()
        got = timed("r", read)
        ok = bool(ok and (got == want_slots).all())
        if not ok:
            raise SystemExit("round %d: an answer differs from the numpy reference" % rnd)
    c.trace_destroy(tr)
    prog.release()
    c.close()
    med = {key: statistics.median(v) for key, v in legs.items() if v}
    med_outer = {key: statistics.median(v) for key, v in outer.items()}
    held = med["e1"] <= med["d"]
    res = {"constraints": n, "rows": R, "rounds": a.rounds, "changed_slots": int(len(changed)), "asked": a.asked, "slots_read": a.slots,
           "library_ms": legs, "around_the_call_ms": outer, "median_ms": med, "median_around_the_call_ms": med_outer,
           "answers_equal_reference": ok, "mark_pass_no_dearer_than_regrouping": held}
    print(json.dumps(res))
    fmt = lambda v: ", ".join("%.2f" % x for x in v)      # noqa: E731
    what = {"d": "`lig_rows_diagnose_attached`, lin_cap = %d" % lin_cap,
            "e1": "`lig_rows_explain_attached`, the first %d violated constraint(s) of (d)" % a.asked[0],
            "e2": "`lig_rows_explain_attached`, the first %d" % a.asked[1],
            "e3": "`lig_rows_explain_attached`, the first %d" % a.asked[2],
            "e3w": "as (e3) through `Context.rows_explain_attached`: fresh numpy output arrays in every call",
            "r": "`lig_rows_read_slots`, %d random slots" % a.slots}
    with open(a.out, "w") as f:
        f.write("# lig_rows_explain_attached and lig_rows_read_slots next to lig_rows_diagnose_attached (tools/time_explain.py)\n\n")
        f.write("Trace: %d single-term constraints w_s = b_s (coefficient +1, one right-hand side each) over %d linear rows at l = %d, k = %d, "
                "attached to a prepared program whose term list was released; %d slots (1 %%) changed after the right-hand sides were fixed.  "
                "%d rounds after one warm-up round, the legs alternating inside every round; times in ms: the library's own wall time of the "
                "blocking call (`ms_total`, taken at entry; `lig_rows_read_slots` reports none) and the wall time around the call.  The output "
                "arrays of (e1), (e2), (e3) and (r) are allocated once; (e3w) allocates them per call.  Nothing is asserted about speed.\n\n" % (n, R, l, k, len(changed), a.rounds))
        f.write("| leg | what | median ms | median ms around the call | all rounds, ms (library; around the call for (r)) |\n|---|---|---|---|---|\n")
        for key in names:
            f.write("| (%s) | %s | %s | %.2f | %s |\n" % (key, what[key], "%.2f" % med[key] if key in med else "--", med_outer[key],
                                                      fmt(legs[key] or outer[key])))
        f.write("\nEvery round, every leg: residual = the record of (d), value = the committed (changed) witness, coef = 1, rhs = the table entry, "
                "the slots read = the matrix that was shipped: %s.\n\n" % ("identical" if ok else "DIFFERENT"))
        f.write("Expectation checked: one mark pass over the program's %d entries (plus scan, collect and the right-hand-side index) costs no more "
                "than the count / scan / scatter regrouping and evaluation of the attached diagnose.  Median of (e1) %.2f ms against (d) %.2f ms: "
                "it %s.\n\n" % (n, med["e1"], med["d"], "held" if held else "did NOT hold"))
        f.write("(e3w) and (e3) are the same library call with the same output bytes; they differ in the caller's output arrays alone (%d bytes "
                "of records): pages the device-to-host copy is the first to touch.  Rounds of (e3w): %.2f .. %.2f ms against %.2f .. %.2f ms for "
                "(e3).\n\n" % (168 * a.asked[2], min(legs["e3w"]), max(legs["e3w"]), min(legs["e3"]), max(legs["e3"])))
        f.write("Scratch of one attached explain call at this size: %d bytes for marks and positions, %d for the right-hand-side index, and per "
                "asked constraint here 4 + 20 + 88 + 84 bytes (asked list, items, records).\n" % (8 * (n + 1), 4 * n))
    return 0


if __name__ == "__main__":
    sys.exit(main())
