#!/usr/bin/env python3
"""What lig_rows_explain_slots_attached and lig_rows_untouched_slots_attached cost next to lig_rows_explain_attached, in ONE command on one
box.  Records, asserts nothing about speed.

Trace of tools/time_explain.py: the 2^24 single-term-constraint trace (k = 8192, l = 8000, linear rows; constraint c names slot c with
coefficient +1 and has a right-hand side, w_s = b_s, the witnesses taken from a table of 251 values), 1 % of the witness slots changed
after the right-hand sides were fixed, attached to a program prepared from the system whose term list is then released.  The rows hold
rows * l - 2^24 slots behind the last constraint: those are the untouched ones.  One lig_rows_diagnose_attached names the violated
constraints; the asked slots are the slots of their terms (here: their own numbers).  Eight legs ALTERNATE `--rounds` times on the
committed trace (one warm-up round in front, not recorded):

  (s1)  lig_rows_explain_slots_attached for the slot of the first violated constraint, term_cap = 1
  (s2)  ... for the slots of the first 1024
  (s3)  ... of the first 65 536: segment lengths, scan, collect, the order of the m items on the host, then the selection pass of
        lig_rows_explain_attached over the distinct constraints, the value gather and the fill
  (e1)  lig_rows_explain_attached for the same 1 constraint, term_cap = 1
  (e2)  ... the same 1024
  (e3)  ... the same 65 536
  (u0)  lig_rows_untouched_slots_attached, cap = 0: flags and one scan per slice of 2^22 slots, the counts only
  (u1)  ... cap = 65 536: the compaction and the records besides

The output arrays are allocated and touched once, as a C caller keeps them.  The library's own wall time (ms_total, taken at entry) is
recorded; the median of the rounds and their spread are reported.  Every round checks the answers against numpy: value = the committed
witness, coef = 1, constraint_terms = 1, residual = the record of the explain leg, the untouched slots = those behind the last constraint.
Writes a markdown file (default profiles/r20_explain_slots.md) and prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the shape and the package loader; importing it runs nothing)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-constraints", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--asked", type=int, nargs=3, default=[1, 1024, 65536])
    ap.add_argument("--cap", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_explain_slots.md"))
    a = ap.parse_args()
    import ctypes as C
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
    top = max(a.asked)
    if top > len(changed):
        raise SystemExit("only %d constraints are violated at this size: --asked %s is too many" % (len(changed), a.asked))
    free = np.arange(n, R * l, dtype=np.uint32)                  # the slots behind the last constraint: no term touches them
    c = pkg.Context(l, k, n_enc, device=0)
    prog = c.linear_prepare(system, kinds)
    del system                                                   # the caller of lig_linear_prepare who released its term list
    tr, keep = c.rows_begin(kinds, bad, generated_at=1)
    c.rows_attach_linear(tr, prog)
    c.rows_commit(tr)
    dinfo, lin, _ = c.rows_diagnose_attached(tr, lin_cap=top, quad_cap=0)
    if (int(dinfo.n_linear_bad), len(lin)) != (len(changed), top) or not (lin["constraint"] == changed[:top]).all():
        raise SystemExit("lig_rows_diagnose_attached does not name the changed slots")
    names = ["s1", "s2", "s3", "e1", "e2", "e3", "u0", "u1"]
    legs = {key: [] for key in names}
    rec_buf, sterm_buf = np.zeros(top, dtype=pkg.SLOT_RECORD), np.zeros(top, dtype=pkg.SLOT_TERM)
    con_buf, eterm_buf = np.zeros(top, dtype=pkg.EXPLAIN_CONSTRAINT), np.zeros(top, dtype=pkg.EXPLAIN_TERM)
    un_buf = np.zeros(max(a.cap, 1), dtype=pkg.SLOT_VALUE)
    ptr = lambda arr: arr.ctypes.data_as(C.c_void_p)      # noqa: E731

    def slots_call(asked, m):
        info = pkg.SlotInfo()
        info.struct_bytes = C.sizeof(pkg.SlotInfo)
        c.check(c.L.lig_rows_explain_slots_attached(tr, ptr(asked), m, ptr(rec_buf), ptr(sterm_buf), m, C.byref(info)))
        return info, rec_buf[:m], sterm_buf[:info.n_terms_reported]

    def explain_call(asked, m):
        info = pkg.ExplainInfo()
        info.struct_bytes = C.sizeof(pkg.ExplainInfo)
        c.check(c.L.lig_rows_explain_attached(tr, ptr(asked), m, ptr(con_buf), ptr(eterm_buf), m, C.byref(info)))
        return info, con_buf[:m], eterm_buf[:info.n_terms_reported]

    def untouched_call(cap):
        info = pkg.UntouchedInfo()
        info.struct_bytes = C.sizeof(pkg.UntouchedInfo)
        c.check(c.L.lig_rows_untouched_slots_attached(tr, 0, ptr(un_buf) if cap else None, cap, C.byref(info)))
        return info, un_buf[:info.n_reported]

    def timed(leg, out):
        if rnd:
            legs[leg].append(out[0].ms_total)
        return out

    ok = True
    for rnd in range(a.rounds + 1):
        print("round %d of %d" % (rnd, a.rounds), file=sys.stderr, flush=True)
        for i, m in enumerate(a.asked):
            asked = np.ascontiguousarray(lin["constraint"][:m])
            sinfo, rec, sterms = timed("s%d" % (i + 1), slots_call(asked, m))
            einfo, con, eterms = timed("e%d" % (i + 1), explain_call(asked, m))
            w = np.zeros((m, 8), dtype=np.uint32)
            w[:, 0] = asked.astype(np.uint64) % 251 + 1001        # the changed witness
            one = np.zeros((m, 8), dtype=np.uint32)
            one[:, 0] = 1
            ok = ok and (int(sinfo.n_terms_total), int(sinfo.n_terms_reported), int(sinfo.n_constraints_distinct)) == (m, m, m)
            ok = ok and (rec["slot"] == asked).all() and (rec["row_kind"] == 0).all() and (rec["n_terms"] == 1).all() and (rec["first_term"] == np.arange(m)).all()
            ok = ok and rec["value"].tobytes() == w.tobytes() == eterms["value"].tobytes()
            ok = ok and (sterms["slot"] == asked).all() and (sterms["constraint"] == asked).all() and (sterms["coef_index"] == pkg.COEF_ONE).all()
            ok = ok and (sterms["constraint_terms"] == 1).all() and sterms["coef"].tobytes() == one.tobytes()
            ok = ok and sterms["residual"].tobytes() == con["residual"].tobytes() == lin["residual"][:m].tobytes()
        for leg, cap in (("u0", 0), ("u1", a.cap)):
            uinfo, un = timed(leg, untouched_call(cap))
            rep = min(cap, len(free))
            wf = np.zeros((rep, 8), dtype=np.uint32)
            wf[:, 0] = free[:rep].astype(np.uint64) % 251 + 1
            ok = ok and (int(uinfo.n_untouched), int(uinfo.n_untouched_nonzero), int(uinfo.n_reported)) == (len(free), len(free), rep)
            ok = ok and (un["slot"] == free[:rep]).all() and (un["row_kind"] == 0).all() and un["value"].tobytes() == wf.tobytes()
        if not ok:
            raise SystemExit("round %d: an answer differs from the numpy reference" % rnd)
    c.trace_destroy(tr)
    prog.release()
    c.close()
    med = {key: statistics.median(v) for key, v in legs.items()}
    spread = {key: max(v) - min(v) for key, v in legs.items()}
    res = {"constraints": n, "rows": R, "rounds": a.rounds, "changed_slots": int(len(changed)), "asked": a.asked, "cap": a.cap,
           "untouched_slots": int(len(free)), "library_ms": legs, "median_ms": med, "spread_ms": spread, "answers_equal_reference": bool(ok)}
    print(json.dumps(res))
    fmt = lambda v: ", ".join("%.2f" % x for x in v)      # noqa: E731
    what = {"s1": "`lig_rows_explain_slots_attached`, the slot of the first %d violated constraint(s)" % a.asked[0],
            "s2": "`lig_rows_explain_slots_attached`, the slots of the first %d" % a.asked[1],
            "s3": "`lig_rows_explain_slots_attached`, the slots of the first %d" % a.asked[2],
            "e1": "`lig_rows_explain_attached`, the same %d constraint(s)" % a.asked[0],
            "e2": "`lig_rows_explain_attached`, the same %d" % a.asked[1],
            "e3": "`lig_rows_explain_attached`, the same %d" % a.asked[2],
            "u0": "`lig_rows_untouched_slots_attached`, cap = 0 (counts only)",
            "u1": "`lig_rows_untouched_slots_attached`, cap = %d (%d records)" % (a.cap, min(a.cap, len(free)))}
    with open(a.out, "w") as f:
        f.write("# lig_rows_explain_slots_attached and lig_rows_untouched_slots_attached next to lig_rows_explain_attached (tools/time_explain_slots.py)\n\n")
        f.write("Trace: %d single-term constraints w_s = b_s (coefficient +1, one right-hand side each) over %d linear rows at l = %d, k = %d, "
                "attached to a prepared program whose term list was released; %d slots (1 %%) changed after the right-hand sides were fixed; the "
                "%d slots behind the last constraint are touched by no term.  The asked slots are the slots of the terms of the first violated "
                "constraints `lig_rows_diagnose_attached` names.  %d rounds after one warm-up round, the legs alternating inside every round; "
                "times in ms: the library's own wall time of the blocking call (`ms_total`, taken at entry).  The output arrays are allocated "
                "once.  Nothing is asserted about speed.\n\n" % (n, R, l, k, len(changed), len(free), a.rounds))
        f.write("| leg | what | median ms | spread of the rounds, ms | all rounds, ms |\n|---|---|---|---|---|\n")
        for key in names:
            f.write("| (%s) | %s | %.2f | %.2f | %s |\n" % (key, what[key], med[key], spread[key], fmt(legs[key])))
        f.write("\nEvery round, every leg: value = the committed (changed) witness, coef = 1, constraint_terms = 1, residual = the record of the "
                "explain leg and of the diagnose, the untouched slots and their values = those behind the last constraint: %s.\n\n"
                % ("identical" if ok else "DIFFERENT"))
        f.write("A slot call contains the selection pass of `lig_rows_explain_attached` over its distinct constraints (here as many as asked "
                "slots, asked with term_cap = 0) and adds the segment lengths, a scan over the asked slots, the collect, the value gather, the "
                "host order of the items and the fill; the (e) legs also write and copy their term records, which the inner pass does not.  (s) "
                "minus (e), a lower bound of what the slot side adds: %.2f, %.2f and %.2f ms at %d, %d and %d asked slots.\n\n" % (med["s1"] - med["e1"], med["s2"] - med["e2"], med["s3"] - med["e3"], a.asked[0], a.asked[1], a.asked[2]))
        f.write("The untouched pass walks the %d slots of the trace in %d slices of at most 2^22 (one flag kernel, one 64-bit scan and one "
                "blocking read of the two counts per slice); (u1) adds one compaction and one copy for every slice that reports records.\n\n"
                % (R * l, -(-R // max((1 << 22) // l, 1))))
        f.write("`lig_rows_explain_attached` itself is untouched by this change (the slot entries call its pass as it stands), so no leg on a "
                "build of the parent commit is recorded.\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
