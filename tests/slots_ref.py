"""The yardstick of lig_rows_explain_slots* / lig_rows_untouched_slots*, in Python integers, built on linear_ref, diagnose_ref and
explain_ref.  Nothing here calls the library under test.

For the asked slots (strictly ascending) of a linear_ref.System over a row matrix:
    slot record   (slot, row_kind, n_terms, first_term, w[slot]): n_terms = ALL terms of the statement on the slot, first_term = the index
                  of its first term in the full order
    term record   (slot, constraint, coef_index, constraint_terms, coefficient value, residual of the constraint) in ascending (asked slot,
                  constraint, coef_index as an unsigned number) order -- the specials 0xFFFFFFFE / 0xFFFFFFFF last --, a repeated term
                  repeated; the first term_cap.  The residuals are explain_ref.explain's.
The untouched slots: the slots of the rows of kind <= 3 (LINEAR, QX, QY, QZ) that no term names, ascending, each with its kind and value."""
import explain_ref as er
import linear_ref as lr
import oracle_lib as ol

P = ol.P
le32 = er.le32


def explain_slots(system, kinds, rows, l, asked, term_cap):
    """-> (n_terms_total, n_terms_reported, n_constraints_distinct, slot records, term records)"""
    asked = [int(s) for s in asked]
    assert all(a < b for a, b in zip(asked, asked[1:])) and all(0 <= s < len(kinds) * l for s in asked)
    want = set(asked)
    on = {s: [] for s in asked}
    for c in range(system.n_constraints):
        for t in range(system.term_begin[c], system.term_begin[c + 1]):
            s = int(system.slots[t])
            if s in want:
                on[s].append((c, int(system.coef_idx[t])))
    distinct = sorted({c for s in asked for c, _ in on[s]})
    res = {c: r for c, _, _, _, r in er.explain(system, rows, l, distinct, 0)[2]}
    size = {c: system.term_begin[c + 1] - system.term_begin[c] for c in distinct}
    recs, terms = [], []
    for s in asked:
        w = ol.from_limbs(rows[s // l, s % l])[0]
        recs.append((s, int(kinds[s // l]) & 0x7F, len(on[s]), len(terms), le32(w)))
        for c, ci in sorted(on[s]):
            terms.append((s, c, ci, size[c], le32(system.coef(ci) % P), res[c]))
    return len(terms), min(len(terms), term_cap), len(distinct), recs, terms[:term_cap]


def got_slots(rec):
    """numpy SLOT_RECORD records -> the same form"""
    return [(int(r["slot"]), int(r["row_kind"]), int(r["n_terms"]), int(r["first_term"]), bytes(r["value"])) for r in rec]


def got_terms(rec):
    return [(int(r["slot"]), int(r["constraint"]), int(r["coef_index"]), int(r["constraint_terms"]), bytes(r["coef"]), bytes(r["residual"]))
            for r in rec]


def untouched(system, kinds, rows, l, nonzero_only, cap):
    """-> (n_untouched, n_untouched_nonzero, n_reported, [(slot, row_kind, value)]): the first `cap` of the selected slots"""
    touched = set(int(s) for s in system.slots)
    w = lr.witness(rows, l)
    every = [(r * l + col, int(kinds[r]) & 0x7F) for r in range(len(kinds)) if (int(kinds[r]) & 0x7F) <= 3 for col in range(l)]
    free = [(s, kd, w[s]) for s, kd in every if s not in touched]
    nonzero = [x for x in free if x[2]]
    pick = (nonzero if nonzero_only else free)[:cap]
    return len(free), len(nonzero), len(pick), [(s, kd, le32(v)) for s, kd, v in pick]


def got_values(rec):
    return [(int(r["slot"]), int(r["row_kind"]), bytes(r["value"])) for r in rec]


__all__ = ["explain_slots", "got_slots", "got_terms", "untouched", "got_values", "le32"]
