"""The yardstick of lig_rows_explain / lig_rows_explain_attached / lig_rows_read_slots, in Python integers, built on linear_ref and
diagnose_ref.  Nothing here calls the library under test.

For the asked constraints (strictly ascending) of a linear_ref.System over a row matrix:
    constraint record   (constraint, n_terms, first_term, b_c, residual): n_terms = ALL its terms, first_term = the index of its first term
                        in the full order, b_c = the table entry named by rhs_coef (0 when the constraint has none),
                        residual = sum a * w - b_c mod p
    term record         (constraint, slot, coef_index, coefficient value, w[slot]) in ascending (asked constraint, slot, coef_index as an
                        unsigned number) order -- the specials 0xFFFFFFFE / 0xFFFFFFFF last --, a repeated term repeated; the first term_cap"""
import numpy as np

import diagnose_ref as dr
import linear_ref as lr
import oracle_lib as ol

P = ol.P


def le32(v):
    return int(v).to_bytes(32, "little")


def explain(system, rows, l, asked, term_cap):
    """-> (n_terms_total, n_terms_reported, constraint records, term records): every field value a Python integer or 32 bytes"""
    asked = [int(c) for c in asked]
    assert all(a < b for a, b in zip(asked, asked[1:])) and all(0 <= c < system.n_constraints for c in asked)
    rhs = dict(zip(system.rhs_constraint, system.rhs_coef))
    cons, terms = [], []
    for c in asked:
        seg = sorted((int(system.slots[t]), int(system.coef_idx[t])) for t in range(system.term_begin[c], system.term_begin[c + 1]))
        b = system.coef(rhs[c]) % P if c in rhs else 0
        acc = 0
        first = len(terms)
        for s, ci in seg:
            w = ol.from_limbs(rows[s // l, s % l])[0]
            a = system.coef(ci) % P
            acc += a * w
            terms.append((c, s, ci, le32(a), le32(w)))
        cons.append((c, len(seg), first, le32(b), le32((acc - b) % P)))
    return len(terms), min(len(terms), term_cap), cons, terms[:term_cap]


def got_constraints(rec):
    """numpy EXPLAIN_CONSTRAINT records -> the same form (reserved must be zero)"""
    assert not rec["reserved"].any()
    return [(int(r["constraint"]), int(r["n_terms"]), int(r["first_term"]), bytes(r["rhs"]), bytes(r["residual"])) for r in rec]


def got_terms(rec):
    assert not rec["reserved"].any()
    return [(int(r["constraint"]), int(r["slot"]), int(r["coef_index"]), bytes(r["coef"]), bytes(r["value"])) for r in rec]


def residuals(system, rows, l, asked):
    """-> {constraint: residual} of the asked constraints, through explain()"""
    return {c: int.from_bytes(res, "little") for c, _, _, _, res in explain(system, rows, l, asked, 0)[2]}


def slot_values(rows, l, slots):
    """-> (n, 8) uint32: the committed elements lig_rows_read_slots returns"""
    slots = np.asarray(slots, dtype=np.int64)
    return np.ascontiguousarray(rows[slots // l, slots % l]).astype(np.uint32).reshape(len(slots), 8)


__all__ = ["explain", "got_constraints", "got_terms", "residuals", "slot_values", "le32", "dr", "lr"]
