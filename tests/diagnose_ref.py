"""The yardstick of lig_rows_diagnose, in Python integers: the residual of every linear constraint of a linear_ref.System and of every
(quadratic term, column < l) over a row matrix.  Nothing here calls the library under test.

    linear     res_c = sum_j a_cj * w[slot_cj] - b_c  mod p
    quadratic  x[i] * y[i] - z[i] for a QX,QY,QZ / BQX,BQY,BQZ triple, b[i] * b[i] - b[i] for a BIT row (x = y = z = that row),
               x[i] - z[i] for an EQX,EQY pair (y = 0xFFFFFFFF) -- the terms of quad_terms() in csrc/rows_plan.hpp, in its order"""
import numpy as np

import linear_ref as lr
import oracle_lib as ol

P = ol.P
NO_ROW = 0xFFFFFFFF
QZ, BIT, EQY, BQZ = 3, 5, 7, 10


def quad_terms(kinds):
    """-> [(x, y, z)] row indices, the rule of quad_terms() (csrc/rows_plan.hpp) restated"""
    out = []
    for r, kd in enumerate(int(v) & 0x7F for v in kinds):
        if kd in (QZ, BQZ):
            out.append((r - 2, r - 1, r))
        elif kd == BIT:
            out.append((r, r, r))
        elif kd == EQY:
            out.append((r - 1, NO_ROW, r))
    return out


def linear_violations(system, rows, l):
    """-> [(constraint, residual)] with a nonzero residual, ascending"""
    w = dict(enumerate(lr.witness(rows, l))) if len(system.slots) > 20000 else {}      # (a large system: every slot at once)

    def wit(s):
        if s not in w:
            w[s] = ol.from_limbs(rows[s // l, s % l])[0]
        return w[s]

    rhs = dict(zip(system.rhs_constraint, system.rhs_coef))
    out = []
    for c in range(system.n_constraints):
        acc = 0
        for t in range(system.term_begin[c], system.term_begin[c + 1]):
            acc += system.coef(system.coef_idx[t]) * wit(system.slots[t])
        if c in rhs:
            acc -= system.coef(rhs[c])
        if acc % P:
            out.append((c, acc % P))
    return out


def quad_violations(kinds, rows, l):
    """-> [(row_x, row_y, row_z, column, residual)] with a nonzero residual, ascending (term, column)"""
    out = []
    for x, y, z in quad_terms(kinds):
        if x == y == z:
            # a bit row: b * b - b = 0 exactly for b in {0, 1} (a field has no zero divisors); only the other slots need integers
            d = rows[x, :l]
            cols = np.flatnonzero(d[:, 1:].any(axis=1) | (d[:, 0] > 1))
            for i in cols:
                b = ol.from_limbs(d[i])[0]
                out.append((x, y, z, int(i), (b * b - b) % P))
            continue
        xs, zs = ol.from_limbs(rows[x, :l]), ol.from_limbs(rows[z, :l])
        ys = ol.from_limbs(rows[y, :l]) if y != NO_ROW else None
        for i in range(l):
            res = (xs[i] - zs[i]) % P if ys is None else (xs[i] * ys[i] - zs[i]) % P
            if res:
                out.append((x, y, z, i, res))
    return out


def residual_bytes(v):
    return int(v).to_bytes(32, "little")


def linear_records(viol):
    """what lig_rows_diagnose reports for these violations: [(constraint, residual bytes)]"""
    return [(c, residual_bytes(r)) for c, r in viol]


def quad_records(viol):
    return [(x, y, z, i, residual_bytes(r)) for x, y, z, i, r in viol]


def got_linear(rec):
    """numpy DIAG_LINEAR records -> the same form"""
    return [(int(r["constraint"]), bytes(r["residual"])) for r in rec]


def got_quad(rec):
    return [(int(r["row_x"]), int(r["row_y"]), int(r["row_z"]), int(r["column"]), bytes(r["residual"])) for r in rec]


def holds(system, rows, l):
    return not linear_violations(system, rows, l)
