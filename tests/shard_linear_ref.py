"""Sparse linear systems on the sharded rows entry, restated in Python: which terms a rank keeps and which constraints it has to sample
under the deal of shard_rows_plan / local_rows_of, and a system every constraint of which lives on one row.  Nothing here calls
lig_linear_shard_count or lig_shard_rows_set_linear."""
import numpy as np

import linear_ref as lr


def python_count(amd, system, kinds, l, rank, world):
    """-> (local_terms, needed_constraints) of `rank`: a term is kept when its row is dealt to the rank; a constraint is needed when it
    has a kept term or lies in the rank's slice [rank * n_rhs // world, (rank + 1) * n_rhs // world) of the right-hand sides"""
    _, b = amd.shard_rows_plan(kinds, world)
    mine = set(amd.local_rows_of(b, rank, world))
    n_rhs = len(system.rhs_constraint)
    needed = set(system.rhs_constraint[rank * n_rhs // world:(rank + 1) * n_rhs // world])
    kept = 0
    for c in range(system.n_constraints):
        for t in range(system.term_begin[c], system.term_begin[c + 1]):
            if system.slots[t] // l in mine:
                kept += 1
                needed.add(c)
    return kept, len(needed)


def nonempty_constraints(system):
    """constraints with a term or a right-hand side: what one rank alone has to sample"""
    return len({c for c in range(system.n_constraints) if system.term_begin[c + 1] > system.term_begin[c]} | set(system.rhs_constraint))


def row_local_system(kinds, l, per_row=6, seed=3, first_random=0):
    """every constraint touches ONE row (1 to 4 slots of it, coefficients +1 / -1); every third has a right-hand side (table entry 0 = 1).
    Only its structure matters here: it is counted, never proved."""
    rng = np.random.default_rng(seed)
    term_begin, slots, cidx, rhs_c, rhs_b = [0], [], [], [], []
    for r in range(len(kinds)):
        if kinds[r] > 3:
            continue
        for _ in range(per_row):
            for col in rng.choice(l, size=int(rng.integers(1, 5)), replace=False):
                slots.append(r * l + int(col))
                cidx.append(lr.ONE if rng.random() < 0.5 else lr.NEG_ONE)
            if (len(term_begin) - 1) % 3 == 0:
                rhs_c.append(len(term_begin) - 1)
                rhs_b.append(0)
            term_begin.append(len(slots))
    return lr.System(term_begin, slots, cidx, rhs_c, rhs_b, [1], first_random)
