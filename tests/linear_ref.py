"""The yardstick of the sparse linear systems (lig_linear_system), in Python integers: traces with known witnesses, seeded systems
over them, and the two formulas

    Rn[slot s] = sum over terms (c, s, a) of a * r_c  (mod p)          const_sum = - sum_c b_c * r_c  (mod p)

with r_c = element first_random + c of the oracle's AES-256-CTR field stream keyed by the stage-1 seed (oracle_lib.rng_fill, pinned
to the reference's generate_random by tests/golden/aes_ctr.json).  Nothing here calls the library under test."""
import numpy as np

import oracle_lib as ol

P = ol.P
ONE, NEG_ONE = 0xFFFFFFFF, 0xFFFFFFFE
GEN = 31


class System:
    """term_begin / slots / coef_idx / rhs_constraint / rhs_coef / coefs (Python integers) / first_random"""

    def __init__(self, term_begin, slots, coef_idx, rhs_constraint, rhs_coef, coefs, first_random):
        self.term_begin, self.slots, self.coef_idx = list(term_begin), list(slots), list(coef_idx)
        self.rhs_constraint, self.rhs_coef, self.coefs, self.first_random = list(rhs_constraint), list(rhs_coef), list(coefs), first_random

    @property
    def n_constraints(self):
        return len(self.term_begin) - 1

    def coef(self, idx):
        return 1 if idx == ONE else P - 1 if idx == NEG_ONE else self.coefs[idx]

    def to_binding(self, amd, **override):
        kw = dict(term_begin=self.term_begin, slots=self.slots, coef_idx=self.coef_idx, rhs_constraint=self.rhs_constraint,
                  rhs_coef=self.rhs_coef, coefs=self.coefs, first_random=self.first_random)
        kw.update(override)
        return amd.LinearSystem.make(**kw)


def expected(system, stage1_seed, rows, l, k):
    """-> (Rn as (rows, k, 8) uint32, const_sum bytes): the two formulas, term by term"""
    nc = system.n_constraints
    r = ol.from_limbs(ol.rng_fill(stage1_seed, system.first_random, nc)) if nc else []
    acc = {}
    for c in range(nc):
        for t in range(system.term_begin[c], system.term_begin[c + 1]):
            s = system.slots[t]
            acc[s] = (acc.get(s, 0) + system.coef(system.coef_idx[t]) * r[c]) % P
    rn = np.zeros((rows, k, 8), dtype=np.uint32)
    if acc:
        slots = sorted(acc)
        limbs = ol.to_limbs([acc[s] for s in slots])
        for s, v in zip(slots, limbs):
            rn[s // l, s % l] = v
    cs = 0
    for c, b in zip(system.rhs_constraint, system.rhs_coef):
        cs = (cs + system.coef(b) * r[c]) % P
    return rn, ((P - cs) % P).to_bytes(32, "little")


def witness(rows, l):
    """the data slots of every row as Python integers: w[row * l + column]"""
    return ol.from_limbs(np.ascontiguousarray(rows[:, :l]).reshape(-1, 8))


def build_trace(l, k, n, n_lin, n_quad, prog=None, seed=5, narrow=False):
    """-> (kinds, rows, masks): the oracle's row stream (its pads and masks) with seeded witnesses in the data slots -- full-width
    field elements, or (narrow) bits and 16-bit values; z = x * y.  A few linear-row slots are made equal in pairs: equal_pairs().
    With a batch program in front the rows stay the job's own (the oracle proves batch rows only as part of its synthetic job)."""
    job = ol.make_job(l, k, n, 192, n_lin, n_quad, generated_at=GEN, threads=8)
    if prog is not None:
        prog.attach(job)
    rows, mc, ml, mq = ol.form_rows(job)
    kinds = ol.row_kinds(job).copy()
    rows = rows.copy()
    if prog is not None:
        return kinds, rows, (mc, ml, mq)
    rng = np.random.default_rng(seed)
    j = 0
    for r in range(len(kinds)):
        if kinds[r] == 0:
            if narrow:
                rows[r, :l] = 0
                rows[r, :l, 0] = rng.integers(0, 2 if j % 2 else 1 << 16, l).astype(np.uint32)
            else:
                rows[r, :l] = ol.rand_field(rng, l)
            j += 1
        elif kinds[r] == 1:
            hi = 2 if narrow else 1 << 32
            x, y = rng.integers(0, hi, l, dtype=np.uint64), rng.integers(0, hi, l, dtype=np.uint64)
            for d, v in enumerate((x, y, x * y)):
                rows[r + d, :l] = 0
                rows[r + d, :l, 0] = (v & 0xFFFFFFFF).astype(np.uint32)
                rows[r + d, :l, 1] = (v >> 32).astype(np.uint32)
    for a, b in equal_pairs(kinds, l):
        rows[b // l, b % l] = rows[a // l, a % l]
    return kinds, rows, (mc, ml, mq)


def linear_rows(kinds):
    return [r for r in range(len(kinds)) if kinds[r] == 0]


def equal_pairs(kinds, l, count=200):
    """(slot, slot) pairs on the first two linear rows whose witnesses build_trace makes equal"""
    lr = linear_rows(kinds)
    if len(lr) < 2:
        return []
    return [(lr[0] * l + i, lr[1] * l + (i * 7 + 3) % l) for i in range(min(count, l // 8))]


def make_system(kinds, rows, l, n_constraints, first_random, seed, hot_terms=20000):
    """A seeded system over the trace whose statement HOLDS (b_c is computed from the witness).  On purpose: slots with 0, 1, 2 and
    several terms; one slot with >= hot_terms terms; a slot repeated inside one constraint; constraints without terms; the table
    coefficients 0, 1 and p - 1 next to the two specials; powers of two and full-width coefficients; one row no term touches."""
    rng = np.random.default_rng(seed)
    w = witness(rows, l)
    ok_rows = [r for r in range(len(kinds)) if kinds[r] <= 3]
    untouched = ok_rows[len(ok_rows) // 2]                       # a LINEAR / Q row without any term
    pool = np.array([r * l + c for r in ok_rows if r != untouched for c in range(l)], dtype=np.int64)
    singles, free = pool[3], set(int(s) for s in pool[4:40])     # pool[3]: exactly one term; pool[4:40]: no term at all
    hot = int(pool[0])
    draw = pool[~np.isin(pool, list(free) + [int(singles), hot, int(pool[1]), int(pool[2])])]
    coefs = [0, 1, P - 1] + [1 << e for e in (1, 2, 7, 31, 32, 64, 200, 253)] + [int(v) for v in ol.from_limbs(ol.rand_field(rng, 40))]
    n_fixed = len(coefs)
    term_begin, slots, cidx, rhs_c, rhs_b, b_index = [0], [], [], [], [], {}

    def pick_coef():
        u = rng.random()
        return ONE if u < 0.4 else NEG_ONE if u < 0.7 else int(rng.integers(0, n_fixed))

    sysm = System(term_begin, slots, cidx, rhs_c, rhs_b, coefs, first_random)
    for c in range(n_constraints):
        terms = []
        if c == 0:
            terms = [(int(singles), ONE)]
        elif c == 1:                                            # pool[1] exactly twice, inside ONE constraint; pool[2] exactly twice, in two
            terms = [(int(pool[1]), 5), (int(pool[1]), NEG_ONE), (int(pool[2]), ONE)]
        elif c == 2:
            terms = [(int(pool[2]), 12)]
        elif c % 97 == 5:
            terms = []                                          # a constraint without terms
        else:
            for s in rng.choice(draw, size=int(rng.integers(1, 5))):
                terms.append((int(s), pick_coef()))
            if c % 11 == 0:
                terms.append((terms[0][0], pick_coef()))        # a slot repeated inside the constraint
        if 3 <= c < 3 + hot_terms:
            terms.append((hot, pick_coef()))
        b = 0
        for s, ci in terms:
            slots.append(s)
            cidx.append(ci)
            b = (b + sysm.coef(ci) * w[s]) % P
        term_begin.append(len(slots))
        if b:
            if b not in b_index:
                b_index[b] = len(coefs)
                coefs.append(b)
            rhs_c.append(c)
            rhs_b.append(b_index[b])
    sysm.__init__(term_begin, slots, cidx, rhs_c, rhs_b, coefs, first_random)
    sysm.untouched_row, sysm.single_slot, sysm.hot_slot = untouched, int(singles), hot
    return sysm


def make_equality_system(kinds, l, first_random):
    """the pure +1 / -1 / right-hand side 0 system: w[a] - w[b] = 0 for the pairs build_trace made equal"""
    pairs = equal_pairs(kinds, l)
    slots, cidx = [], []
    for a, b in pairs:
        slots += [a, b]
        cidx += [ONE, NEG_ONE]
    return System(range(0, 2 * len(pairs) + 1, 2), slots, cidx, [], [], [], first_random)


def holds(system, rows, l):
    """the statement itself, in integers: sum_j a_cj * w[slot_cj] == b_c for every constraint"""
    w = witness(rows, l)
    rhs = dict(zip(system.rhs_constraint, system.rhs_coef))
    for c in range(system.n_constraints):
        lhs = sum(system.coef(system.coef_idx[t]) * w[system.slots[t]] for t in range(system.term_begin[c], system.term_begin[c + 1])) % P
        if lhs != (system.coef(rhs[c]) if c in rhs else 0):
            return False
    return True


def oracle_commitment(l, k, n, n_lin, n_quad, prog):
    """-> (root, stage-1 seed) of the oracle's own prover over the synthetic job with a batch program in front: the rows of
    build_trace(prog=...) are that job's rows, and both values depend on the committed rows and the public data only"""
    import ctypes as C
    job = ol.make_job(l, k, n, 192, n_lin, n_quad, generated_at=GEN, threads=8)
    prog.attach(job)
    pr = ol.Proof()
    assert ol.lib().lo_prove(C.byref(job), C.byref(pr)) == 0
    out = bytes(pr.root), bytes(pr.stage1_seed)
    ol.lib().lo_proof_free(C.byref(pr))
    return out


def oracle_envelope(l, k, n, kinds, rows, masks, system):
    """-> (stage-1 seed, Rn, const_sum, the oracle's proof dict): commit once without randomness for the seed (as
    tests/golden/make_ref_backend.py does), restate matrix and constant, prove"""
    p0 = ol.prove_rows(l, k, n, 192, kinds, rows, *masks, None, None, generated_at=GEN, threads=8)
    rn, cs = expected(system, p0["stage1_seed"], len(kinds), l, k)
    p1 = ol.prove_rows(l, k, n, 192, kinds, rows, *masks, rn, cs, generated_at=GEN, threads=8)
    assert p1["root"] == p0["root"] and p1["stage1_seed"] == p0["stage1_seed"]
    return p0["stage1_seed"], rn, cs, p1
