"""GPU: lig_rows_diagnose_attached -- the violated constraints of a committed rows job, evaluated against the statement ATTACHED to the
trace (lig_rows_set_linear / lig_rows_attach_linear, with the values of lig_rows_set_linear_values in force): the slot-major index of
the program is regrouped by constraint on the device (csrc/diagnose.hip), no term list is passed.

Every case compares the new call with two things on the same trace, never with itself: lig_rows_diagnose given the term list and the table
in force (same counts, same record BYTES), and the Python integers of tests/diagnose_ref.py.  No test hands a kernel an invalid index; the
misuse cases check return codes of calls that launch nothing."""
import ctypes as C

import numpy as np
import pytest

import diagnose_ref as dr
import hip_lib
import linear_ref as lr
import oracle_lib as ol

pytestmark = pytest.mark.gpu

P = ol.P
L_, K_, N_ = SHAPE = (320, 512, 2048)
ONE, NEG_ONE = lr.ONE, lr.NEG_ONE
E_ARG, E_STATE = -1, -3
HEAVY_MIN = 2048                                              # csrc/lin_common.hpp


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


_trace = {}


def base_trace():
    """the 12-row trace of tests/test_gpu_diagnose.py: 6 linear rows and 2 triples at (320, 512, 2048); its quadratic part holds"""
    if not _trace:
        kinds, rows, _ = lr.build_trace(L_, K_, N_, 5 * L_ + 17, L_ + 9)
        assert len(kinds) == 12 and all(int(kd) <= 3 for kd in kinds)
        assert dr.quad_violations(kinds, rows, L_) == []
        _trace.update(kinds=kinds, rows=rows)
    return _trace["kinds"], _trace["rows"]


def shipped(amd, kinds, rows):
    """(kinds | DRAW_PAD, rows with garbage in the pad slots the library draws)"""
    kinds, msgs = np.asarray(kinds, dtype=np.uint8).copy(), rows.copy()
    draws = (kinds <= 3) | (kinds == amd.ROW_KINDS["INIT"])
    msgs[draws, L_:] = 0xDEADBEEF
    kinds[draws] |= amd.ROW_DRAW_PAD
    return kinds, msgs


def begun(amd, c, kinds, rows):
    """-> (trace, what must stay alive until it is committed)"""
    k2, msgs = shipped(amd, kinds, rows)
    return c.rows_begin(k2, msgs, generated_at=lr.GEN)


def wit(rows, s):
    return ol.from_limbs(rows[s // L_, s % L_])[0]


def bump(rows, s, d=1):
    rows[s // L_, s % L_] = ol.to_limbs([(wit(rows, s) + d) % P])[0]


def diag_info(amd):
    info = amd.DiagInfo()
    info.struct_bytes = C.sizeof(amd.DiagInfo)
    return info


def check(amd, c, tr, system, kinds, rows, lin_cap=1024, quad_cap=1024, want_q=None):
    """diagnose_attached on `tr` against (a) rows_diagnose with `system` -- the statement in force, its coefs = the table in force -- and
    (b) the reference over `rows` -> (linear, quadratic) reference violations"""
    want_l = dr.linear_violations(system, rows, L_) if system is not None else []
    want_q = dr.quad_violations(kinds, rows, L_) if want_q is None else want_q
    info, lin, quad = c.rows_diagnose_attached(tr, lin_cap=lin_cap, quad_cap=quad_cap)
    info0, lin0, quad0 = c.rows_diagnose(tr, system.to_binding(amd) if system is not None else None, lin_cap=lin_cap, quad_cap=quad_cap)
    print("attached: linear %d violated, %d reported; quadratic %d violated, %d reported; %.3f ms (with the term list: %.3f ms)" %
          (info.n_linear_bad, info.n_linear_reported, info.n_quad_bad, info.n_quad_reported, info.ms_total, info0.ms_total))
    counts = (len(want_l), len(want_q), min(lin_cap, len(want_l)), min(quad_cap, len(want_q)))
    assert (info.n_linear_bad, info.n_quad_bad, info.n_linear_reported, info.n_quad_reported) == counts
    assert (info0.n_linear_bad, info0.n_quad_bad, info0.n_linear_reported, info0.n_quad_reported) == counts
    assert lin.tobytes() == lin0.tobytes() and quad.tobytes() == quad0.tobytes()
    assert dr.got_linear(lin) == dr.linear_records(want_l[:lin_cap])
    assert dr.got_quad(quad) == dr.quad_records(want_q[:quad_cap])
    return want_l, want_q


class Builder:
    """a linear_ref.System constraint by constraint; b_c is computed from the witness unless given.  Right-hand sides get table entries of
    their own, behind the coefficients of the terms, so a test can change them alone."""

    def __init__(self, rows, term_coefs=()):
        self.w = lr.witness(rows, L_)
        self.term_begin, self.slots, self.cidx, self.rhs_c, self.rhs_b = [0], [], [], [], []
        self.coefs, self.n_term_coefs = list(term_coefs), len(term_coefs)

    def value(self, ci):
        return 1 if ci == ONE else P - 1 if ci == NEG_ONE else self.coefs[ci]

    def add(self, terms, b=None, off=0):
        for s, ci in terms:
            assert ci in (ONE, NEG_ONE) or ci < self.n_term_coefs
            self.slots.append(s)
            self.cidx.append(ci)
        self.term_begin.append(len(self.slots))
        if b is None:
            b = (sum(self.value(ci) * self.w[s] for s, ci in terms) + off) % P
        c = len(self.term_begin) - 2
        if b:
            self.rhs_c.append(c)
            self.rhs_b.append(len(self.coefs))
            self.coefs.append(b)
        return c

    def system(self):
        return lr.System(self.term_begin, self.slots, self.cidx, self.rhs_c, self.rhs_b, self.coefs, 0)


TERM_COEFS = [0, 1, P - 1, 2, 1 << 200, (1 << 253) + 12345, P - 2, 7]

_seeded = {}


def seeded_case():
    """1500 constraints with 0 to 6 terms over the base trace, +1 / -1 / table coefficients mixed; every third constraint is built from
    pairs (s, +1), (s, -1) and so has no right-hand side (and holds whatever w[s] is); the statement holds"""
    if not _seeded:
        kinds, rows = base_trace()
        rng = np.random.default_rng(17)
        b = Builder(rows, TERM_COEFS)
        S = len(kinds) * L_

        def pick():
            u = rng.random()
            return ONE if u < 0.35 else NEG_ONE if u < 0.6 else int(rng.integers(0, len(TERM_COEFS)))

        for cn in range(1500):
            if cn % 3 == 0:
                terms = [(int(s), ci) for s in rng.integers(0, S, int(rng.integers(0, 4))) for ci in (ONE, NEG_ONE)]
            else:
                terms = [(int(s), pick()) for s in rng.integers(0, S, int(rng.integers(0, 7)))]
            b.add(terms)
        system = b.system()
        sizes = np.diff(system.term_begin)
        assert set(sizes.tolist()) == set(range(7)) and 0 < len(system.rhs_constraint) < 1100
        assert lr.holds(system, rows, L_)
        _seeded.update(system=system)
    return _seeded["system"]


def live_slot(system, start):
    """a slot whose change violates a constraint: the only term of its slot in a constraint >= start, with coefficient +1"""
    for cn in range(start, system.n_constraints):
        seg = range(system.term_begin[cn], system.term_begin[cn + 1])
        for t in seg:
            if system.coef_idx[t] == ONE and [system.slots[u] for u in seg].count(system.slots[t]) == 1:
                return system.slots[t]
    raise AssertionError("no such slot")


def attach(amd, c, tr, system, how):
    """how = "set": lig_rows_set_linear; "prepare": lig_linear_prepare + lig_rows_attach_linear, the caller's reference released at once"""
    if how == "set":
        c.rows_set_linear(tr, system.to_binding(amd))
        return
    prog = c.linear_prepare(system.to_binding(amd), base_trace()[0])
    c.rows_attach_linear(tr, prog)
    prog.release()


# ---------------------------------------------------------------- 1: a seeded system, satisfied and corrupted, attached both ways
@pytest.mark.parametrize("how", ["set", "prepare"])
def test_seeded_system_satisfied_and_corrupted(amd, how):
    kinds, truth = base_trace()
    system = seeded_case()
    bad = truth.copy()
    rng = np.random.default_rng(3)
    touched = sorted(set(system.slots))
    victims = [int(s) for s in rng.choice(touched, size=6, replace=False)]
    for s in victims:
        bump(bad, s, 1 + s)
    c = amd.Context(*SHAPE)
    try:
        for rows in (truth, bad):
            tr, keep = begun(amd, c, kinds, rows)
            attach(amd, c, tr, system, how)
            c.rows_commit(tr)
            want_l, _ = check(amd, c, tr, system, kinds, rows)
            if rows is truth:
                assert want_l == []
            else:
                assert want_l and [cn for cn, _ in want_l] == sorted(cn for cn, _ in want_l)
                for cn, _ in want_l:                          # exactly the constraints that touch a changed slot (and not only through w - w)
                    assert set(victims) & set(system.slots[system.term_begin[cn]:system.term_begin[cn + 1]])
            c.trace_destroy(tr)
    finally:
        c.close()


# ---------------------------------------------------------------- 2: segment edges
def test_segment_edges(amd):
    kinds, truth = base_trace()
    rows = truth.copy()
    last = len(kinds) * L_ - 1                                # the last slot of the last row
    b = Builder(truth, TERM_COEFS)
    e0 = b.add([])                                            # empty constraints at the front ...
    e1 = b.add([])                                            # ... two in a row
    first = b.add([(0, ONE), (last, 7)])
    rhs_only = b.add([], b=(1 << 250) + 3)                    # a right-hand side and no term: residual -b
    rep = b.add([(700, 4), (700, NEG_ONE), (700, 7), (9, ONE)])       # a slot that repeats inside one constraint
    rep_bad = b.add([(701, 4), (701, NEG_ONE), (701, 7)], off=1)
    at_last = b.add([(last, ONE)])
    mid = b.add([])
    last_ok = b.add([(last, NEG_ONE), (last, ONE), (3, 2)])
    e2 = b.add([])                                            # ... and at the end
    system = b.system()
    bump(rows, last, 5)                                       # the last slot of the last row: constraints first (coefficient 7) and at_last
    c = amd.Context(*SHAPE)
    try:
        tr, keep = begun(amd, c, kinds, rows)
        c.rows_set_linear(tr, system.to_binding(amd))
        c.rows_commit(tr)
        want_l, _ = check(amd, c, tr, system, kinds, rows)
        assert want_l == [(first, 35), (rhs_only, P - ((1 << 250) + 3)), (rep_bad, P - 1), (at_last, 5)]
        assert {e0, e1, rep, mid, last_ok, e2}.isdisjoint(cn for cn, _ in want_l)
        c.trace_destroy(tr)
    finally:
        c.close()


# ---------------------------------------------------------------- 3: heavy in both directions
def test_heavy_constraints_and_heavy_slots(amd):
    """constraints with exactly 2048 terms (the lane path) and 2049 (one workgroup per constraint); slots named by 2049 different
    constraints (heavy slot segments of the program, spread over 2049 segments by the regrouping); each satisfied and violated by one slot"""
    kinds, truth = base_trace()
    rows = truth.copy()
    S = len(kinds) * L_
    victim, hot_ok, hot_bad = 11 * L_ + 77, 10 * L_ + 5, 10 * L_ + 6
    free = np.array([s for s in range(S) if s not in (victim, hot_ok, hot_bad)])
    rng = np.random.default_rng(4)
    b = Builder(truth, TERM_COEFS)
    expect = []
    for count in (HEAVY_MIN, HEAVY_MIN + 1):
        for violated in (False, True):
            terms = [(int(s), [ONE, NEG_ONE, 3, 4, 5][int(ci)]) for s, ci in zip(rng.choice(free, count), rng.integers(0, 5, count))]
            if violated:
                terms[count // 2] = (victim, ONE)
            cn = b.add(terms)
            if violated:
                expect.append((cn, 1))
            b.add([(int(rng.choice(free)), ONE)])             # small constraints in between
    for hot, d in ((hot_ok, 0), (hot_bad, 3)):
        for i in range(HEAVY_MIN + 1):
            ci = [ONE, NEG_ONE, 3, 7][i % 4]
            cn = b.add([(hot, ci)] + ([(int(free[i]), ONE)] if i % 5 == 0 else []))
            if d:
                expect.append((cn, d * b.value(ci) % P))
    system = b.system()
    assert [system.term_begin[i + 1] - system.term_begin[i] for i in (0, 2, 4, 6)] == [2048, 2048, 2049, 2049]
    assert system.slots.count(hot_ok) == system.slots.count(hot_bad) == HEAVY_MIN + 1
    bump(rows, victim, 1)
    bump(rows, hot_bad, 3)
    c = amd.Context(*SHAPE)
    try:
        with c.linear_prepare(system.to_binding(amd), kinds) as prog:
            for r in (truth, rows):
                tr, keep = begun(amd, c, kinds, r)
                c.rows_attach_linear(tr, prog)
                c.rows_commit(tr)
                want_l, _ = check(amd, c, tr, system, kinds, r, lin_cap=4096)      # (the victims lie on rows of a triple: its terms are violated too)
                assert want_l == ([] if r is truth else expect)
                c.trace_destroy(tr)
        assert [cn for cn, _ in expect[:2]] == [2, 6] and len(expect) == 2 + HEAVY_MIN + 1
    finally:
        c.close()


# ---------------------------------------------------------------- 4: grid-stride boundary of the regrouping passes
def test_grid_stride_boundary_of_the_regrouping(amd):
    """1024 x 256 + 257 single-term constraints over 3840 slots (every slot about 68 times): lanes of the count and scatter passes take a
    second entry, lanes of the evaluation a second constraint; violations in the first and the last constraint"""
    kinds, truth = base_trace()
    rows = truth.copy()
    S = len(kinds) * L_
    NC = 1024 * 256 + 257
    w = lr.witness(truth, L_)
    # constraint c: w[c * 7 % S] = table[c * 7 % S] -- every slot is named, in an order that is not the slot order
    slot = (np.arange(NC, dtype=np.int64) * 7 + 1) % S
    first_slot, last_slot = int(slot[0]), int(slot[NC - 1])
    only = {s: int(np.count_nonzero(slot == s)) for s in (first_slot, last_slot)}
    system = lr.System(range(NC + 1), slot.tolist(), [ONE] * NC, range(NC), slot.tolist(), w, 0)
    assert system.n_constraints > 1024 * 256 and len(system.slots) > 1024 * 256
    # change the table entry, not the witness: only the first and the last constraint get another right-hand side
    system.coefs = system.coefs + [(w[first_slot] + 9) % P, (w[last_slot] + P - 4) % P]
    system.rhs_coef[0], system.rhs_coef[NC - 1] = S, S + 1
    assert only[first_slot] > 1 and only[last_slot] > 1
    c = amd.Context(*SHAPE)
    try:
        tr, keep = begun(amd, c, kinds, rows)
        with c.linear_prepare(system.to_binding(amd), kinds) as prog:
            c.rows_attach_linear(tr, prog)
        c.rows_commit(tr)
        want_l, _ = check(amd, c, tr, system, kinds, rows, want_q=[])
        assert want_l == [(0, P - 9), (NC - 1, 4)]
        c.trace_destroy(tr)
    finally:
        c.close()


# ---------------------------------------------------------------- 5: values
def test_values_in_force(amd):
    kinds, rows = base_trace()
    system = seeded_case()
    T = list(system.coefs)
    n_fixed = len(TERM_COEFS)
    T2, T3 = list(T), list(T)
    for i in (n_fixed, n_fixed + 10, len(T) - 1):             # right-hand-side entries only
        T2[i] = (T2[i] + 1) % P
    T3[n_fixed + 20] = (T3[n_fixed + 20] + 5) % P

    def with_table(tab):
        return lr.System(system.term_begin, system.slots, system.coef_idx, system.rhs_constraint, system.rhs_coef, tab, 0)

    c, cb = amd.Context(*SHAPE), amd.Context(*SHAPE)
    try:
        with c.linear_prepare(system.to_binding(amd), kinds) as prog:
            (ta, keep_a), (tb, keep_b) = begun(amd, c, kinds, rows), begun(amd, cb, kinds, rows)
            c.rows_attach_linear(ta, prog)
            cb.rows_attach_linear(tb, prog)
            c.rows_commit(ta)
            cb.rows_commit(tb)
            assert check(amd, c, ta, system, kinds, rows, want_q=[])[0] == []
            c.rows_set_linear_values(ta, T2)                  # the conversion is queued on the side stream: the call orders itself after it
            want_l, _ = check(amd, c, ta, with_table(T2), kinds, rows, want_q=[])
            assert [res for _, res in want_l] == [P - 1] * 3
            cb.rows_set_linear_values(tb, T3)                 # two traces on one program, each with its own values
            want_b, _ = check(amd, cb, tb, with_table(T3), kinds, rows, want_q=[])
            assert [res for _, res in want_b] == [P - 5] and want_b[0][0] not in [cn for cn, _ in want_l]
            assert check(amd, c, ta, with_table(T2), kinds, rows, want_q=[])[0] == want_l
            c.rows_set_linear_values(ta, None)                # the program's own table again
            assert check(amd, c, ta, system, kinds, rows, want_q=[])[0] == []
            assert check(amd, cb, tb, with_table(T3), kinds, rows, want_q=[])[0] == want_b
            c.trace_destroy(ta)
            cb.trace_destroy(tb)
    finally:
        cb.close()
        c.close()


# ---------------------------------------------------------------- 6: caps
def test_caps(amd):
    kinds, truth = base_trace()
    system = seeded_case()
    rows = truth.copy()
    rng = np.random.default_rng(8)
    on_linear_rows = sorted(s for s in set(system.slots) if int(kinds[s // L_]) == 0)
    for s in rng.choice(on_linear_rows, size=12, replace=False):
        bump(rows, int(s), 2)
    rows[7, 3, 0] ^= 1                                        # z of both triples: quadratic violations
    rows[7, 200, 1] ^= 4
    rows[11, 319, 0] ^= 1
    want_q = dr.quad_violations(kinds, rows, L_)
    assert len(want_q) == 3
    c = amd.Context(*SHAPE)
    try:
        tr, keep = begun(amd, c, kinds, rows)
        c.rows_set_linear(tr, system.to_binding(amd))
        c.rows_commit(tr)
        want_l, _ = check(amd, c, tr, system, kinds, rows, want_q=want_q)
        assert len(want_l) >= 8
        check(amd, c, tr, system, kinds, rows, lin_cap=0, quad_cap=0, want_q=want_q)          # NULL arrays: counts only
        check(amd, c, tr, system, kinds, rows, lin_cap=3, quad_cap=1024, want_q=want_q)       # the first three, ascending; all are counted
        check(amd, c, tr, system, kinds, rows, lin_cap=1024, quad_cap=2, want_q=want_q)
        check(amd, c, tr, system, kinds, rows, lin_cap=1, quad_cap=1, want_q=want_q)
        c.trace_destroy(tr)
    finally:
        c.close()


# ---------------------------------------------------------------- 7: window and state
def test_window_and_state(amd):
    kinds, truth = base_trace()
    system = seeded_case()
    other = truth.copy()
    bump(other, live_slot(system, 5), 1)
    assert dr.linear_violations(system, other, L_)
    c = amd.Context(*SHAPE)
    try:
        sysb = system.to_binding(amd)

        def rc(t, lin_cap=0, quad_cap=0):
            return c.L.lig_rows_diagnose_attached(t, None, lin_cap, None, quad_cap, C.byref(diag_info(amd)))

        def proves(t):
            _, info = c.rows_prove(t, None, None)
            return (info.valid_code, info.valid_linear, info.valid_quad)

        k2, m0 = shipped(amd, kinds, truth)
        _, m1 = shipped(amd, kinds, other)
        tr, keep = c.rows_begin(k2, m0, generated_at=lr.GEN)
        c.rows_set_linear(tr, sysb)
        assert rc(tr) == E_STATE                              # before the first commit
        c.rows_commit(tr)
        assert rc(tr, lin_cap=5) == E_ARG and rc(tr, quad_cap=5) == E_ARG          # a NULL array with a cap > 0
        short = diag_info(amd)
        short.struct_bytes -= 8
        assert c.L.lig_rows_diagnose_attached(tr, None, 0, None, 0, C.byref(short)) == E_ARG
        assert c.L.lig_rows_diagnose_attached(tr, None, 0, None, 0, None) == E_ARG
        c.rows_restart(tr, m1)                                # between commit and prove: the second matrix, the window stays open
        check(amd, c, tr, system, kinds, truth, want_q=[])
        assert proves(tr) == (1, 1, 1)
        check(amd, c, tr, system, kinds, truth, want_q=[])    # the proof does not end the window
        c.rows_commit(tr)
        assert check(amd, c, tr, system, kinds, other, want_q=[])[0]
        assert proves(tr) == (1, 0, 1)
        c.rows_restart(tr, m0)                                # after prove: straight into the matrix
        assert rc(tr) == E_STATE
        c.rows_commit(tr)
        check(amd, c, tr, system, kinds, truth, want_q=[])
        assert proves(tr) == (1, 1, 1)
        c.trace_destroy(tr)
        # nothing attached
        tr, keep = c.rows_begin(k2, m0, generated_at=lr.GEN)
        c.rows_commit(tr)
        assert rc(tr) == E_STATE
        c.rows_set_linear(tr, sysb)
        check(amd, c, tr, system, kinds, truth, want_q=[])
        c.rows_set_linear(tr, None)                           # detached again
        assert rc(tr) == E_STATE
        c.rows_set_linear(tr, sysb)
        assert proves(tr) == (1, 1, 1)
        c.trace_destroy(tr)
        tr = c.synth_prepare(700, 330)
        assert rc(tr) == E_STATE
        c.trace_destroy(tr)
    finally:
        c.close()


# ---------------------------------------------------------------- 8: nothing is disturbed
def test_nothing_is_disturbed(amd):
    kinds, truth = base_trace()
    system = seeded_case()
    rows = truth.copy()
    bump(rows, live_slot(system, 40), 1)
    tab = list(system.coefs)
    tab[len(TERM_COEFS) + 3] = (tab[len(TERM_COEFS) + 3] + 1) % P
    in_force = lr.System(system.term_begin, system.slots, system.coef_idx, system.rhs_constraint, system.rhs_coef, tab, 0)
    c, cb = amd.Context(*SHAPE), amd.Context(*SHAPE)
    try:
        with c.linear_prepare(system.to_binding(amd), kinds) as prog:
            def envelope(cx, when, r=rows):
                tr, keep = begun(amd, cx, kinds, r)
                cx.rows_attach_linear(tr, prog)
                cx.rows_set_linear_values(tr, tab)
                cx.rows_commit(tr)
                if when == "after commit":
                    first = cx.rows_diagnose_attached(tr)
                    second = cx.rows_diagnose_attached(tr)    # a second call: the same bytes
                    assert first[0].n_linear_bad >= 2
                    assert [a.tobytes() for a in first[1:]] == [a.tobytes() for a in second[1:]]
                    assert (first[0].n_linear_bad, first[0].n_quad_bad) == (second[0].n_linear_bad, second[0].n_quad_bad)
                    check(amd, cx, tr, in_force, kinds, r, want_q=[])
                proof, info = cx.rows_prove(tr, None, None)
                if when == "after prove":
                    check(amd, cx, tr, in_force, kinds, r, want_q=[])
                cx.trace_destroy(tr)
                return proof, bytes(info.const_sum), bytes(info.stage2_seed), (info.valid_code, info.valid_linear, info.valid_quad)

            plain = envelope(c, "never")
            assert plain[3] == (1, 0, 1)
            assert envelope(c, "after commit") == plain and envelope(c, "after prove") == plain
            # a second trace on the same program, proved around a diagnosis of the first
            usual = envelope(cb, "never", truth)
            (ta, keep_a), (tb, keep_b) = begun(amd, c, kinds, rows), begun(amd, cb, kinds, truth)
            c.rows_attach_linear(ta, prog)
            cb.rows_attach_linear(tb, prog)
            cb.rows_set_linear_values(tb, tab)
            c.rows_commit(ta)
            cb.rows_commit(tb)
            check(amd, c, ta, system, kinds, rows, want_q=[])
            proof, info = cb.rows_prove(tb, None, None)
            check(amd, c, ta, system, kinds, rows, want_q=[])
            assert (proof, bytes(info.const_sum), bytes(info.stage2_seed)) == usual[:3]
            c.trace_destroy(ta)
            cb.trace_destroy(tb)
    finally:
        cb.close()
        c.close()


# ---------------------------------------------------------------- 9: the quadratic part alone
def test_quadratic_part_alone(amd):
    kinds, truth = base_trace()
    empty = lr.System([0], [], [], [], [], [], 0)             # zero constraints
    c = amd.Context(*SHAPE)
    try:
        # a trace without any quadratic term, a small system attached
        lin_kinds = [0] * 12
        rows = np.zeros((12, K_, 8), dtype=np.uint32)
        rows[:, :L_] = ol.rand_field(np.random.default_rng(31), 12 * L_).reshape(12, L_, 8)
        b = Builder(rows)
        b.add([(3, ONE), (400, NEG_ONE)])
        bad = b.add([(3, ONE)], off=1)
        tr, keep = begun(amd, c, lin_kinds, rows)
        c.rows_set_linear(tr, b.system().to_binding(amd))
        c.rows_commit(tr)
        want_l, want_q = check(amd, c, tr, b.system(), lin_kinds, rows)
        assert want_l == [(bad, P - 1)] and want_q == []
        c.trace_destroy(tr)
        # a system with zero constraints attached: what rows_diagnose(trace, None) gives
        rows = truth.copy()
        rows[7, 5, 0] ^= 1
        rows[11, 300, 2] ^= 8
        tr, keep = begun(amd, c, kinds, rows)
        c.rows_set_linear(tr, empty.to_binding(amd))
        c.rows_commit(tr)
        _, want_q = check(amd, c, tr, None, kinds, rows)
        assert len(want_q) == 2
        check(amd, c, tr, empty, kinds, rows, want_q=want_q)
        c.trace_destroy(tr)
    finally:
        c.close()
