"""GPU: lig_rows_explain / lig_rows_explain_attached / lig_rows_read_slots -- asked constraints of a committed rows job as the library holds
them (terms, coefficient values, committed witness values, right-hand side, residual; csrc/diagnose.hip) and a read-back of committed slots.

Every case compares the attached call with the term-list call on the same trace (same counts, same record BYTES) and with the Python integers
of tests/explain_ref.py, never with itself.  No test hands a kernel an invalid index; the misuse cases check return codes of calls that launch
nothing.  Everything runs at (l, k, n) = (320, 512, 2048) on the 12-row trace of tests/test_gpu_diagnose_attached.py."""
import ctypes as C
import gc

import numpy as np
import pytest

import diagnose_ref as dr
import explain_ref as er
import hip_lib
import linear_ref as lr
import oracle_lib as ol

pytestmark = pytest.mark.gpu

P = ol.P
L_, K_, N_ = SHAPE = (320, 512, 2048)
ONE, NEG_ONE = lr.ONE, lr.NEG_ONE
E_ARG, E_STATE = -1, -3
HEAVY_MIN = 2048                                              # csrc/lin_common.hpp
TERM_COEFS = [0, 1, P - 1, 2, 1 << 200, (1 << 253) + 12345, P - 2, 7]


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


_trace = {}


def base_trace():
    """6 linear rows and 2 triples at (320, 512, 2048): computed once, never changed (the tests copy)"""
    if not _trace:
        kinds, rows, _ = lr.build_trace(L_, K_, N_, 5 * L_ + 17, L_ + 9)
        assert len(kinds) == 12 and all(int(kd) <= 3 for kd in kinds)
        _trace.update(kinds=kinds, rows=rows)
    return _trace["kinds"], _trace["rows"]


def shipped(amd, kinds, rows):
    """(kinds | DRAW_PAD, rows with garbage in the pad slots the library draws)"""
    kinds, msgs = np.asarray(kinds, dtype=np.uint8).copy(), rows.copy()
    msgs[:, L_:] = 0xDEADBEEF
    kinds |= amd.ROW_DRAW_PAD
    return kinds, msgs


def begun(amd, c, kinds, rows):
    k2, msgs = shipped(amd, kinds, rows)
    return c.rows_begin(k2, msgs, generated_at=lr.GEN)


def wit(rows, s):
    return ol.from_limbs(rows[s // L_, s % L_])[0]


def bump(rows, s, d=1):
    rows[s // L_, s % L_] = ol.to_limbs([(wit(rows, s) + d) % P])[0]


class Builder:
    """a linear_ref.System constraint by constraint; b_c is computed from the witness (so the statement holds) unless given.  Right-hand
    sides get table entries of their own, behind the coefficients of the terms, so a test can change them alone."""

    def __init__(self, rows, term_coefs=TERM_COEFS):
        self.w = lr.witness(rows, L_)
        self.term_begin, self.slots, self.cidx, self.rhs_c, self.rhs_b = [0], [], [], [], []
        self.coefs, self.n_term_coefs = list(term_coefs), len(term_coefs)

    def value(self, ci):
        return 1 if ci == ONE else P - 1 if ci == NEG_ONE else self.coefs[ci]

    def add(self, terms, b=None):
        for s, ci in terms:
            assert ci in (ONE, NEG_ONE) or ci < self.n_term_coefs
            self.slots.append(s)
            self.cidx.append(ci)
        self.term_begin.append(len(self.slots))
        if b is None:
            b = sum(self.value(ci) * self.w[s] for s, ci in terms) % P
        c = len(self.term_begin) - 2
        if b:
            self.rhs_c.append(c)
            self.rhs_b.append(len(self.coefs))
            self.coefs.append(b)
        return c

    def system(self):
        return lr.System(self.term_begin, self.slots, self.cidx, self.rhs_c, self.rhs_b, self.coefs, 0)


def with_table(system, tab):
    return lr.System(system.term_begin, system.slots, system.coef_idx, system.rhs_constraint, system.rhs_coef, tab, 0)


_shapes = {}


def shapes_case():
    """the shapes a kernel can get wrong, in one statement that holds on the base trace -> (system, names of the constraints)"""
    if not _shapes:
        kinds, rows = base_trace()
        S = len(kinds) * L_
        rng = np.random.default_rng(23)
        b = Builder(rows)
        at = {}
        at["pm_one"] = b.add([(17, ONE), (S - 1, NEG_ONE), (400, ONE), (3, NEG_ONE)])                    # +1 / -1 only, the last slot of the trace
        at["table"] = b.add([(900, 4), (5, 5), (2500, 7), (5, 3), (1200, 0)])                            # table coefficients only (a zero among them)
        at["thrice"] = b.add([(700, 4), (9, ONE), (700, 7), (700, 4), (700, NEG_ONE)])                   # slot 700: index 4 twice, 7 once, and a special
        at["empty"] = b.add([])
        at["no_rhs"] = b.add([(33, ONE), (33, NEG_ONE), (34, 2), (34, 1)])                               # w - w + (p - 1) w + w: b_c = 0
        assert at["no_rhs"] not in b.rhs_c and at["pm_one"] in b.rhs_c
        at["rhs_only"] = b.add([], b=(1 << 250) + 3)                                                     # a right-hand side and no term: residual -b
        picks = [ONE, NEG_ONE, 3, 4, 5, 7]
        distinct = rng.choice(S, HEAVY_MIN + 1, replace=False)
        at["heavy"] = b.add([(int(s), picks[int(ci)]) for s, ci in zip(distinct, rng.integers(0, 6, HEAVY_MIN + 1))])
        at["mixed"] = b.add([(2000, 6), (1, ONE), (2000, ONE)])
        hot = 10 * L_ + 5                                                                                 # one slot of a triple's row, 2049 times
        at["heavy_one_slot"] = b.add([(hot, picks[int(ci)]) for ci in rng.integers(0, 6, HEAVY_MIN + 1)])
        at["edge"] = b.add([(distinct[0], ONE)] * HEAVY_MIN)                                              # exactly HEAVY_MIN terms
        at["last"] = b.add([(hot, 7), (0, ONE)])
        system = b.system()
        sizes = np.diff(system.term_begin).tolist()
        assert sizes[at["heavy"]] == sizes[at["heavy_one_slot"]] == HEAVY_MIN + 1 and at["last"] == system.n_constraints - 1
        assert [c for c, _ in dr.linear_violations(system, rows, L_)] == [at["rhs_only"]]                # (violated by construction)
        _shapes.update(system=system, at=at, hot=hot)
    return _shapes["system"], _shapes["at"]


def check(amd, c, tr, system, rows, asked, term_cap=1 << 15):
    """explain_attached on `tr` against (a) rows_explain with `system` -- the statement in force, its coefs = the table in force -- and
    (b) the reference over `rows` -> (info, constraint records, term records) of the attached call"""
    asked = [int(a) for a in asked]
    total, rep, want_c, want_t = er.explain(system, rows, L_, asked, term_cap)
    info, con, terms = c.rows_explain_attached(tr, asked, term_cap=term_cap)
    info0, con0, terms0 = c.rows_explain(tr, system.to_binding(amd), asked, term_cap=term_cap)
    print("explain_attached: %d asked, %d terms, %d reported, %.3f ms (with the term list: %.3f ms)" %
          (len(asked), info.n_terms_total, info.n_terms_reported, info.ms_total, info0.ms_total))
    assert (info.n_terms_total, info.n_terms_reported) == (total, rep) == (info0.n_terms_total, info0.n_terms_reported)
    assert len(con) == len(con0) == len(asked) and len(terms) == len(terms0) == rep
    assert con.tobytes() == con0.tobytes() and terms.tobytes() == terms0.tobytes()
    assert er.got_constraints(con) == want_c
    assert er.got_terms(terms) == want_t
    return info, con, terms


# ---------------------------------------------------------------- 1: shapes and asked lists
def test_shapes_and_asked_lists(amd):
    kinds, rows = base_trace()
    system, at = shapes_case()
    NC = system.n_constraints
    c = amd.Context(*SHAPE)
    try:
        tr, keep = begun(amd, c, kinds, rows)
        c.rows_set_linear(tr, system.to_binding(amd))
        c.rows_commit(tr)
        _, con, terms = check(amd, c, tr, system, rows, range(NC))                        # all of them
        assert [int(n) for n in con["n_terms"]] == np.diff(system.term_begin).tolist()
        assert not con["residual"][[i for i in range(NC) if i != at["rhs_only"]]].any()
        assert bytes(con["residual"][at["rhs_only"]]) == er.le32(P - ((1 << 250) + 3))
        seg = terms[int(con["first_term"][at["thrice"]]):][:5]
        assert [(int(t["slot"]), int(t["coef_index"])) for t in seg] == [(9, ONE), (700, 4), (700, 4), (700, 7), (700, NEG_ONE)]
        assert seg[1].tobytes() == seg[2].tobytes()                                       # the term the statement holds twice, twice
        check(amd, c, tr, system, rows, [0])                                              # the first alone
        check(amd, c, tr, system, rows, [NC - 1])                                         # the last alone
        check(amd, c, tr, system, rows, [at["empty"]])                                    # an empty constraint alone: no term at all
        check(amd, c, tr, system, rows, [at["heavy"]])
        check(amd, c, tr, system, rows, [i for i in range(NC) if i != at["heavy"]])       # skips the heavy one
        check(amd, c, tr, system, rows, [at["table"], at["heavy_one_slot"], at["last"]])
        info, con, terms = c.rows_explain_attached(tr, [])                                # nothing asked: nothing returned
        assert (info.n_terms_total, info.n_terms_reported, len(con), len(terms)) == (0, 0, 0, 0)
        c.trace_destroy(tr)
    finally:
        c.close()


# ---------------------------------------------------------------- 2: a bumped witness
def test_bumped_witness_residuals_are_the_diagnose_records(amd):
    kinds, truth = base_trace()
    system, at = shapes_case()
    rows = truth.copy()
    hot = _shapes["hot"]
    heavy_slot = system.slots[system.term_begin[at["heavy"]] + 1000]
    for s, d in ((700, 5), (hot, 3), (heavy_slot, 1), (33, 9)):                           # (33: w - w and (p - 1) w + w elsewhere -- no_rhs still holds)
        bump(rows, s, d)
    NC = system.n_constraints
    c = amd.Context(*SHAPE)
    try:
        tr, keep = begun(amd, c, kinds, rows)
        c.rows_set_linear(tr, system.to_binding(amd))
        c.rows_commit(tr)
        dinfo, lin, _ = c.rows_diagnose_attached(tr, lin_cap=64, quad_cap=0)
        bad = {int(r["constraint"]): bytes(r["residual"]) for r in lin}
        assert dinfo.n_linear_bad == len(bad) and {at["thrice"], at["heavy"], at["heavy_one_slot"], at["last"], at["rhs_only"]} <= set(bad)
        assert at["no_rhs"] not in bad and at["pm_one"] not in bad
        _, con, terms = check(amd, c, tr, system, rows, range(NC))
        for r in con:
            assert bytes(r["residual"]) == bad.get(int(r["constraint"]), bytes(32))
        shown = {int(t["slot"]): bytes(t["value"]) for t in terms}
        for s in (700, hot, heavy_slot, 33):
            assert shown[s] == er.le32(wit(rows, s)) != er.le32(wit(truth, s))
        _, con, _ = check(amd, c, tr, system, rows, sorted(bad))                          # only the violated ones: every residual nonzero
        assert [bytes(r["residual"]) for r in con] == [bad[cn] for cn in sorted(bad)]
        c.trace_destroy(tr)
    finally:
        c.close()


# ---------------------------------------------------------------- 3: term_cap
def test_term_cap(amd):
    kinds, rows = base_trace()
    system, at = shapes_case()
    NC = system.n_constraints
    tb = system.term_begin
    c = amd.Context(*SHAPE)
    try:
        tr, keep = begun(amd, c, kinds, rows)
        with c.linear_prepare(system.to_binding(amd), kinds) as prog:
            c.rows_attach_linear(tr, prog)
        c.rows_commit(tr)
        total = tb[-1]
        full = check(amd, c, tr, system, rows, range(NC), term_cap=total)                 # exactly enough
        for cap in (0, 1, tb[at["thrice"]] + 2, tb[at["heavy"]] + 1000, tb[at["heavy_one_slot"]] + 7, total - 1, total + 5):
            info, con, terms = check(amd, c, tr, system, rows, range(NC), term_cap=cap)   # cap = 0: NULL term array
            assert (info.n_terms_total, info.n_terms_reported) == (total, min(cap, total))
            assert con.tobytes() == full[1].tobytes()                                     # con_out complete whatever the cap
            assert terms.tobytes() == full[2][:cap].tobytes()
        c.trace_destroy(tr)
    finally:
        c.close()


# ---------------------------------------------------------------- 4: values in force
def test_values_in_force(amd):
    kinds, rows = base_trace()
    system, at = shapes_case()
    NC = system.n_constraints
    T = list(system.coefs)
    T2, T3 = list(T), list(T)
    rhs_entry = system.rhs_coef[system.rhs_constraint.index(at["pm_one"])]
    T2[rhs_entry] = (T2[rhs_entry] + 1) % P                   # one right-hand side ...
    T2[4] = (T2[4] + 6) % P                                   # ... and one term coefficient (index 4: table, thrice, heavy ...)
    T3[7] = 11
    c, cb = amd.Context(*SHAPE), amd.Context(*SHAPE)
    try:
        with c.linear_prepare(system.to_binding(amd), kinds) as prog:
            (ta, keep_a), (tb, keep_b) = begun(amd, c, kinds, rows), begun(amd, cb, kinds, rows)
            c.rows_attach_linear(ta, prog)
            cb.rows_attach_linear(tb, prog)
            c.rows_commit(ta)
            cb.rows_commit(tb)
            plain = check(amd, c, ta, system, rows, range(NC))
            c.rows_set_linear_values(ta, T2)                  # the conversion is queued on the side stream: the call orders itself after it
            _, con, terms = check(amd, c, ta, with_table(system, T2), rows, range(NC))
            assert bytes(con["rhs"][at["pm_one"]]) == er.le32(T2[rhs_entry]) and bytes(con["residual"][at["pm_one"]]) == er.le32(P - 1)
            assert {bytes(t["coef"]) for t in terms if int(t["coef_index"]) == 4} == {er.le32(T2[4])}
            assert con["residual"][at["table"]].any() and not con["residual"][at["no_rhs"]].any()
            cb.rows_set_linear_values(tb, T3)                 # two traces on one program, each with its own values
            _, con_b, terms_b = check(amd, cb, tb, with_table(system, T3), rows, range(NC))
            assert {bytes(t["coef"]) for t in terms_b if int(t["coef_index"]) == 7} == {er.le32(11)}
            assert {bytes(t["coef"]) for t in terms_b if int(t["coef_index"]) == 4} == {er.le32(T[4])}
            assert check(amd, c, ta, with_table(system, T2), rows, range(NC))[1].tobytes() == con.tobytes()
            c.rows_set_linear_values(ta, None)                # the program's own table again
            back = check(amd, c, ta, system, rows, range(NC))
            assert back[1].tobytes() == plain[1].tobytes() and back[2].tobytes() == plain[2].tobytes()
            assert check(amd, cb, tb, with_table(system, T3), rows, range(NC))[1].tobytes() == con_b.tobytes()
            c.trace_destroy(ta)
            cb.trace_destroy(tb)
    finally:
        cb.close()
        c.close()


# ---------------------------------------------------------------- 5: released term list, two prepares, two calls
def test_released_term_list_and_two_prepares(amd):
    kinds, truth = base_trace()
    system, at = shapes_case()
    rows = truth.copy()
    bump(rows, _shapes["hot"], 2)
    NC = system.n_constraints
    asked = list(range(NC))
    c = amd.Context(*SHAPE)
    try:
        sysb = system.to_binding(amd)
        p1 = c.linear_prepare(sysb, kinds)
        p2 = c.linear_prepare(system.to_binding(amd), kinds)                             # a second prepare of the same system
        del sysb                                                                          # every array of the term list is gone ...
        gc.collect()
        got = []
        for prog in (p1, p2):
            tr, keep = begun(amd, c, kinds, rows)
            c.rows_attach_linear(tr, prog)
            prog.release()                                                                # ... and so is the caller's reference
            c.rows_commit(tr)
            first = c.rows_explain_attached(tr, asked, term_cap=1 << 15)
            second = c.rows_explain_attached(tr, asked, term_cap=1 << 15)                 # two calls in a row: the same bytes
            assert [a.tobytes() for a in first[1:]] == [a.tobytes() for a in second[1:]]
            assert (first[0].n_terms_total, first[0].n_terms_reported) == (second[0].n_terms_total, second[0].n_terms_reported)
            # against the reference alone first (no term list is handed to the library), then against the term-list call
            total, rep, want_c, want_t = er.explain(system, rows, L_, asked, 1 << 15)
            assert er.got_constraints(first[1]) == want_c and er.got_terms(first[2]) == want_t
            check(amd, c, tr, system, rows, asked)
            got.append(first)
            c.trace_destroy(tr)
        assert [a.tobytes() for a in got[0][1:]] == [a.tobytes() for a in got[1][1:]]     # whichever prepare made the program
    finally:
        c.close()


# ---------------------------------------------------------------- 6: derived product row, mixed operand rows
def test_derived_and_mixed_rows(amd):
    kinds, truth = base_trace()
    rows = truth.copy()
    rng = np.random.default_rng(41)
    QX = [r for r in range(12) if int(kinds[r]) == 1]
    assert len(QX) == 2
    x0, lin0 = QX[0], [r for r in range(12) if int(kinds[r]) == 0][0]
    # first triple: x = bits with three full-width records, y = bytes with two; the linear row lin0 = 16-bit words with three records
    xs = [int(v) for v in rng.integers(0, 2, L_)]
    ys = [int(v) for v in rng.integers(0, 256, L_)]
    ls = [int(v) for v in rng.integers(0, 1 << 16, L_)]
    xs[4], xs[100], xs[L_ - 1] = P - 1, (1 << 200) + 3, 1 << 64
    ys[4], ys[7] = P - 1, (1 << 253) + 1
    ls[0], ls[150], ls[L_ - 1] = P - 2, 1 << 16, (1 << 130) + 5
    zs = [a * b % P for a, b in zip(xs, ys)]
    for r, v in ((x0, xs), (x0 + 1, ys), (x0 + 2, zs), (lin0, ls)):
        rows[r, :L_] = ol.to_limbs(v)
    assert dr.quad_violations(kinds, rows, L_) == []
    widths, wide = amd.mixed_widths(rows, kinds, L_, derive_products=True)
    assert (int(widths[x0]), int(wide[x0])) == (amd.ELEM_BIT, 3) and (int(widths[x0 + 1]), int(wide[x0 + 1])) == (1, 2)
    assert (int(widths[lin0]), int(wide[lin0])) == (2, 3) and [int(widths[r + 2]) for r in QX] == [amd.ELEM_PRODUCT] * 2
    k2, msgs = shipped(amd, kinds, rows)
    msgs[[r + 2 for r in QX]] = 0xDEADBEEF                                                # nothing of the expected products reaches the library
    packed = amd.pack_rows_mixed(msgs, widths, wide, L_)
    # a statement over derived slots, record slots and narrow slots
    z0, z1 = (x0 + 2) * L_, (QX[1] + 2) * L_
    b = Builder(rows)
    on_z = b.add([(z0 + 4, ONE), (z0 + 100, 4), (z1 + 9, NEG_ONE), (x0 * L_ + 4, 3)])   # (p - 1)(p - 1), a record times a byte, a product of the second triple
    on_rec = b.add([(lin0 * L_ + 150, 7), (lin0 * L_ + L_ - 1, ONE), ((x0 + 1) * L_ + 7, 5), (lin0 * L_ + 1, ONE)])
    system = b.system()
    c = amd.Context(*SHAPE)
    try:
        tr, keep = c.rows_begin(k2, packed, generated_at=lr.GEN, elem_bytes=widths, wide_per_row=wide)
        c.rows_set_linear(tr, system.to_binding(amd))
        c.rows_commit(tr)
        # the whole derived row, then records and narrow slots of the mixed rows, in no order and with repeats
        slots = list(range(z0, z0 + L_)) + [z1 + L_ - 1, z1, lin0 * L_ + L_ - 1, x0 * L_ + 100, lin0 * L_, z0 + 4, (x0 + 1) * L_ + 7, x0 * L_ + 4,
                                            lin0 * L_ + 150, z0 + 4, 12 * L_ - 1, 0, x0 * L_ + 5, z0 + 4]
        got = c.rows_read_slots(tr, slots)
        assert got.shape == (len(slots), 8) and got.dtype == np.uint32
        assert (got == er.slot_values(rows, L_, slots)).all()
        assert ol.from_limbs(got[:L_]) == zs and ol.from_limbs(got[4:5]) == [(P - 1) * (P - 1) % P]
        assert ol.from_limbs(got[[L_ + 2, L_ + 3]]) == [ls[L_ - 1], xs[100]]                # the record values
        assert c.rows_read_slots(tr, []).shape == (0, 8)
        _, con, terms = check(amd, c, tr, system, rows, [on_z, on_rec])
        assert not con["residual"].any()
        shown = {int(t["slot"]): int.from_bytes(bytes(t["value"]), "little") for t in terms}
        assert shown[z0 + 4] == zs[4] == 1 and shown[z0 + 100] == zs[100] == ((1 << 200) + 3) * ys[100] % P
        assert shown[z1 + 9] == wit(truth, QX[1] * L_ + 9) * wit(truth, (QX[1] + 1) * L_ + 9) % P
        assert shown[lin0 * L_ + 150] == 1 << 16 and shown[(x0 + 1) * L_ + 7] == (1 << 253) + 1
        _, info = c.rows_prove(tr, None, None)
        assert (info.valid_code, info.valid_linear, info.valid_quad) == (1, 1, 1)
        assert (c.rows_read_slots(tr, slots) == got).all()                                # the proof does not end the window
        c.trace_destroy(tr)
    finally:
        c.close()


# ---------------------------------------------------------------- 7: nothing is disturbed
def test_envelope_is_untouched(amd):
    kinds, truth = base_trace()
    system, at = shapes_case()
    rows = truth.copy()
    bump(rows, 700, 1)
    NC = system.n_constraints
    tab = list(system.coefs)
    tab[7] = 13
    in_force = with_table(system, tab)
    c = amd.Context(*SHAPE)
    try:
        with c.linear_prepare(system.to_binding(amd), kinds) as prog:
            def envelope(when):
                tr, keep = begun(amd, c, kinds, rows)
                c.rows_attach_linear(tr, prog)
                c.rows_set_linear_values(tr, tab)
                c.rows_commit(tr)
                if when == "after commit":
                    check(amd, c, tr, in_force, rows, range(NC))
                    assert (c.rows_read_slots(tr, [700, 0, 3839]) == er.slot_values(rows, L_, [700, 0, 3839])).all()
                proof, info = c.rows_prove(tr, None, None)
                if when == "after prove":
                    check(amd, c, tr, in_force, rows, [at["thrice"], at["heavy"]], term_cap=100)
                    assert (c.rows_read_slots(tr, [700]) == er.slot_values(rows, L_, [700])).all()
                c.trace_destroy(tr)
                return proof, bytes(info.const_sum), bytes(info.stage2_seed), (info.valid_code, info.valid_linear, info.valid_quad)

            plain = envelope("never")
            assert plain[3] == (1, 0, 1)
            assert envelope("after commit") == plain and envelope("after prove") == plain
    finally:
        c.close()


# ---------------------------------------------------------------- 8: window, state and arguments on a real trace
def test_window_state_and_argument_errors(amd):
    kinds, truth = base_trace()
    system, at = shapes_case()
    NC, S = system.n_constraints, len(kinds) * L_
    c = amd.Context(*SHAPE)
    try:
        sysb = system.to_binding(amd)
        con, terms = np.zeros(NC, dtype=amd.EXPLAIN_CONSTRAINT), np.zeros(16, dtype=amd.EXPLAIN_TERM)
        vals = np.zeros((4, 8), dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)

        def info():
            i = amd.ExplainInfo()
            i.struct_bytes = C.sizeof(amd.ExplainInfo)
            return i

        def rc_att(t, asked):
            a = np.asarray(asked, dtype=np.uint32)
            return c.L.lig_rows_explain_attached(t, p(a), len(a), p(con), p(terms), len(terms), C.byref(info()))

        def rc_list(t, asked, sys=sysb):
            a = np.asarray(asked, dtype=np.uint32)
            return c.L.lig_rows_explain(t, C.byref(sys) if sys is not None else None, p(a), len(a), p(con), p(terms), len(terms), C.byref(info()))

        def rc_read(t, slots):
            s = np.asarray(slots, dtype=np.uint32)
            return c.L.lig_rows_read_slots(t, p(s), len(s), p(vals))

        def proves(t):
            _, i = c.rows_prove(t, None, None)
            return (i.valid_code, i.valid_linear, i.valid_quad)

        k2, m0 = shipped(amd, kinds, truth)
        tr, keep = c.rows_begin(k2, m0, generated_at=lr.GEN)
        c.rows_set_linear(tr, sysb)
        assert (rc_att(tr, [0]), rc_list(tr, [0]), rc_read(tr, [0])) == (E_STATE,) * 3    # before the first commit
        c.rows_commit(tr)
        # argument errors: decided on the host, nothing launched; the trace still proves after them
        for asked in ([1, 0], [2, 2], [0, NC], [NC], [0, 5, 4], [0xFFFFFFFF]):            # unsorted, duplicate, out of range
            assert rc_att(tr, asked) == E_ARG and rc_list(tr, asked) == E_ARG
        assert rc_list(tr, [0], sys=None) == E_ARG                                        # the term-list entry without a term list
        assert rc_read(tr, [0, S]) == E_ARG and rc_read(tr, [0xFFFFFFFF]) == E_ARG and rc_read(tr, [S - 1]) == 0
        a = np.zeros(1, dtype=np.uint32)
        assert c.L.lig_rows_explain_attached(tr, p(a), 1, None, p(terms), 16, C.byref(info())) == E_ARG
        assert c.L.lig_rows_explain_attached(tr, p(a), 1, p(con), None, 16, C.byref(info())) == E_ARG
        assert c.L.lig_rows_explain_attached(tr, p(a), 1, p(con), None, 0, C.byref(info())) == 0
        assert c.L.lig_rows_explain_attached(tr, p(a), 1, p(con), p(terms), 16, None) == E_ARG
        short = info()
        short.struct_bytes -= 8
        assert c.L.lig_rows_explain_attached(tr, p(a), 1, p(con), p(terms), 16, C.byref(short)) == E_ARG
        assert c.L.lig_rows_read_slots(tr, None, 0, None) == 0                            # nothing to read: LIG_OK
        bad_sys = system.to_binding(amd, slots=[S] + system.slots[1:])                    # a slot out of range: lig_linear_check rejects it
        assert rc_list(tr, [0], sys=bad_sys) == E_ARG
        check(amd, c, tr, system, truth, [0, at["last"]])
        assert proves(tr) == (1, 0, 1)                                                    # (rhs_only is violated by construction)
        check(amd, c, tr, system, truth, [at["rhs_only"]])                                # the proof does not end the window
        c.rows_restart(tr, m0)                                                            # after prove: straight into the matrix
        assert (rc_att(tr, [0]), rc_list(tr, [0]), rc_read(tr, [0])) == (E_STATE,) * 3
        c.rows_commit(tr)
        check(amd, c, tr, system, truth, [0])
        assert proves(tr) == (1, 0, 1)
        c.trace_destroy(tr)
        # nothing attached: only the attached entry minds
        tr, keep = c.rows_begin(k2, m0, generated_at=lr.GEN)
        c.rows_commit(tr)
        assert rc_att(tr, [0]) == E_STATE and rc_list(tr, [0]) == 0 and rc_read(tr, [5]) == 0
        c.rows_set_linear(tr, sysb)
        check(amd, c, tr, system, truth, [0, 1])
        c.rows_set_linear(tr, None)                                                       # detached again
        assert rc_att(tr, [0]) == E_STATE
        c.rows_set_linear(tr, sysb)
        assert proves(tr) == (1, 0, 1)
        c.trace_destroy(tr)
        tr = c.synth_prepare(700, 330)
        assert (rc_att(tr, [0]), rc_list(tr, [0]), rc_read(tr, [0])) == (E_STATE,) * 3
        c.trace_destroy(tr)
    finally:
        c.close()
