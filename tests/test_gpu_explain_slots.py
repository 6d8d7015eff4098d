"""GPU: lig_rows_explain_slots* / lig_rows_untouched_slots* -- the constraints through asked slots of a committed rows job (their sizes,
coefficient values and residuals; csrc/diagnose.hip) and the witness slots no linear constraint touches.

Every case compares the attached call with the term-list call on the same trace (same counts, same record BYTES) and both with the Python
integers of tests/slots_ref.py, never a call with itself.  No test hands a kernel an invalid index; the misuse cases check return codes of
calls that launch nothing.  Everything runs at (l, k, n) = (320, 512, 2048) on the 12-row trace of tests/test_gpu_explain.py."""
import collections
import ctypes as C
import gc

import numpy as np
import pytest

import explain_ref as er
import hip_lib
import linear_ref as lr
import oracle_lib as ol
import slots_ref as sr
from test_gpu_explain import HEAVY_MIN, Builder, base_trace, begun, bump, shapes_case, shipped, wit, with_table

pytestmark = pytest.mark.gpu

P = ol.P
L_, K_, N_ = SHAPE = (320, 512, 2048)
ONE, NEG_ONE = lr.ONE, lr.NEG_ONE
E_ARG, E_STATE = -1, -3
S_ = 12 * L_


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


_case = {}


def slots_case():
    """the statement of shapes_case with constraints added so that one slot carries exactly HEAVY_MIN terms and another HEAVY_MIN + 1 (both
    over several constraints, one of them repeating a term) -> (system, the asked slots by name); it holds on the base trace but for rhs_only"""
    if not _case:
        kinds, rows = base_trace()
        base, at = shapes_case()
        rhs = dict(zip(base.rhs_constraint, base.rhs_coef))
        b = Builder(rows)
        for c in range(base.n_constraints):                       # replayed as it stands (rhs_only keeps its right-hand side)
            seg = range(base.term_begin[c], base.term_begin[c + 1])
            b.add([(base.slots[t], base.coef_idx[t]) for t in seg], b=base.coef(rhs[c]) if c in rhs else 0)
        used = collections.Counter(base.slots)
        free = [s for s in range(2 * L_, 5 * L_) if s not in used]               # linear rows
        exact, over, none = free[0], free[1], free[2]
        picks = [ONE, NEG_ONE, 3, 4, 5, 7]
        rng = np.random.default_rng(77)
        for slot, count in ((exact, HEAVY_MIN), (over, HEAVY_MIN + 1)):
            left = count
            for n in (1000, 700, left - 1700):                    # three constraints, each with a neighbour slot in the middle
                b.add([(slot, picks[int(ci)]) for ci in rng.integers(0, 6, n // 2)] + [(slot + 40, 2)] +
                      [(slot, picks[int(ci)]) for ci in rng.integers(0, 6, n - n // 2)])
        system = b.system()
        count = collections.Counter(system.slots)
        assert count[exact] == HEAVY_MIN and count[over] == HEAVY_MIN + 1 and count[none] == 0
        hot = 10 * L_ + 5
        assert count[hot] == HEAVY_MIN + 3 and count[700] == 4 and count[5] == 2 and count[0] == 1 and count[S_ - 1] == 2      # (hot and the last slot: in "heavy" too)
        one = next(s for s in range(S_) if count[s] == 1 and s not in (0, S_ - 1))
        on_q = [next(s for s in range(r * L_, (r + 1) * L_) if count[s] >= 1) for r in (5, 6, 7)]      # a QX, a QY and a QZ row
        assert [int(kinds[r]) for r in (5, 6, 7, 10)] == [1, 2, 3, 2]
        names = dict(none=none, one=one, thrice=700, twice=5, first=0, last=S_ - 1, exact=exact, over=over, hot=hot, qx=on_q[0], qy=on_q[1], qz=on_q[2])
        assert len(set(names.values())) == len(names)
        _case.update(system=system, names=names)
    return _case["system"], _case["names"]


def check(amd, c, tr, system, kinds, rows, asked, term_cap=1 << 15):
    """explain_slots_attached on `tr` against (a) rows_explain_slots with `system` -- the statement in force, its coefs = the table in
    force -- and (b) the reference over `rows` -> (info, slot records, term records) of the attached call"""
    asked = [int(a) for a in asked]
    total, rep, distinct, want_s, want_t = sr.explain_slots(system, kinds, rows, L_, asked, term_cap)
    info, rec, terms = c.rows_explain_slots_attached(tr, asked, term_cap=term_cap)
    info0, rec0, terms0 = c.rows_explain_slots(tr, system.to_binding(amd), asked, term_cap=term_cap)
    print("explain_slots_attached: %d asked, %d terms, %d reported, %d constraints, %.3f ms (with the term list: %.3f ms)" %
          (len(asked), info.n_terms_total, info.n_terms_reported, info.n_constraints_distinct, info.ms_total, info0.ms_total))
    assert (info.n_terms_total, info.n_terms_reported, info.n_constraints_distinct) == (total, rep, distinct)
    assert (info0.n_terms_total, info0.n_terms_reported, info0.n_constraints_distinct) == (total, rep, distinct)
    assert len(rec) == len(rec0) == len(asked) and len(terms) == len(terms0) == rep
    assert rec.tobytes() == rec0.tobytes() and terms.tobytes() == terms0.tobytes()
    assert sr.got_slots(rec) == want_s
    assert sr.got_terms(terms) == want_t
    return info, rec, terms


def check_untouched(amd, c, tr, system, kinds, rows, nonzero_only, cap):
    n, nz, rep, want = sr.untouched(system, kinds, rows, L_, nonzero_only, cap)
    info, out = c.rows_untouched_slots_attached(tr, nonzero_only=nonzero_only, cap=cap)
    info0, out0 = c.rows_untouched_slots(tr, system.to_binding(amd), nonzero_only=nonzero_only, cap=cap)
    print("untouched_slots_attached: %d untouched, %d nonzero, %d reported, %.3f ms (with the term list: %.3f ms)" %
          (info.n_untouched, info.n_untouched_nonzero, info.n_reported, info.ms_total, info0.ms_total))
    assert (info.n_untouched, info.n_untouched_nonzero, info.n_reported) == (n, nz, rep)
    assert (info0.n_untouched, info0.n_untouched_nonzero, info0.n_reported) == (n, nz, rep)
    assert len(out) == len(out0) == rep and out.tobytes() == out0.tobytes()
    assert sr.got_values(out) == want
    return info, out


# ---------------------------------------------------------------- 1: slot shapes and asked lists
def test_slot_shapes_and_asked_lists(amd):
    kinds, rows = base_trace()
    system, nm = slots_case()
    c = amd.Context(*SHAPE)
    try:
        tr, keep = begun(amd, c, kinds, rows)
        c.rows_set_linear(tr, system.to_binding(amd))
        c.rows_commit(tr)
        shapes = sorted(nm.values())
        _, rec, terms = check(amd, c, tr, system, kinds, rows, shapes)
        by = {int(r["slot"]): r for r in rec}
        assert [int(by[nm[k]]["n_terms"]) for k in ("none", "one", "thrice", "twice", "exact", "over", "hot")] == [0, 1, 4, 2, HEAVY_MIN, HEAVY_MIN + 1, HEAVY_MIN + 3]
        assert [int(by[nm[k]]["row_kind"]) for k in ("first", "qx", "qy", "qz", "hot", "last")] == [0, 1, 2, 3, 2, 3]
        seg = terms[int(by[700]["first_term"]):][:4]                                      # one constraint: index 4 twice, 7, then the special
        assert len({int(t["constraint"]) for t in seg}) == 1 and [int(t["coef_index"]) for t in seg] == [4, 4, 7, NEG_ONE]
        assert seg[0].tobytes() == seg[1].tobytes() and {int(t["constraint_terms"]) for t in seg} == {5}
        seg = terms[int(by[5]["first_term"]):][:2]                                        # one constraint twice, two coefficients
        assert int(seg[0]["constraint"]) == int(seg[1]["constraint"]) and [int(t["coef_index"]) for t in seg] == [3, 5]
        assert bytes(seg[0]["coef"]) == er.le32(system.coefs[3]) != bytes(seg[1]["coef"])
        check(amd, c, tr, system, kinds, rows, [nm["one"]])                               # one slot
        check(amd, c, tr, system, kinds, rows, [nm["none"]])                              # one slot without a term: no record at all
        check(amd, c, tr, system, kinds, rows, [nm["over"]])                              # a heavy slot alone
        info, rec, _ = check(amd, c, tr, system, kinds, rows, range(S_))                  # every slot of the trace
        assert info.n_terms_total == len(system.slots) and int(rec["n_terms"].sum()) == len(system.slots)
        for call in (lambda: c.rows_explain_slots_attached(tr, []), lambda: c.rows_explain_slots(tr, system.to_binding(amd), [])):
            info, rec, terms = call()                                                     # nothing asked: nothing returned
            assert (info.n_terms_total, info.n_terms_reported, info.n_constraints_distinct, len(rec), len(terms)) == (0, 0, 0, 0, 0)
        c.trace_destroy(tr)
    finally:
        c.close()


# ---------------------------------------------------------------- 2: term_cap
def test_term_cap(amd):
    kinds, rows = base_trace()
    system, nm = slots_case()
    shapes = sorted(nm.values())
    c = amd.Context(*SHAPE)
    try:
        tr, keep = begun(amd, c, kinds, rows)
        with c.linear_prepare(system.to_binding(amd), kinds) as prog:
            c.rows_attach_linear(tr, prog)
        c.rows_commit(tr)
        full = check(amd, c, tr, system, kinds, rows, shapes, term_cap=1 << 15)
        total = full[0].n_terms_total
        first = {int(r["slot"]): int(r["first_term"]) for r in full[1]}
        assert total == sum(int(r["n_terms"]) for r in full[1]) and total < 1 << 15
        for cap in (0, 1, first[nm["exact"]] + 1000, first[nm["hot"]] + HEAVY_MIN + 1, total - 1, total, total + 5):      # inside two heavy segments
            info, rec, terms = check(amd, c, tr, system, kinds, rows, shapes, term_cap=cap)                                 # cap = 0: NULL term array
            assert (info.n_terms_total, info.n_terms_reported) == (total, min(cap, total))
            assert rec.tobytes() == full[1].tobytes()                                     # slot_out complete whatever the cap
            assert terms.tobytes() == full[2][:cap].tobytes()
        at = 0
        for r in full[1]:                                                                 # first_term / n_terms tile the full order
            assert int(r["first_term"]) == at and (full[2][at:at + int(r["n_terms"])]["slot"] == r["slot"]).all()
            at += int(r["n_terms"])
        assert at == total
        c.trace_destroy(tr)
    finally:
        c.close()


# ---------------------------------------------------------------- 3: a bumped witness
def test_bumped_slot_residuals_are_the_explain_records(amd):
    kinds, truth = base_trace()
    system, nm = slots_case()
    rows = truth.copy()
    bump(rows, 700, 5)
    bump(rows, nm["over"], 3)
    neighbour = nm["none"]                                        # untouched by the statement: bumping it changes no residual
    bump(rows, neighbour, 9)
    count = collections.Counter(system.slots)
    quiet = next(s for s in range(701, 3 * L_) if count[s] >= 1)  # a slot next to 700 whose constraints all still hold
    NC = system.n_constraints
    c = amd.Context(*SHAPE)
    try:
        tr, keep = begun(amd, c, kinds, rows)
        c.rows_set_linear(tr, system.to_binding(amd))
        c.rows_commit(tr)
        _, con, _ = c.rows_explain_attached(tr, list(range(NC)), term_cap=0)
        shown = {int(r["constraint"]): (int(r["n_terms"]), bytes(r["residual"])) for r in con}
        _, rec, terms = check(amd, c, tr, system, kinds, rows, sorted({700, nm["over"], neighbour, quiet, nm["hot"], 9}))
        for t in terms:                                                                   # what lig_rows_explain_attached says of that constraint
            assert (int(t["constraint_terms"]), bytes(t["residual"])) == shown[int(t["constraint"])]
        through = lambda s: [t for t in terms if int(t["slot"]) == s]
        assert through(700) and all(t["residual"].any() for t in through(700)) and all(t["residual"].any() for t in through(nm["over"]))
        assert len({bytes(t["residual"]) for t in through(nm["over"])}) == 3              # three constraints, three residuals
        assert through(quiet) and not any(t["residual"].any() for t in through(quiet)) and not through(neighbour)
        assert [t["residual"].any() for t in through(9)] == [True]                        # slot 9 shares the violated constraint of slot 700
        by = {int(r["slot"]): r for r in rec}
        assert bytes(by[700]["value"]) == er.le32(wit(rows, 700)) != er.le32(wit(truth, 700))
        assert bytes(by[neighbour]["value"]) == er.le32(wit(rows, neighbour)) and int(by[neighbour]["n_terms"]) == 0
        c.trace_destroy(tr)
    finally:
        c.close()


# ---------------------------------------------------------------- 4: values in force
def test_values_in_force(amd):
    kinds, rows = base_trace()
    system, nm = slots_case()
    asked = sorted({700, 5, 17, S_ - 1, 3, 400, nm["hot"]})
    T = list(system.coefs)
    T2, T3 = list(T), list(T)
    pm_one = next(c for c in range(system.n_constraints) if system.slots[system.term_begin[c]:system.term_begin[c + 1]] == [17, S_ - 1, 400, 3])
    rhs_entry = system.rhs_coef[system.rhs_constraint.index(pm_one)]
    T2[rhs_entry] = (T2[rhs_entry] + 1) % P                       # one right-hand side ...
    T2[4] = (T2[4] + 6) % P                                       # ... and one term coefficient (index 4: slot 700 among others)
    T3[7] = 11
    c, cb = amd.Context(*SHAPE), amd.Context(*SHAPE)
    try:
        with c.linear_prepare(system.to_binding(amd), kinds) as prog:
            (ta, keep_a), (tb, keep_b) = begun(amd, c, kinds, rows), begun(amd, cb, kinds, rows)
            c.rows_attach_linear(ta, prog)
            cb.rows_attach_linear(tb, prog)
            c.rows_commit(ta)
            cb.rows_commit(tb)
            plain = check(amd, c, ta, system, kinds, rows, asked)
            c.rows_set_linear_values(ta, T2)                      # the conversion is queued on the side stream: the call orders itself after it
            _, rec, terms = check(amd, c, ta, with_table(system, T2), kinds, rows, asked)
            assert {bytes(t["coef"]) for t in terms if int(t["coef_index"]) == 4} == {er.le32(T2[4])}
            assert {bytes(t["residual"]) for t in terms if int(t["constraint"]) == pm_one} == {er.le32(P - 1)}
            assert all(t["residual"].any() for t in terms if int(t["slot"]) == 700)      # its constraint uses index 4
            cb.rows_set_linear_values(tb, T3)                     # two traces on one program, each with its own values
            _, rec_b, terms_b = check(amd, cb, tb, with_table(system, T3), kinds, rows, asked)
            assert {bytes(t["coef"]) for t in terms_b if int(t["coef_index"]) == 7} == {er.le32(11)}
            assert {bytes(t["coef"]) for t in terms_b if int(t["coef_index"]) == 4} == {er.le32(T[4])}
            assert check(amd, c, ta, with_table(system, T2), kinds, rows, asked)[2].tobytes() == terms.tobytes()
            c.rows_set_linear_values(ta, None)                    # the program's own table again
            back = check(amd, c, ta, system, kinds, rows, asked)
            assert back[1].tobytes() == plain[1].tobytes() and back[2].tobytes() == plain[2].tobytes()
            c.trace_destroy(ta)
            cb.trace_destroy(tb)
    finally:
        cb.close()
        c.close()


# ---------------------------------------------------------------- 5: released term list, two prepares, two calls
def test_released_term_list_and_two_prepares(amd):
    kinds, truth = base_trace()
    system, nm = slots_case()
    rows = truth.copy()
    bump(rows, nm["hot"], 2)
    asked = sorted(nm.values())
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
            first = c.rows_explain_slots_attached(tr, asked, term_cap=1 << 15)
            total, rep, distinct, want_s, want_t = sr.explain_slots(system, kinds, rows, L_, asked, 1 << 15)      # the reference alone first
            assert sr.got_slots(first[1]) == want_s and sr.got_terms(first[2]) == want_t
            check(amd, c, tr, system, kinds, rows, asked)
            un = c.rows_untouched_slots_attached(tr, cap=S_)
            got.append((first[1].tobytes(), first[2].tobytes(), un[1].tobytes(), un[0].n_untouched, un[0].n_untouched_nonzero))
            c.trace_destroy(tr)
        assert got[0] == got[1]                                                           # whichever prepare made the program
    finally:
        c.close()


# ---------------------------------------------------------------- 6: derived product row, mixed operand rows
def test_derived_and_mixed_rows(amd):
    """the inputs of tests/test_gpu_explain.py::test_derived_and_mixed_rows"""
    kinds, truth = base_trace()
    rows = truth.copy()
    rng = np.random.default_rng(41)
    QX = [r for r in range(12) if int(kinds[r]) == 1]
    x0, lin0 = QX[0], [r for r in range(12) if int(kinds[r]) == 0][0]
    xs = [int(v) for v in rng.integers(0, 2, L_)]
    ys = [int(v) for v in rng.integers(0, 256, L_)]
    ls = [int(v) for v in rng.integers(0, 1 << 16, L_)]
    xs[4], xs[100], xs[L_ - 1] = P - 1, (1 << 200) + 3, 1 << 64
    ys[4], ys[7] = P - 1, (1 << 253) + 1
    ls[0], ls[150], ls[L_ - 1] = P - 2, 1 << 16, (1 << 130) + 5
    zs = [a * b % P for a, b in zip(xs, ys)]
    for r, v in ((x0, xs), (x0 + 1, ys), (x0 + 2, zs), (lin0, ls)):
        rows[r, :L_] = ol.to_limbs(v)
    widths, wide = amd.mixed_widths(rows, kinds, L_, derive_products=True)
    assert (int(widths[x0]), int(wide[x0])) == (amd.ELEM_BIT, 3) and [int(widths[r + 2]) for r in QX] == [amd.ELEM_PRODUCT] * 2
    k2, msgs = shipped(amd, kinds, rows)
    msgs[[r + 2 for r in QX]] = 0xDEADBEEF                                                # nothing of the expected products reaches the library
    packed = amd.pack_rows_mixed(msgs, widths, wide, L_)
    z0, z1 = (x0 + 2) * L_, (QX[1] + 2) * L_
    b = Builder(rows)
    b.add([(z0 + 4, ONE), (z0 + 100, 4), (z1 + 9, NEG_ONE), (x0 * L_ + 4, 3)])
    b.add([(lin0 * L_ + 150, 7), (lin0 * L_ + L_ - 1, ONE), ((x0 + 1) * L_ + 7, 5), (lin0 * L_ + 1, ONE)])
    system = b.system()
    c = amd.Context(*SHAPE)
    try:
        tr, keep = c.rows_begin(k2, packed, generated_at=lr.GEN, elem_bytes=widths, wide_per_row=wide)
        c.rows_set_linear(tr, system.to_binding(amd))
        c.rows_commit(tr)
        asked = sorted({z0 + 4, z0 + 100, z0 + 5, z1 + 9, z1, x0 * L_ + 4, x0 * L_ + 100, x0 * L_ + 5, (x0 + 1) * L_ + 7, lin0 * L_, lin0 * L_ + 1,
                        lin0 * L_ + 150, lin0 * L_ + L_ - 1})
        _, rec, terms = check(amd, c, tr, system, kinds, rows, asked)
        shown = {int(r["slot"]): int.from_bytes(bytes(r["value"]), "little") for r in rec}
        assert shown[z0 + 4] == zs[4] == 1 and shown[z0 + 100] == zs[100] == ((1 << 200) + 3) * ys[100] % P and shown[z0 + 5] == zs[5]      # the products
        assert shown[z1 + 9] == wit(truth, QX[1] * L_ + 9) * wit(truth, (QX[1] + 1) * L_ + 9) % P
        assert shown[lin0 * L_ + 150] == 1 << 16 and shown[(x0 + 1) * L_ + 7] == (1 << 253) + 1 and shown[x0 * L_ + 100] == (1 << 200) + 3   # records
        assert shown[x0 * L_ + 5] == xs[5] and shown[lin0 * L_ + 1] == ls[1]                                                                  # narrow slots
        assert not terms["residual"].any() and (rec["value"].view("<u4").reshape(-1, 8) == c.rows_read_slots(tr, asked)).all()
        check_untouched(amd, c, tr, system, kinds, rows, True, S_)                        # bits and bytes: many zero values drop out
        c.trace_destroy(tr)
    finally:
        c.close()


# ---------------------------------------------------------------- 7: untouched slots
def test_untouched_slots(amd):
    kinds, truth = base_trace()
    system, nm = slots_case()
    rows = truth.copy()
    rows[1, 200:L_] = 0                                           # a short linear row: its zero fill
    rows[6, 300:L_] = 0                                           # ... and a short QY row
    rows[0, 0] = 0                                                # (touched: not listed either way)
    sparse = Builder(rows)
    sparse.add([(5, ONE), (7 * L_ + 9, 3), (5, 2)])               # rows 0 and 7 only: every other row is touched nowhere
    sparse.add([(L_ - 1, NEG_ONE)])
    sparse = sparse.system()
    empty = lr.System([0], [], [], [], [], [], 0)
    c = amd.Context(*SHAPE)
    try:
        tr, keep = begun(amd, c, kinds, rows)
        c.rows_set_linear(tr, system.to_binding(amd))
        c.rows_commit(tr)
        n, nz, _, every = sr.untouched(system, kinds, rows, L_, False, S_)
        zero_fill = [s for s, _, v in every if v == bytes(32)]
        assert 0 < nz < n < S_ and set(zero_fill) <= set(range(L_ + 200, 2 * L_)) | set(range(6 * L_ + 300, 7 * L_)) and len(zero_fill) > 30
        for nonzero_only in (False, True):
            for cap in (0, 97, S_):                               # counts only; below the count; above it
                info, out = check_untouched(amd, c, tr, system, kinds, rows, nonzero_only, cap)
                assert (info.n_untouched, info.n_untouched_nonzero) == (n, nz) and info.n_reported == min(cap, nz if nonzero_only else n)
        _, out = check_untouched(amd, c, tr, system, kinds, rows, True, S_)
        assert not set(int(s) for s in out["slot"]) & set(zero_fill) and out["value"].any(axis=1).all()
        _, out = check_untouched(amd, c, tr, system, kinds, rows, False, S_)
        assert set(zero_fill) <= set(int(s) for s in out["slot"]) and nm["none"] in out["slot"] and 700 not in out["slot"]
        c.rows_set_linear(tr, sparse.to_binding(amd))             # rows the system touches nowhere: every slot of them
        info, out = check_untouched(amd, c, tr, sparse, kinds, rows, False, S_)
        assert info.n_untouched == S_ - 3 and [int(s) for s in out["slot"]] == [s for s in range(S_) if s not in (5, L_ - 1, 7 * L_ + 9)]
        assert [int(kd) for kd in out["row_kind"]] == [int(kinds[int(s) // L_]) for s in out["slot"]] and set(out["row_kind"]) == {0, 1, 2, 3}
        c.rows_set_linear(tr, empty.to_binding(amd))              # the empty system: every LINEAR .. QZ slot
        info, out = check_untouched(amd, c, tr, empty, kinds, rows, False, S_)
        assert info.n_untouched == S_ and (out["slot"] == np.arange(S_)).all()
        assert (out["value"].view("<u4").reshape(-1, 8) == er.slot_values(rows, L_, range(S_))).all()
        c.trace_destroy(tr)
    finally:
        c.close()


# ---------------------------------------------------------------- 8: nothing is disturbed
def test_envelope_is_untouched(amd):
    kinds, truth = base_trace()
    system, nm = slots_case()
    rows = truth.copy()
    bump(rows, 700, 1)
    tab = list(system.coefs)
    tab[7] = 13
    in_force = with_table(system, tab)
    asked = sorted(nm.values())
    c = amd.Context(*SHAPE)
    try:
        with c.linear_prepare(system.to_binding(amd), kinds) as prog:
            def all_four(tr):
                check(amd, c, tr, in_force, kinds, rows, asked, term_cap=5000)            # (both explain_slots entries ...)
                check_untouched(amd, c, tr, in_force, kinds, rows, True, 50)              # (... and both untouched_slots entries)

            def envelope(when):
                tr, keep = begun(amd, c, kinds, rows)
                c.rows_attach_linear(tr, prog)
                c.rows_set_linear_values(tr, tab)
                c.rows_commit(tr)
                if when == "after commit":
                    all_four(tr)
                proof, info = c.rows_prove(tr, None, None)
                if when == "after prove":
                    all_four(tr)
                c.trace_destroy(tr)
                return proof, bytes(info.const_sum), bytes(info.stage2_seed), (info.valid_code, info.valid_linear, info.valid_quad)

            plain = envelope("never")
            assert plain[3] == (1, 0, 1)
            assert envelope("after commit") == plain and envelope("after prove") == plain
    finally:
        c.close()


# ---------------------------------------------------------------- 9: window, state and arguments on a real trace
def test_window_state_and_argument_errors(amd):
    kinds, truth = base_trace()
    system, nm = slots_case()
    c = amd.Context(*SHAPE)
    try:
        sysb = system.to_binding(amd)
        rec, terms, vals = np.zeros(8, dtype=amd.SLOT_RECORD), np.zeros(16, dtype=amd.SLOT_TERM), np.zeros(16, dtype=amd.SLOT_VALUE)
        p = lambda a: a.ctypes.data_as(C.c_void_p)

        def sinfo(short=0):
            i = amd.SlotInfo()
            i.struct_bytes = C.sizeof(amd.SlotInfo) - short
            return i

        def uinfo(short=0):
            i = amd.UntouchedInfo()
            i.struct_bytes = C.sizeof(amd.UntouchedInfo) - short
            return i

        def rc_att(t, asked):
            a = np.asarray(asked, dtype=np.uint32)
            return c.L.lig_rows_explain_slots_attached(t, p(a), len(a), p(rec), p(terms), len(terms), C.byref(sinfo()))

        def rc_list(t, asked, sys=sysb):
            a = np.asarray(asked, dtype=np.uint32)
            return c.L.lig_rows_explain_slots(t, C.byref(sys) if sys is not None else None, p(a), len(a), p(rec), p(terms), len(terms), C.byref(sinfo()))

        def rc_un_att(t):
            return c.L.lig_rows_untouched_slots_attached(t, 0, p(vals), len(vals), C.byref(uinfo()))

        def rc_un_list(t, sys=sysb):
            return c.L.lig_rows_untouched_slots(t, C.byref(sys) if sys is not None else None, 1, p(vals), len(vals), C.byref(uinfo()))

        def all_rc(t):
            return (rc_att(t, [0]), rc_list(t, [0]), rc_un_att(t), rc_un_list(t))

        def good(t):
            check(amd, c, t, system, kinds, truth, [0, 700, S_ - 1])
            check_untouched(amd, c, t, system, kinds, truth, False, 16)

        def proves(t):
            _, i = c.rows_prove(t, None, None)
            return (i.valid_code, i.valid_linear, i.valid_quad)

        k2, m0 = shipped(amd, kinds, truth)
        tr, keep = c.rows_begin(k2, m0, generated_at=lr.GEN)
        c.rows_set_linear(tr, sysb)
        assert all_rc(tr) == (E_STATE,) * 4                                               # before the first commit
        c.rows_commit(tr)
        # argument errors: decided on the host, nothing launched; the trace still answers after each
        for asked in ([1, 0], [2, 2], [0, S_], [S_], [0, 5, 4], [0xFFFFFFFF]):            # unsorted, repeated, out of range
            assert rc_att(tr, asked) == E_ARG and rc_list(tr, asked) == E_ARG
            good(tr)
        assert rc_list(tr, [0], sys=None) == E_ARG and rc_un_list(tr, sys=None) == E_ARG  # the term-list entries without a term list
        a = np.zeros(1, dtype=np.uint32)
        att = c.L.lig_rows_explain_slots_attached
        assert att(tr, p(a), 1, None, p(terms), 16, C.byref(sinfo())) == E_ARG
        assert att(tr, None, 1, p(rec), p(terms), 16, C.byref(sinfo())) == E_ARG
        assert att(tr, p(a), 1, p(rec), None, 16, C.byref(sinfo())) == E_ARG
        assert att(tr, p(a), 1, p(rec), None, 0, C.byref(sinfo())) == 0                   # counts and slot_out only
        assert att(tr, p(a), 1, p(rec), p(terms), 16, None) == E_ARG
        assert att(tr, p(a), 1, p(rec), p(terms), 16, C.byref(sinfo(short=8))) == E_ARG
        assert att(tr, None, 0, None, None, 0, C.byref(sinfo())) == 0                     # nothing asked: LIG_OK
        un = c.L.lig_rows_untouched_slots_attached
        assert un(tr, 0, None, 16, C.byref(uinfo())) == E_ARG and un(tr, 0, None, 0, C.byref(uinfo())) == 0
        assert un(tr, 0, p(vals), 16, None) == E_ARG and un(tr, 0, p(vals), 16, C.byref(uinfo(short=8))) == E_ARG
        good(tr)
        bad_sys = system.to_binding(amd, slots=[S_] + system.slots[1:])                   # a slot out of range: lig_linear_check rejects it
        assert rc_list(tr, [0], sys=bad_sys) == E_ARG and rc_list(tr, [], sys=bad_sys) == E_ARG and rc_un_list(tr, sys=bad_sys) == E_ARG
        good(tr)
        assert proves(tr) == (1, 0, 1)                                                    # (rhs_only is violated by construction)
        good(tr)                                                                          # the proof does not end the window
        c.rows_restart(tr, m0)                                                            # after prove: straight into the matrix
        assert all_rc(tr) == (E_STATE,) * 4
        c.rows_commit(tr)
        good(tr)
        assert proves(tr) == (1, 0, 1)
        c.trace_destroy(tr)
        # nothing attached: only the attached entries mind
        tr, keep = c.rows_begin(k2, m0, generated_at=lr.GEN)
        c.rows_commit(tr)
        assert all_rc(tr) == (E_STATE, 0, E_STATE, 0)
        c.rows_set_linear(tr, sysb)
        good(tr)
        c.rows_set_linear(tr, None)                                                       # detached again
        assert (rc_att(tr, [0]), rc_un_att(tr)) == (E_STATE, E_STATE)
        c.rows_set_linear(tr, sysb)
        assert proves(tr) == (1, 0, 1)
        c.trace_destroy(tr)
        tr = c.synth_prepare(700, 330)
        assert all_rc(tr) == (E_STATE,) * 4
        c.trace_destroy(tr)
    finally:
        c.close()
