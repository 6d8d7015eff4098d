"""GPU: lig_rows_diagnose -- the violated constraints of a committed rows job, named on the device (csrc/diagnose.hip).

Expected values never come from the library: tests/diagnose_ref.py restates both residuals in Python integers over the rows the test
ships (derived rows: x * y mod p in Python).  Every comparison is bit-exact: constraint numbers, rows, columns, residual bytes, order
and counts.  No test hands a kernel an invalid index; the misuse cases check return codes of calls that launch nothing."""
import ctypes as C

import numpy as np
import pytest

import batch_prog
import diagnose_ref as dr
import hip_lib
import linear_ref as lr
import oracle_lib as ol

pytestmark = pytest.mark.gpu

P = ol.P
SMALL, BIG = (320, 512, 2048), (8000, 8192, 32768)
ONE, NEG_ONE = lr.ONE, lr.NEG_ONE
LINEAR, QX, QY, QZ, BIT, EQX, EQY = 0, 1, 2, 3, 5, 6, 7


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def shipped(amd, kinds, rows, l):
    """(kinds | DRAW_PAD, rows with garbage in the pad slots the library draws)"""
    kinds, msgs = np.asarray(kinds, dtype=np.uint8).copy(), rows.copy()
    draws = (kinds <= 3) | (kinds == amd.ROW_KINDS["INIT"])
    msgs[draws, l:] = 0xDEADBEEF
    kinds[draws] |= amd.ROW_DRAW_PAD
    return kinds, msgs


def check(amd, c, tr, system, kinds, rows, lin_cap=1024, quad_cap=1024):
    """diagnose the committed trace and compare everything with the reference over `rows` -> (linear, quadratic) reference violations"""
    l = c.l
    want_l = dr.linear_violations(system, rows, l) if system is not None else []
    want_q = dr.quad_violations(kinds, rows, l)
    info, lin, quad = c.rows_diagnose(tr, system.to_binding(amd) if system is not None else None, lin_cap=lin_cap, quad_cap=quad_cap)
    print("linear: %d violated, %d reported; quadratic: %d violated, %d reported; %.3f ms" %
          (info.n_linear_bad, info.n_linear_reported, info.n_quad_bad, info.n_quad_reported, info.ms_total))
    assert (info.n_linear_bad, info.n_quad_bad) == (len(want_l), len(want_q))
    assert (info.n_linear_reported, info.n_quad_reported) == (min(lin_cap, len(want_l)), min(quad_cap, len(want_q)))
    assert dr.got_linear(lin) == dr.linear_records(want_l[:lin_cap])
    assert dr.got_quad(quad) == dr.quad_records(want_q[:quad_cap])
    return want_l, want_q


def committed(amd, c, kinds, rows, **kw):
    k2, msgs = shipped(amd, kinds, rows, c.l)
    tr, keep = c.rows_begin(k2, msgs, generated_at=lr.GEN, **kw)
    c.rows_commit(tr)
    return tr


def field_rows(kinds, l, k, seed):
    """rows of a trace made here: canonical field elements in the data slots, z = x * y for every triple, zeros in the pads"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((len(kinds), k, 8), dtype=np.uint32)
    for r, kd in enumerate(kinds):
        if kd in (LINEAR, QX, QY):
            rows[r, :l] = ol.rand_field(rng, l)
        elif kd == QZ:
            xs, ys = ol.from_limbs(rows[r - 2, :l]), ol.from_limbs(rows[r - 1, :l])
            rows[r, :l] = ol.to_limbs([x * y % P for x, y in zip(xs, ys)])
    return rows


def wit(rows, l, s):
    return ol.from_limbs(rows[s // l, s % l])[0]


def set_wit(rows, l, s, v):
    rows[s // l, s % l] = ol.to_limbs([v % P])[0]


class Builder:
    """a linear_ref.System constraint by constraint; b_c is computed from the witness unless given"""

    def __init__(self, rows, l):
        self.rows, self.l = rows, l
        self.term_begin, self.slots, self.cidx, self.rhs_c, self.rhs_b, self.coefs = [0], [], [], [], [], []

    def coef(self, v):
        if v not in self.coefs:
            self.coefs.append(v)
        return self.coefs.index(v)

    def value(self, ci):
        return 1 if ci == ONE else P - 1 if ci == NEG_ONE else self.coefs[ci]

    def add(self, terms, b=None, off=0):
        """terms: [(slot, coefficient index)]; b = None: the value that makes the constraint hold, plus `off`; -> constraint number"""
        for s, ci in terms:
            self.slots.append(s)
            self.cidx.append(ci)
        self.term_begin.append(len(self.slots))
        if b is None:
            b = (sum(self.value(ci) * wit(self.rows, self.l, s) for s, ci in terms) + off) % P
        c = len(self.term_begin) - 2
        if b:
            self.rhs_c.append(c)
            self.rhs_b.append(self.coef(b))
        return c

    def system(self):
        return lr.System(self.term_begin, self.slots, self.cidx, self.rhs_c, self.rhs_b, self.coefs, 0)


_small = {}


def small_case():
    """12 rows at (320, 512, 2048): 6 linear rows, 2 triples, a seeded system and the equality system, both true"""
    if not _small:
        l, k, n = SMALL
        kinds, rows, _ = lr.build_trace(l, k, n, 5 * l + 17, l + 9)
        assert len(kinds) == 12
        _small.update(kinds=kinds, rows=rows, system=lr.make_system(kinds, rows, l, 3000, 0, seed=11, hot_terms=60),
                      eq=lr.make_equality_system(kinds, l, 0))
        assert lr.holds(_small["system"], rows, l) and lr.holds(_small["eq"], rows, l)
    return _small


@pytest.mark.parametrize("which", ["system", "eq"])
def test_satisfied_trace_has_no_violation_and_proves(amd, which):
    cz = small_case()
    c = amd.Context(*SMALL)
    try:
        tr = committed(amd, c, cz["kinds"], cz["rows"])
        assert check(amd, c, tr, cz[which], cz["kinds"], cz["rows"]) == ([], [])
        c.rows_set_linear(tr, cz[which].to_binding(amd))
        _, info = c.rows_prove(tr, None, None)
        assert (info.valid_code, info.valid_linear, info.valid_quad) == (1, 1, 1)
        c.trace_destroy(tr)
    finally:
        c.close()


def test_corrupted_slots_are_named_exactly(amd):
    cz = small_case()
    l, system = SMALL[0], cz["system"]
    rows = cz["rows"].copy()
    rng = np.random.default_rng(2)
    used = sorted(set(system.slots) - {system.hot_slot})
    victims = [system.single_slot] + [int(s) for s in rng.choice(used, size=9, replace=False)]
    for s in victims:
        set_wit(rows, l, s, wit(rows, l, s) + 1 + s)
    assert not lr.holds(system, rows, l)
    c = amd.Context(*SMALL)
    try:
        tr = committed(amd, c, cz["kinds"], rows)
        want_l, _ = check(amd, c, tr, system, cz["kinds"], rows)
        assert 10 <= len(want_l) and want_l[0][0] == 0
        check(amd, c, tr, system, cz["kinds"], rows, lin_cap=3, quad_cap=2)            # the first three; the counts are unchanged
        check(amd, c, tr, system, cz["kinds"], rows, lin_cap=0, quad_cap=0)            # counts only
        c.rows_set_linear(tr, system.to_binding(amd))
        _, info = c.rows_prove(tr, None, None)
        assert info.valid_linear == 0
        check(amd, c, tr, system, cz["kinds"], rows)                                   # after the proof: the matrix is still the committed one
        c.trace_destroy(tr)
    finally:
        c.close()


def test_coefficients_and_shapes(amd):
    l, k, n = SMALL
    kinds = [LINEAR] * 12
    rows = field_rows(kinds, l, k, seed=7)
    set_wit(rows, l, 5, P - 1)                                # a witness slot holding p - 1
    set_wit(rows, l, 6, 0)
    b = Builder(rows, l)
    big = (1 << 253) + 12345
    assert big < P
    tab = [b.coef(v) for v in (0, 1, P - 1, big, P - 2, 7)]
    every = [(5, ci) for ci in tab + [ONE, NEG_ONE]] + [(321 + i, ci) for i, ci in enumerate(tab + [ONE, NEG_ONE])]
    ok_all = b.add(every)                                     # every kind of coefficient, on p - 1 and on random witnesses: holds
    bad_all = b.add(every, off=5)                             # the same terms, b off by 5: residual p - 5
    rep_ok = b.add([(700, tab[3]), (700, NEG_ONE), (700, tab[5]), (6, ONE)])         # a slot repeated inside one constraint
    rep_bad = b.add([(700, tab[3]), (700, NEG_ONE), (700, tab[5])], off=P - 1)
    empty_bad = b.add([], b=big)                              # no term, b != 0: violated, residual p - b
    empty_ok = b.add([])                                      # no term, no right-hand side: holds
    zero_coef = b.add([(900, tab[0])], b=0)                   # 0 * w = 0
    neg = b.add([(5, ONE)], b=P - 1)                          # w = p - 1 against the table entry p - 1
    neg_bad = b.add([(5, NEG_ONE)], b=P - 1)                  # -(p - 1) = 1, b = p - 1: residual 2
    system = b.system()
    c = amd.Context(l, k, n)
    try:
        tr = committed(amd, c, kinds, rows)
        want_l, _ = check(amd, c, tr, system, kinds, rows)
        assert want_l == [(bad_all, P - 5), (rep_bad, 1), (empty_bad, P - big), (neg_bad, 2)]
        assert {ok_all, rep_ok, empty_ok, zero_coef, neg}.isdisjoint(cn for cn, _ in want_l)
        # argument errors on a real trace, decided before anything is launched: a short struct_bytes, a NULL array with a nonzero cap
        sysb = system.to_binding(amd)
        short = diag_info(amd)
        short.struct_bytes -= 8
        assert c.L.lig_rows_diagnose(tr, C.byref(sysb), None, 0, None, 0, C.byref(short)) == -1
        assert c.L.lig_rows_diagnose(tr, C.byref(sysb), None, 5, None, 0, C.byref(diag_info(amd))) == -1
        assert c.L.lig_rows_diagnose(tr, C.byref(sysb), None, 0, None, 5, C.byref(diag_info(amd))) == -1
        assert c.L.lig_rows_diagnose(tr, C.byref(sysb), None, 0, None, 0, None) == -1
        # a system lig_linear_check rejects is LIG_E_ARG, nothing is launched
        beyond = system.to_binding(amd, slots=system.slots[:-1] + [len(kinds) * l])
        assert c.L.lig_rows_diagnose(tr, C.byref(beyond), None, 0, None, 0, C.byref(diag_info(amd))) == -1
        c.trace_destroy(tr)
    finally:
        c.close()


def diag_info(amd):
    info = amd.DiagInfo()
    info.struct_bytes = C.sizeof(amd.DiagInfo)
    return info


def test_heavy_constraints(amd):
    """exactly 2048 terms (the lane path) and 2049 (one workgroup per constraint), each once satisfied and once violated by one slot"""
    l, k, n = SMALL
    kinds = [LINEAR] * 14
    truth = field_rows(kinds, l, k, seed=9)
    rows = truth.copy()
    victim = 13 * l + 77                                      # only the violated constraints touch it
    set_wit(rows, l, victim, wit(truth, l, victim) + 1)
    rng = np.random.default_rng(4)
    good, bad = Builder(rows, l), Builder(truth, l)           # b_c from the shipped witness / from the witness before the change
    b = Builder(rows, l)
    b.coefs = [3, P - 4, (1 << 200) + 9]
    good.coefs = bad.coefs = b.coefs
    expect = []
    for count in (2048, 2049):
        for violated in (False, True):
            terms = [(int(s), [ONE, NEG_ONE, 0, 1, 2][int(ci)]) for s, ci in zip(rng.integers(0, 12 * l, count), rng.integers(0, 5, count))]
            if violated:
                terms[count // 2] = (victim, ONE)
            src = bad if violated else good
            rhs = sum(src.value(ci) * wit(src.rows, l, s) for s, ci in terms) % P
            cn = b.add(terms, b=rhs)
            if violated:
                expect.append((cn, 1))
            b.add([(int(rng.integers(0, 12 * l)), ONE)])        # small constraints in between
    system = b.system()
    assert [system.term_begin[i + 1] - system.term_begin[i] for i in (0, 2, 4, 6)] == [2048, 2048, 2049, 2049]
    c = amd.Context(l, k, n)
    try:
        tr = committed(amd, c, kinds, rows)
        want_l, _ = check(amd, c, tr, system, kinds, rows)
        assert want_l == expect and [cn for cn, _ in expect] == [2, 6]
        c.trace_destroy(tr)
    finally:
        c.close()


def test_quadratic_triples_of_every_width(amd):
    """a full-width, an 8-byte and a bit-packed triple, one wrong z slot each"""
    l, k, n = SMALL
    kinds = [QX, QY, QZ] * 3 + [LINEAR]
    rows = field_rows(kinds, l, k, seed=21)
    rng = np.random.default_rng(22)
    for base, hi in ((3, 1 << 32), (6, 2)):
        x, y = rng.integers(0, hi, l, dtype=np.uint64), rng.integers(0, hi, l, dtype=np.uint64)
        for d, v in enumerate((x, y, x * y)):
            rows[base + d, :l] = 0
            rows[base + d, :l, 0] = (v & 0xFFFFFFFF).astype(np.uint32)
            rows[base + d, :l, 1] = (v >> 32).astype(np.uint32)
    assert dr.quad_violations(kinds, rows, l) == []
    rows[2, 0, 3] ^= 1 << 9                                   # full width: column 0
    rows[5, l - 1, 1] ^= 1                                    # 8 bytes: the last column, bit 32
    rows[8, 257, 0] ^= 1                                      # bits: column 257 (another workgroup of the pass)
    widths = np.array([32, 32, 32, 8, 8, 8] + [amd.ELEM_BIT] * 3 + [32], dtype=np.uint8)
    k2, msgs = shipped(amd, kinds, rows, l)
    c = amd.Context(l, k, n)
    try:
        tr, keep = c.rows_begin(k2, amd.pack_rows(msgs, widths, l), generated_at=lr.GEN, elem_bytes=widths)
        c.rows_commit(tr)
        _, want_q = check(amd, c, tr, None, kinds, rows)
        assert [(x, y, z, i) for x, y, z, i, _ in want_q] == [(0, 1, 2, 0), (3, 4, 5, l - 1), (6, 7, 8, 257)]
        check(amd, c, tr, None, kinds, rows, quad_cap=2)
        c.trace_destroy(tr)
    finally:
        c.close()


def batch_trace():
    """rows of a batch program in front of the synthetic stream: init rows, a batch product, an equality pair, four bit rows"""
    l, k, n = SMALL
    p = batch_prog.Program()
    p.set(0, [3 + 2 * i for i in range(10)])
    p.set_scalar(1, 9)
    p.mul(2, 0, 1)
    p.copy(3, 2)
    p.set(4, [5, 2, 1])
    p.bit_decompose([5, 6, 7, 8], 4)
    kinds, rows, _ = lr.build_trace(l, k, n, l + 5, l + 3, p)
    return kinds, rows


def test_bit_equality_and_batch_product_rows(amd):
    l, k, n = SMALL
    kinds, rows = batch_trace()
    assert 12 <= len(kinds) <= 40 and {5, 6, 7, 8, 9, 10} <= set(int(v) for v in kinds)
    assert dr.quad_violations(kinds, rows, l) == []
    rows = rows.copy()
    bit, eqy, bqz = [int(np.flatnonzero(kinds == kd)[0]) for kd in (BIT, EQY, 10)]
    rows[bit, 3, 0] = 2                                       # a BIT row holding a 2: residual 2
    rows[eqy, 300, 0] ^= 1                                    # an EQX / EQY pair differing in one column
    rows[bqz, 1, 2] ^= 4                                      # a batch product with a wrong z
    c = amd.Context(l, k, n)
    try:
        tr = committed(amd, c, kinds, rows)
        _, want_q = check(amd, c, tr, None, kinds, rows)
        assert sorted((x, y, z, i) for x, y, z, i, _ in want_q) == sorted([(bit, bit, bit, 3), (eqy - 1, dr.NO_ROW, eqy, 300), (bqz - 2, bqz - 1, bqz, 1)])
        assert (bit, bit, bit, 3, 2) in want_q
        c.trace_destroy(tr)
    finally:
        c.close()


def test_trace_without_a_quadratic_term(amd):
    l, k, n = SMALL
    kinds = [LINEAR] * 12
    rows = field_rows(kinds, l, k, seed=31)
    b = Builder(rows, l)
    b.add([(3, ONE), (400, NEG_ONE)])
    b.add([(3, ONE)], off=1)
    c = amd.Context(l, k, n)
    try:
        tr = committed(amd, c, kinds, rows)
        want_l, want_q = check(amd, c, tr, b.system(), kinds, rows)
        assert want_l == [(1, P - 1)] and want_q == []
        check(amd, c, tr, None, kinds, rows)                  # no system either: nothing to evaluate
        c.trace_destroy(tr)
    finally:
        c.close()


def test_derived_product_triple_pinned_to_a_wrong_value(amd):
    l, k, n = SMALL
    kinds = [LINEAR] * 9 + [QX, QY, QZ]
    rows = field_rows(kinds, l, k, seed=41)                   # rows[11] = x * y mod p: what the library derives
    b = Builder(rows, l)
    b.add([(11 * l + 17, ONE)])                               # z[17] = x[17] * y[17]: holds
    wrong = b.add([(11 * l + 18, ONE)], off=1)                # z[18] pinned to x * y + 1
    b.add([(11 * l + 319, NEG_ONE), (5, ONE)])
    system = b.system()
    widths = np.array([32] * 11 + [amd.ELEM_PRODUCT], dtype=np.uint8)
    k2, msgs = shipped(amd, kinds, rows, l)
    msgs[11] = 0x5A5A5A5A                                     # (not shipped)
    c = amd.Context(l, k, n)
    try:
        tr, keep = c.rows_begin(k2, amd.pack_rows(msgs, widths, l), generated_at=lr.GEN, elem_bytes=widths)
        c.rows_commit(tr)
        want_l, want_q = check(amd, c, tr, system, kinds, rows)
        assert want_q == [] and want_l == [(wrong, P - 1)]
        c.trace_destroy(tr)
    finally:
        c.close()


def test_window_and_pipelining(amd):
    cz = small_case()
    l, system, kinds = SMALL[0], cz["system"], cz["kinds"]
    used = sorted(set(system.slots) - {system.hot_slot})
    traces = []
    for i in range(2):
        rows = cz["rows"].copy()
        s = used[10 + 50 * i]
        set_wit(rows, l, s, wit(rows, l, s) + 1)
        traces.append(rows)
    assert dr.linear_violations(system, traces[0], l) != dr.linear_violations(system, traces[1], l)
    c = amd.Context(*SMALL)
    try:
        sysb = system.to_binding(amd)

        def rc():
            return c.L.lig_rows_diagnose(tr, C.byref(sysb), None, 0, None, 0, C.byref(diag_info(amd)))

        k2, m0 = shipped(amd, kinds, traces[0], l)
        _, m1 = shipped(amd, kinds, traces[1], l)
        tr, keep = c.rows_begin(k2, m0, generated_at=lr.GEN)
        assert rc() == -3                                     # before the first commit
        c.rows_set_linear(tr, sysb)
        c.rows_commit(tr)
        c.rows_restart(tr, m1)                                # between commit and prove: the second matrix
        check(amd, c, tr, system, kinds, traces[0])
        c.rows_prove(tr, None, None)
        check(amd, c, tr, system, kinds, traces[0])           # the proof does not end the window
        c.rows_commit(tr)
        check(amd, c, tr, system, kinds, traces[1])
        c.rows_prove(tr, None, None)
        c.rows_restart(tr, m0)                                # after prove: straight into the matrix
        assert rc() == -3
        c.rows_commit(tr)
        check(amd, c, tr, system, kinds, traces[0])
        c.trace_destroy(tr)
        tr = c.synth_prepare(700, 330)
        assert c.L.lig_rows_diagnose(tr, None, None, 0, None, 0, C.byref(diag_info(amd))) == -3
        c.trace_destroy(tr)
    finally:
        c.close()


def test_envelope_of_a_diagnosed_trace_is_unchanged(amd):
    cz = small_case()
    l, system, kinds = SMALL[0], cz["system"], cz["kinds"]
    c = amd.Context(*SMALL)
    try:
        proofs = []
        for diagnose in (False, True):
            tr = committed(amd, c, kinds, cz["rows"])
            c.rows_set_linear(tr, system.to_binding(amd))
            if diagnose:
                check(amd, c, tr, system, kinds, cz["rows"])
            proof, info = c.rows_prove(tr, None, None)
            proofs.append((proof, bytes(info.const_sum), bytes(info.stage2_seed)))
            c.trace_destroy(tr)
        assert proofs[0] == proofs[1]
    finally:
        c.close()


def test_grid_stride_boundary(amd):
    """300,000 single-term constraints: more than 1024 workgroups x 256 lanes, so lanes take a second constraint"""
    l, k, n = SMALL
    R, NC = 940, 300000
    kinds = [LINEAR] * R
    rows = np.zeros((R, k, 8), dtype=np.uint32)
    slot = np.arange(R * l, dtype=np.uint32)
    rows[:, :l, 0] = (slot % 251 + 1).reshape(R, l)           # w[s] = s % 251 + 1
    cons = np.arange(NC)
    system = lr.System(range(NC + 1), cons, [ONE] * NC, cons, cons % 251, range(1, 252), 0)        # w[c] = table[c % 251]
    planted = [0, 262143, 262144, 299999]
    for s in planted:
        rows[s // l, s % l, 0] += 1000
    c = amd.Context(l, k, n)
    try:
        tr = committed(amd, c, kinds, rows)
        want_l, _ = check(amd, c, tr, system, kinds, rows)
        assert want_l == [(s, 1000) for s in planted]
        c.trace_destroy(tr)
    finally:
        c.close()


def test_packing_size_that_is_no_multiple_of_the_workgroup(amd):
    l, k, n = BIG
    assert l % 256
    kinds = [LINEAR, LINEAR, QX, QY, QZ, LINEAR]
    rows = field_rows(kinds, l, k, seed=51)
    rng = np.random.default_rng(52)
    b = Builder(rows, l)
    b.coefs = [5, P - 3, (1 << 253) + 1]
    lin_slots = [r * l + i for r in (0, 1, 5) for i in (0, 255, 256, l - 1)]
    for i in range(2000):
        terms = [(int(s), [ONE, NEG_ONE, 0, 1, 2][int(ci)]) for s, ci in zip(rng.integers(0, 6 * l, 3), rng.integers(0, 5, 3))]
        b.add(terms + ([(lin_slots[i % len(lin_slots)], ONE)] if i % 7 == 0 else []))
    for s in (l - 1, 5 * l + 256):
        set_wit(rows, l, s, wit(rows, l, s) + 3)              # after the right-hand sides were fixed
    rows[4, l - 1, 0] ^= 1                                    # z wrong in the last column
    rows[4, 4096, 5] ^= 2
    c = amd.Context(l, k, n)
    try:
        tr = committed(amd, c, kinds, rows)
        want_l, want_q = check(amd, c, tr, b.system(), kinds, rows)
        assert len(want_l) >= 2 and [(x, y, z, i) for x, y, z, i, _ in want_q] == [(2, 3, 4, 4096), (2, 3, 4, l - 1)]
        c.trace_destroy(tr)
    finally:
        c.close()


def test_quadratic_slices(amd):
    """3300 bit rows x 320 columns: more items than one slice of the quadratic pass holds (2^20); violations on both sides of the boundary"""
    l, k, n = SMALL
    R = 3300
    per = (1 << 20) // l
    assert per < R
    kinds = [BIT] * R
    rng = np.random.default_rng(61)
    rows = np.zeros((R, k, 8), dtype=np.uint32)
    rows[:, :, 0] = rng.integers(0, 2, (R, k))
    planted = [(0, 0), (per - 1, l - 1), (per, 0), (per, 5), (R - 1, l - 1)]
    for r, i in planted:
        rows[r, i, 0] = 2 + r
    c = amd.Context(l, k, n)
    try:
        tr = committed(amd, c, kinds, rows)
        _, want_q = check(amd, c, tr, None, kinds, rows)
        assert [(x, i) for x, _, _, i, _ in want_q] == planted
        check(amd, c, tr, None, kinds, rows, quad_cap=3)      # the cap is reached in the second slice
        check(amd, c, tr, None, kinds, rows, quad_cap=2)      # ... in the first
        c.trace_destroy(tr)
    finally:
        c.close()
