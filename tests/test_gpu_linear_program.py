"""GPU: prepared linear systems -- one lig_linear_program for many proofs, verifications and contexts (lig_linear_prepare,
lig_rows_attach_linear, lig_rows_verify_attach_linear, lig_rows_set_linear_values, lig_rows_verify_set_linear_values,
lig_linear_program_form).

Everything runs at (l, k, n) = (320, 512, 2048) on a trace of 16 rows; equality is bit-exact.  Expected values never come from the
entries under test: matrix and constant are tests/linear_ref.py's restatement in Python integers, envelopes are the oracle's prover
over that matrix, and the one-owner entries (lig_rows_set_linear, lig_rows_verify_set_linear, lig_linear_form -- themselves pinned to
the oracle by tests/test_gpu_linear_system.py) say what an attached program has to reproduce.

The system (Structure below) has a FIXED structure and a table that is a function of (fixed coefficients F, witness w): every
constraint with terms has a right-hand side with a table entry of its own, b_c = sum a * w.  So two statements of the same program --
T = table(F, w) and T' = table(F', w') -- share term list and right-hand-side indices and differ in the VALUES only: what
lig_rows_set_linear_values is for.  No test hands a kernel an invalid index: the misuse cases check codes of calls that launch nothing."""
import ctypes as C

import numpy as np
import pytest

import hip_lib
import linear_ref as lr
import oracle_lib as ol

pytestmark = pytest.mark.gpu

L_, K_, N_ = 320, 512, 2048
P = lr.P
N_LIN, N_QUAD = 6 * 320 + 17, 2 * 320 + 9
N_CONSTRAINTS, FIRST_RANDOM, HOT_TERMS, N_ASSERT = 2600, 1000, 2100, 40
F0 = [0, 1, P - 1, 2, 1 << 200, (1 << 253) + 12345] + [int(v) for v in ol.from_limbs(ol.rand_field(np.random.default_rng(77), 7))]
F1 = F0[:3] + [3, 1 << 199, (1 << 253) + 54321] + [(v * 7 + 1) % P for v in F0[6:]]          # other values, same length


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


class Structure:
    """the fixed part: which constraint touches which slot with which coefficient index, which table entry is its right-hand side.
    On purpose: +1 / -1 and table coefficients; constraints without terms; a slot repeated inside a constraint; untouched rows at the
    front, in the middle and at the end; terms on the rows of the quadratic triples; one slot with more than 2048 terms, table
    coefficients among them; N_ASSERT constraints +1 * w[s] = b on slots nothing else touches (the public outputs)."""

    def __init__(self, kinds):
        l = L_
        rng = np.random.default_rng(2024)
        ok = [r for r in range(len(kinds)) if kinds[r] <= 3]
        self.untouched = [ok[0], ok[len(ok) // 2], ok[-1]]
        assert kinds[ok[0]] == 0 and kinds[ok[1]] == 0 and kinds[ok[-1]] == 3 and ok[-1] == len(kinds) - 1 and ok[0] == 0
        pool = np.array([r * l + c for r in ok if r not in self.untouched for c in range(l)], dtype=np.int64)
        assert any(kinds[s // l] > 0 for s in pool)
        self.hot, self.asserts, draw = int(pool[0]), [int(s) for s in pool[1:1 + N_ASSERT]], pool[1 + N_ASSERT:]
        self.free_slots = [ok[0] * l + c for c in range(8)]                   # on the untouched front row: no constraint sees them
        nf = len(F0)

        def pick():
            u = rng.random()
            return lr.ONE if u < 0.4 else lr.NEG_ONE if u < 0.7 else int(rng.integers(0, nf))

        self.term_begin, self.slots, self.cidx, self.rhs_c, self.rhs_b = [0], [], [], [], []
        for c in range(N_CONSTRAINTS):
            if c < N_ASSERT:
                terms = [(self.asserts[c], lr.ONE)]
            elif c % 97 == 5:
                terms = []
            else:
                terms = [(int(s), pick()) for s in rng.choice(draw, size=int(rng.integers(1, 5)))]
                if c % 11 == 0:
                    terms.append((terms[0][0], pick()))
            if 50 <= c < 50 + HOT_TERMS:
                terms.append((self.hot, pick()))
            for s, ci in terms:
                self.slots.append(s)
                self.cidx.append(ci)
            self.term_begin.append(len(self.slots))
            if terms:
                self.rhs_c.append(c)
                self.rhs_b.append(nf + len(self.rhs_b))
        assert sum(1 for s in self.slots if s == self.hot) > 2048
        assert any(ci < nf for s, ci in zip(self.slots, self.cidx) if s == self.hot)

    def table(self, fixed, rows):
        """F + the right-hand sides that make the statement hold for the witnesses in `rows`"""
        w = lr.witness(rows, L_)
        probe = lr.System(self.term_begin, self.slots, self.cidx, [], [], fixed, FIRST_RANDOM)
        out = list(fixed)
        for c in self.rhs_c:
            out.append(sum(probe.coef(self.cidx[t]) * w[self.slots[t]] for t in range(self.term_begin[c], self.term_begin[c + 1])) % P)
        return out

    def system(self, table):
        return lr.System(self.term_begin, self.slots, self.cidx, self.rhs_c, self.rhs_b, table, FIRST_RANDOM)


class World:
    """the trace, its three witness variants and the two tables; oracle envelopes are computed once per (rows, table) and shared"""

    def __init__(self):
        self.kinds, rows, self.masks = lr.build_trace(L_, K_, N_, N_LIN, N_QUAD)
        self.st = Structure(self.kinds)
        rng = np.random.default_rng(9)
        self.rows = {"A": rows, "A2": rows.copy(), "B": rows.copy()}
        for s in self.st.free_slots:                                          # A2: another witness of the SAME statement
            self.rows["A2"][s // L_, s % L_] = ol.rand_field(rng, 1)[0]
        for s in self.st.asserts[::3]:                                        # B: other public outputs
            self.rows["B"][s // L_, s % L_] = ol.rand_field(rng, 1)[0]
        self.T = self.st.table(F0, self.rows["A"])
        self.T2 = self.st.table(F1, self.rows["B"])
        assert len(self.T) == len(self.T2) and self.T != self.T2
        self.sysT, self.sysT2 = self.st.system(self.T), self.st.system(self.T2)
        assert lr.holds(self.sysT, self.rows["A"], L_) and lr.holds(self.sysT, self.rows["A2"], L_) and lr.holds(self.sysT2, self.rows["B"], L_)
        assert not lr.holds(self.sysT, self.rows["B"], L_) and not lr.holds(self.sysT2, self.rows["A"], L_)
        self._oracle = {}

    def oracle(self, which, table):
        """-> (stage-1 seed, Rn, const_sum, the oracle's proof dict) for rows[which] under sysT / sysT2"""
        key = (which, table)
        if key not in self._oracle:
            self._oracle[key] = lr.oracle_envelope(L_, K_, N_, self.kinds, self.rows[which], self.masks, self.sysT if table == "T" else self.sysT2)
        return self._oracle[key]

    def shipped(self, amd, which):
        kinds, msgs = self.kinds.copy(), self.rows[which].copy()
        msgs[:, L_:] = 0xDEADBEEF                                             # every row is LINEAR / QX / QY / QZ: the library draws the pads
        return kinds | amd.ROW_DRAW_PAD, msgs


_world = []


@pytest.fixture(scope="module")
def W():
    if not _world:
        _world.append(World())
    return _world[0]


def vflags(v):
    return [v.valid_merkle, v.valid_code, v.valid_linear, v.valid_quad, v.code_equal, v.linear_equal, v.quad_equal, v.accept]


def pflags(info):
    return (info.valid_code, info.valid_linear, info.valid_quad)


def prove(c, amd, W, which, setup, encoding_seed=None):
    """begin -> setup(trace) -> commit -> prove(NULL, NULL) -> (proof, const_sum, flags)"""
    kinds, msgs = W.shipped(amd, which)
    tr, keep = c.rows_begin(kinds, msgs, generated_at=lr.GEN, encoding_seed=encoding_seed)
    try:
        setup(tr)
        c.rows_commit(tr)
        proof, info = c.rows_prove(tr, None, None)
        return proof, bytes(info.const_sum), pflags(info)
    finally:
        c.trace_destroy(tr)


# ---------------------------------------------------------------- 1: the stand-alone form
def test_program_form_equals_linear_form_and_the_python_matrix(amd, W):
    R = len(W.kinds)
    key = bytes((5 * i + 3) & 0xFF for i in range(32))
    c = amd.Context(L_, K_, N_)
    try:
        for system in (W.sysT, lr.make_equality_system(W.kinds, L_, 0)):
            if not system.coefs:
                assert system.rhs_constraint == [] and len(system.slots) > 0     # n_coefs == 0 and n_rhs == 0
            rn, cs = lr.expected(system, key, R, L_, K_)
            sysb = system.to_binding(amd)
            a = c.upload(np.full((R, K_, 8), 0xA5A5A5A5, dtype=np.uint32))
            b = c.upload(np.full((R, K_, 8), 0x5A5A5A5A, dtype=np.uint32))
            with c.linear_prepare(sysb, W.kinds) as prog:
                cs_prog = c.linear_program_form(prog, key, a)
                cs_form = c.linear_form(sysb, W.kinds, key, b)
                got = c.download(a, (R, K_, 8))
                assert np.array_equal(got, c.download(b, (R, K_, 8))) and cs_prog == cs_form
                bad = np.argwhere((got != rn).any(axis=2))
                assert len(bad) == 0, "first differing (row, column): %s of %d" % (bad[:4].tolist(), len(bad))
                assert cs_prog == cs
                if system is W.sysT:
                    for r in W.st.untouched:                              # the memset runs: front, middle, end
                        assert not got[r].any()
                # the same program again: nothing of the first call is left in it
                c.write(a, np.full((R, K_, 8), 0x33333333, dtype=np.uint32))
                assert c.linear_program_form(prog, key, a) == cs and np.array_equal(c.download(a, (R, K_, 8)), rn)
            c.free(a)
            c.free(b)
    finally:
        c.close()


# ---------------------------------------------------------------- 2: the prover
def test_attached_program_proves_what_set_linear_proves_and_the_oracle(amd, W):
    c = amd.Context(L_, K_, N_)
    try:
        sysb = W.sysT.to_binding(amd)
        old = {which: prove(c, amd, W, which, lambda t: c.rows_set_linear(t, sysb)) for which in ("A", "A2")}      # what lig_rows_set_linear gives
        prog = c.linear_prepare(sysb, W.kinds)
        kinds, msgs = W.shipped(amd, "A")
        tr, keep = c.rows_begin(kinds, msgs, generated_at=lr.GEN)
        c.rows_attach_linear(tr, prog)
        prog.release()                                                        # the trace's reference keeps it
        for i, which in enumerate(("A", "A2", "A")):                          # restart with new rows, and back
            seed1, rn, cs, oracle = W.oracle(which, "T")
            again = W.shipped(amd, which)[1]                                  # (host rows stay referenced until the commit has returned)
            if i:
                c.rows_restart(tr, again)
            root, s1 = c.rows_commit(tr)
            assert (root, s1) == (oracle["root"], seed1)
            proof, info = c.rows_prove(tr, None, None)
            assert (proof, bytes(info.const_sum), pflags(info)) == old[which]
            assert proof == oracle["proof"] and bytes(info.const_sum) == cs and pflags(info) == (1, 1, 1) and oracle["valid"] == [1, 1, 1]
        # a constant given by the caller is used as given
        c.rows_restart(tr, msgs)
        c.rows_commit(tr)
        proof, info = c.rows_prove(tr, None, W.oracle("A", "T")[2])
        assert proof == W.oracle("A", "T")[3]["proof"]
        # attach replaces a system set the old way, and the reverse
        c.rows_restart(tr, msgs)
        c.rows_set_linear(tr, sysb)
        with c.linear_prepare(sysb, W.kinds) as p2:
            c.rows_attach_linear(tr, p2)
        c.rows_commit(tr)
        assert c.rows_prove(tr, None, None)[0] == proof
        c.rows_restart(tr, msgs)
        c.rows_set_linear(tr, sysb)
        c.rows_commit(tr)
        assert c.rows_prove(tr, None, None)[0] == proof
        # detached: the old rule is back
        c.rows_restart(tr, msgs)
        c.rows_attach_linear(tr, None)
        c.rows_commit(tr)
        with pytest.raises(amd.LigError, match=r"\(-1\)"):
            c.rows_prove(tr, None, None)
        c.trace_destroy(tr)
    finally:
        c.close()


# ---------------------------------------------------------------- 3: one program, two contexts
@pytest.mark.parametrize("destroy_first", [0, 1])
def test_one_program_two_contexts_two_traces_in_flight(amd, W, destroy_first):
    seeds = [bytes(range(32)), bytes((11 * i + 7) & 0xFF for i in range(32))]
    which = ["A", "A2"]
    ctxs = [amd.Context(L_, K_, N_), amd.Context(L_, K_, N_)]
    try:
        sysb = W.sysT.to_binding(amd)
        want = [prove(ctxs[i], amd, W, which[i], lambda t, i=i: ctxs[i].rows_set_linear(t, sysb), encoding_seed=seeds[i]) for i in range(2)]
        assert want[0][0] != want[1][0]
        prog = ctxs[0].linear_prepare(sysb, W.kinds)
        traces, keeps = [], []
        for i in range(2):
            kinds, msgs = W.shipped(amd, which[i])
            tr, keep = ctxs[i].rows_begin(kinds, msgs, generated_at=lr.GEN, encoding_seed=seeds[i])
            ctxs[i].rows_attach_linear(tr, prog)
            traces.append(tr)
            keeps.append(keep)
        for i in range(2):
            ctxs[i].rows_commit(traces[i])                                    # both committed before either is proved
        prog.release()                                                        # ... and the caller's reference is gone before the proofs
        got = []
        for i in range(2):
            proof, info = ctxs[i].rows_prove(traces[i], None, None)
            got.append((proof, bytes(info.const_sum), pflags(info)))
        assert got == want
        order = [destroy_first, 1 - destroy_first]
        ctxs[order[0]].trace_destroy(traces[order[0]])
        # the survivor still reads the program: one more proof
        j = order[1]
        again = W.shipped(amd, which[j])[1]
        ctxs[j].rows_restart(traces[j], again)
        ctxs[j].rows_commit(traces[j])
        proof, info = ctxs[j].rows_prove(traces[j], None, None)
        assert (proof, bytes(info.const_sum), pflags(info)) == want[j]
        ctxs[j].trace_destroy(traces[j])
    finally:
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------- 4: the verifier
def test_one_program_verifies_many_proofs(amd, W):
    c = amd.Context(L_, K_, N_)
    try:
        sysb = W.sysT.to_binding(amd)
        old = lambda t: c.rows_set_linear(t, sysb)
        good = [W.oracle("A", "T")[3]["proof"], W.oracle("A2", "T")[3]["proof"],
                prove(c, amd, W, "A", old, encoding_seed=bytes((3 * i + 1) & 0xFF for i in range(32)))[0]]
        assert len(set(good)) == 3
        false_proof, _, fl = prove(c, amd, W, "B", old)                       # rows B do not satisfy T
        assert fl == (1, 0, 1)
        tampered = bytearray(good[0])
        tampered[len(tampered) // 2] ^= 0x40
        tampered = bytes(tampered)

        def verify(proof, how):
            vt, _, vi = c.rows_verify_begin(W.kinds, proof)
            if vt is None:
                return [vi.parsed, vi.indices_match, "rejected at begin"]
            how(vt)
            return vflags(c.rows_verify_finish(vt, None, None))

        prog = c.linear_prepare(sysb, W.kinds)
        attach = lambda vt: c.rows_verify_attach_linear(vt, prog)
        setlin = lambda vt: c.rows_verify_set_linear(vt, sysb)
        for proof in good:
            v = verify(proof, attach)
            assert v == [1] * 8 and v == verify(proof, setlin)
        v = verify(false_proof, attach)
        assert v == verify(false_proof, setlin) and v[2] == 0 and v[7] == 0 and v[0] == 1
        v = verify(tampered, attach)
        assert v == verify(tampered, setlin) and v[-1] != 1
        # a verification given up between begin and finish leaks no reference: the release below frees the program, and a program
        # prepared afterwards serves as the first did
        vt, _, _ = c.rows_verify_begin(W.kinds, good[1])
        c.rows_verify_attach_linear(vt, prog)
        c.vtrace_destroy(vt)
        prog.release()
        with pytest.raises(amd.LigError, match="released"):
            attach(None)
        with c.linear_prepare(sysb, W.kinds) as prog2:
            assert verify(good[1], lambda vt: c.rows_verify_attach_linear(vt, prog2)) == [1] * 8
            # attach replaces set_linear on the verifier too, and NULL detaches
            vt, _, _ = c.rows_verify_begin(W.kinds, good[2])
            c.rows_verify_set_linear(vt, sysb)
            c.rows_verify_attach_linear(vt, prog2)
            c.rows_verify_attach_linear(vt, None)
            assert c.L.lig_rows_verify_finish(vt, None, 0, None, C.byref(amd.VerifyInfo())) == -1      # no system, no constant
            c.vtrace_destroy(vt)
    finally:
        c.close()


# ---------------------------------------------------------------- 5: values, prover side
def test_values_belong_to_the_attachment_prover(amd, W):
    c, cb = amd.Context(L_, K_, N_), amd.Context(L_, K_, N_)
    try:
        sysT, sysT2 = W.sysT.to_binding(amd), W.sysT2.to_binding(amd)
        want_T = prove(c, amd, W, "A", lambda t: c.rows_set_linear(t, sysT))
        want_T2 = prove(c, amd, W, "B", lambda t: c.rows_set_linear(t, sysT2))           # a fresh lig_rows_set_linear with coefs = T'
        oT, oT2 = W.oracle("A", "T"), W.oracle("B", "T2")
        assert want_T == (oT[3]["proof"], oT[2], (1, 1, 1)) and want_T2 == (oT2[3]["proof"], oT2[2], (1, 1, 1))
        with c.linear_prepare(sysT, W.kinds) as prog:                         # the program carries T
            msgs = {w: W.shipped(amd, w)[1] for w in ("A", "B")}
            kinds = W.shipped(amd, "A")[0]
            ta, ka = c.rows_begin(kinds, msgs["A"], generated_at=lr.GEN)
            tb, kb = cb.rows_begin(kinds, msgs["B"], generated_at=lr.GEN)
            c.rows_attach_linear(ta, prog)
            cb.rows_attach_linear(tb, prog)
            cb.rows_set_linear_values(tb, W.T2)                               # two traces on one program: T and T'
            c.rows_commit(ta)
            cb.rows_commit(tb)

            def run(cx, t):
                proof, info = cx.rows_prove(t, None, None)
                return proof, bytes(info.const_sum), pflags(info)

            assert run(cb, tb) == want_T2 and run(c, ta) == want_T
            # values persist across lig_rows_restart
            cb.rows_restart(tb, msgs["B"])
            cb.rows_commit(tb)
            assert run(cb, tb) == want_T2
            # the same table given as limbs, set after the commit
            cb.rows_restart(tb, msgs["B"])
            cb.rows_commit(tb)
            cb.rows_set_linear_values(tb, amd.coef_table(W.T2))
            assert run(cb, tb) == want_T2
            # NULL: back to the program's own table; rows A under it
            cb.rows_restart(tb, msgs["A"])
            cb.rows_set_linear_values(tb, None)
            cb.rows_commit(tb)
            assert run(cb, tb) == want_T
            # 6b: a witness that satisfies T but not T' fails the prover's own linear check under T'
            c.rows_restart(ta, msgs["A"])
            c.rows_set_linear_values(ta, W.T2)
            c.rows_commit(ta)
            proof, cs, fl = run(c, ta)
            assert fl == (1, 0, 1) and cs == lr.expected(W.sysT2, oT[0], len(W.kinds), L_, K_)[1]
            c.trace_destroy(ta)
            cb.trace_destroy(tb)
    finally:
        cb.close()
        c.close()


# ---------------------------------------------------------------- 6: values, verifier side
def test_values_are_part_of_the_statement_verifier(amd, W):
    c = amd.Context(L_, K_, N_)
    try:
        proof_T2 = W.oracle("B", "T2")[3]["proof"]                            # made under T'
        proof_T = W.oracle("A", "T")[3]["proof"]
        with c.linear_prepare(W.sysT.to_binding(amd), W.kinds) as prog:

            def verify(proof, values):
                vt, _, _ = c.rows_verify_begin(W.kinds, proof)
                c.rows_verify_attach_linear(vt, prog)
                if values is not None:
                    c.rows_verify_set_linear_values(vt, values)
                return vflags(c.rows_verify_finish(vt, None, None))

            assert verify(proof_T2, W.T2) == [1] * 8
            v = verify(proof_T2, None)                                        # with T: another statement
            assert v[2] == 0 and v[7] == 0 and v[0] == 1 and v[1] == 1 and v[3] == 1
            assert verify(proof_T, None) == [1] * 8                           # the values of one verification do not reach the next
            v = verify(proof_T, W.T2)
            assert v[2] == 0 and v[7] == 0
            # ... and answers what lig_rows_verify_set_linear answers for a system with coefs = T'
            vt, _, _ = c.rows_verify_begin(W.kinds, proof_T)
            c.rows_verify_set_linear(vt, W.sysT2.to_binding(amd))
            assert vflags(c.rows_verify_finish(vt, None, None)) == v
    finally:
        c.close()


# ---------------------------------------------------------------- 7: values, direct (k_lin_coefs_mont)
def test_program_form_with_values_of_257_entries(amd):
    n_coefs, rows = 257, 3
    rng = np.random.default_rng(5)
    T = [int(v) for v in ol.from_limbs(ol.rand_field(rng, n_coefs))]
    T2 = [int(v) for v in ol.from_limbs(ol.rand_field(rng, n_coefs))]
    T2[0], T2[1], T2[2], T2[3], T2[255], T2[256] = 0, 1, P - 1, (0x30644E72 << 224) + 5, P - 2, (0x30000000 << 224) | ((1 << 224) - 1)
    assert all(v < P for v in T2) and T2[3] >> 224 and T2[256] >> 224       # top limb set; entry 256 belongs to the second workgroup
    kinds = np.zeros(rows, dtype=np.uint8)
    # constraint i: table[i] * w[slot i] - w[slot i + 1] = table[(i + 1) % n_coefs]: every entry is read as a term and as a right-hand side
    tb, slots, cidx = [0], [], []
    for i in range(n_coefs):
        slots += [i, i + 1]
        cidx += [i, lr.NEG_ONE]
        tb.append(len(slots))
    mk = lambda tab: lr.System(tb, slots, cidx, list(range(n_coefs)), [(i + 1) % n_coefs for i in range(n_coefs)], tab, 7)
    key = bytes(range(100, 132))
    c = amd.Context(L_, K_, N_)
    try:
        out = c.upload(np.full((rows, K_, 8), 0xA5A5A5A5, dtype=np.uint32))
        with c.linear_prepare(mk(T).to_binding(amd), kinds) as prog:
            for tab, values in ((T2, T2), (T, None), (T2, amd.coef_table(T2)), (T, T)):
                rn, cs = lr.expected(mk(tab), key, rows, L_, K_)
                assert c.linear_program_form(prog, key, out, coefs=values) == cs
                assert np.array_equal(c.download(out, (rows, K_, 8)), rn)
            # misuse of the direct entry: launches nothing
            with pytest.raises(amd.LigError, match=r"\(-1\)"):
                c.linear_program_form(prog, key, out, coefs=T2[:-1])
            with pytest.raises(amd.LigError, match=r"\(-1\)"):
                c.linear_program_form(prog, key, out, coefs=T2[:-1] + [P])
    finally:
        c.close()


# ---------------------------------------------------------------- 8: misuse
def test_misuse_returns_codes_and_launches_nothing(amd, W):
    E_ARG, E_STATE = -1, -3
    c = amd.Context(L_, K_, N_)
    c2 = amd.Context(300, K_, N_)                                             # another l
    try:
        sysb = W.sysT.to_binding(amd)
        kinds, msgs = W.shipped(amd, "A")
        other_kinds = W.kinds.copy()
        other_kinds[0] = amd.ROW_KINDS["INIT"]                                # row 0 carries no term: lig_linear_check accepts both
        tiny = lr.System([0, 1], [0], [lr.ONE], [], [], [], 0).to_binding(amd)
        progs = dict(good=c.linear_prepare(sysb, W.kinds), kinds=c.linear_prepare(sysb, other_kinds),
                     rows=c.linear_prepare(sysb, W.kinds[:-1]), l=c2.linear_prepare(tiny, W.kinds))
        assert progs["good"].bytes()[0] > 0
        tr, keep = c.rows_begin(kinds, msgs, generated_at=lr.GEN)
        for name in ("kinds", "rows", "l"):
            assert c.L.lig_rows_attach_linear(tr, progs[name].h) == E_ARG, name
        out = c.malloc(len(W.kinds) * K_ * 32)
        key, cs_out = np.zeros(32, dtype=np.uint8), np.zeros(32, dtype=np.uint8)
        assert c.L.lig_linear_program_form(c.h, progs["l"].h, key.ctypes.data, None, 0, out, cs_out.ctypes.data) == E_ARG
        assert c.L.lig_rows_set_linear_values(tr, None, 0) == E_STATE         # values with nothing attached
        c.rows_attach_linear(tr, progs["good"])
        good_tab = amd.coef_table(W.T)
        assert c.L.lig_rows_set_linear_values(tr, good_tab.ctypes.data, len(good_tab) - 1) == E_ARG
        bad_tab = good_tab.copy()
        bad_tab[len(bad_tab) - 1] = amd.coef_table([P])[0]                    # the last entry = p
        assert c.L.lig_rows_set_linear_values(tr, bad_tab.ctypes.data, len(bad_tab)) == E_ARG
        c.rows_commit(tr)
        seed1, rn, cs, oracle = W.oracle("A", "T")
        with pytest.raises(amd.LigError, match=r"\(-1\)"):                    # rands != NULL with a program attached
            c.rows_prove(tr, rn, cs)
        pinned, ptr = c.host_alloc(K_ * 32)
        pinned[:] = 0
        assert c.L.lig_rows_push_rands(tr, 0, 1, ptr) == E_STATE
        # the trace is still usable, and nothing of the refused values stuck
        proof, info = c.rows_prove(tr, None, None)
        assert proof == oracle["proof"] and bytes(info.const_sum) == cs
        # attach after push_rands
        c.rows_restart(tr, msgs)
        c.rows_attach_linear(tr, None)
        c.rows_commit(tr)
        c.rows_push_rands(tr, 0, 1, ptr.value)
        assert c.L.lig_rows_attach_linear(tr, progs["good"].h) == E_STATE
        c.trace_destroy(tr)
        c.host_free(ptr)
        # a job with dense_rands_per_row
        dense = np.full(len(W.kinds), L_, dtype=np.uint32)
        tr, keep = c.rows_begin(kinds, msgs, generated_at=lr.GEN, dense_rands_per_row=dense)
        assert c.L.lig_rows_attach_linear(tr, progs["good"].h) == E_ARG
        c.trace_destroy(tr)
        # the verifier's side
        vt, _, _ = c.rows_verify_begin(W.kinds, oracle["proof"])
        for name in ("kinds", "rows", "l"):
            assert c.L.lig_rows_verify_attach_linear(vt, progs[name].h) == E_ARG, name
        assert c.L.lig_rows_verify_set_linear_values(vt, None, 0) == E_STATE
        c.rows_verify_attach_linear(vt, progs["good"])
        assert c.L.lig_rows_verify_set_linear_values(vt, good_tab.ctypes.data, len(good_tab) + 1) == E_ARG
        assert c.L.lig_rows_verify_set_linear_values(vt, bad_tab.ctypes.data, len(bad_tab)) == E_ARG
        assert c.L.lig_rows_verify_finish(vt, rn.ctypes.data, 0, None, C.byref(amd.VerifyInfo())) == E_ARG      # rands != NULL
        assert vflags(c.rows_verify_finish(vt, None, None)) == [1] * 8
        for p in progs.values():
            p.release()
        c.L.lig_linear_program_release(None)                                  # NULL is a no-op
    finally:
        c2.close()
        c.close()
