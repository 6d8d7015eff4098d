"""GPU: sparse linear constraints -- the linear-test randomness rows and the constant formed on the device (lig_linear_form,
lig_rows_set_linear, lig_rows_verify_set_linear).

Expected values never come from the library: the randomness matrix and the constant are restated in Python integers
(tests/linear_ref.py: r_c from the oracle's sampler, the two sums mod p), the expected envelope is the oracle's prover over that
matrix.  No test hands a kernel an invalid index; the misuse cases check return codes of calls that launch nothing.

The case with batch rows in front ("small_batch_rows"): the oracle's prove_rows takes LINEAR / QX / QY / QZ rows only and proves
batch rows only inside its own synthetic job, so it cannot produce the envelope of caller rows with batch kinds under a sparse
system.  There the root and the stage-1 seed come from the oracle (its prover over the same rows), matrix and constant from the
Python restatement, and the envelope is checked through the three self-check flags, the constant, the existing uploaded-matrix
path (itself pinned to the oracle with batch rows by test_gpu_rows_api.py) and the verifier's seven predicates."""
import numpy as np
import pytest

import hip_lib
import linear_ref as lr
import test_batch_rows as tb

pytestmark = pytest.mark.gpu

SMALL, BIG = (320, 512, 2048), (8000, 8192, 32768)
# name -> (shape, n_linear, n_quad, batch rows in front, narrow witnesses, system: (n_constraints, first_random) or "equalities")
CASES = {
    "small": (SMALL, 3 * 320 + 17, 320 + 9, False, False, (30000, 0)),
    "small_batch_rows": (SMALL, 2 * 320 + 5, 320, True, False, (70000, 1000)),
    "big": (BIG, 2 * 8000 + 123, 8000 + 5, False, False, (70000, 1000)),
    "equalities": (SMALL, 3 * 320, 0, False, False, "equalities"),
    "narrow": (SMALL, 4 * 320 + 7, 320 + 3, False, True, (30000, 1000)),
}
_cache = {}
_batch_proofs = {}


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


class Case:
    def __init__(self, name):
        (self.l, self.k, self.n), n_lin, n_quad, batch, self.narrow, sysdef = CASES[name]
        self.kinds, self.rows, self.masks = lr.build_trace(self.l, self.k, self.n, n_lin, n_quad, tb.demo_program() if batch else None, narrow=self.narrow)
        assert batch == bool((self.kinds > 3).any())
        if sysdef == "equalities":
            self.system = lr.make_equality_system(self.kinds, self.l, 0)
        else:
            self.system = lr.make_system(self.kinds, self.rows, self.l, sysdef[0], sysdef[1], seed=len(name))
        assert lr.holds(self.system, self.rows, self.l)
        if batch:
            self.root, self.seed1 = lr.oracle_commitment(self.l, self.k, self.n, n_lin, n_quad, tb.demo_program())
            self.rn, self.cs = lr.expected(self.system, self.seed1, len(self.kinds), self.l, self.k)
            self.oracle = None
            return
        self.seed1, self.rn, self.cs, self.oracle = lr.oracle_envelope(self.l, self.k, self.n, self.kinds, self.rows, self.masks, self.system)
        self.root = self.oracle["root"]
        assert self.oracle["valid"] == [1, 1, 1]

    def shipped(self, amd, rows=None):
        """(kinds | DRAW_PAD, rows with garbage in the pad slots the library draws)"""
        kinds, msgs = self.kinds.copy(), (self.rows if rows is None else rows).copy()
        draws = (kinds <= 3) | (kinds == amd.ROW_KINDS["INIT"])
        msgs[draws, self.l:] = 0xDEADBEEF
        kinds[draws] |= amd.ROW_DRAW_PAD
        return kinds, msgs


def case(name):
    if name not in _cache:
        _cache[name] = Case(name)
    return _cache[name]


def flags(v):
    return [v.valid_merkle, v.valid_code, v.valid_linear, v.valid_quad, v.code_equal, v.linear_equal, v.quad_equal]


@pytest.mark.parametrize("name", ["small", "small_batch_rows", "big", "equalities"])
def test_linear_form_equals_the_python_matrix(amd, name):
    cz = case(name)
    R = len(cz.kinds)
    c = amd.Context(cz.l, cz.k, cz.n)
    try:
        sysb = cz.system.to_binding(amd)
        assert c.linear_check(sysb, cz.kinds) == 0
        out = c.upload(np.full((R, cz.k, 8), 0xA5A5A5A5, dtype=np.uint32))       # every element must be written, zeros included
        cs = c.linear_form(sysb, cz.kinds, cz.seed1, out)
        got = c.download(out, (R, cz.k, 8))
        bad = np.argwhere((got != cz.rn).any(axis=2))
        assert len(bad) == 0, "first differing (row, column): %s of %d" % (bad[:4].tolist(), len(bad))
        assert cs == cz.cs
        # the same call again: the same bytes (the sums are exact, no result depends on the order the atomics of the prepare phase took)
        c.write(out, np.full((R, cz.k, 8), 0x5A5A5A5A, dtype=np.uint32))
        assert c.linear_form(sysb, cz.kinds, cz.seed1, out) == cs
        assert np.array_equal(c.download(out, (R, cz.k, 8)), got)
    finally:
        c.close()


@pytest.mark.parametrize("name", ["small", "small_batch_rows", "big", "equalities"])
def test_rows_prove_with_a_linear_system_equals_the_oracle_envelope(amd, name):
    cz = case(name)
    c = amd.Context(cz.l, cz.k, cz.n)
    try:
        kinds, msgs = cz.shipped(amd)
        sysb = cz.system.to_binding(amd)

        proofs = []

        def check(proof, info):
            assert bytes(info.const_sum) == cz.cs
            assert (info.valid_code, info.valid_linear, info.valid_quad) == (1, 1, 1)
            if cz.oracle is not None:
                assert proof == cz.oracle["proof"]
            proofs.append(proof)

        # set_linear after the commit
        tr, keep = c.rows_begin(kinds, msgs, generated_at=lr.GEN)
        root, seed1 = c.rows_commit(tr)
        assert root == cz.root and seed1 == cz.seed1
        c.rows_set_linear(tr, sysb)
        check(*c.rows_prove(tr, None, None))
        # the next trace of the same shape: the structure is resident, no second set_linear
        c.rows_restart(tr, msgs)
        assert c.rows_commit(tr) == (root, seed1)
        check(*c.rows_prove(tr, None, None))
        # a constant given by the caller is used as given
        c.rows_restart(tr, msgs)
        c.rows_commit(tr)
        check(*c.rows_prove(tr, None, cz.cs))
        c.trace_destroy(tr)
        # set_linear before the commit
        tr, keep = c.rows_begin(kinds, msgs, generated_at=lr.GEN)
        c.rows_set_linear(tr, sysb)
        assert c.rows_commit(tr) == (root, seed1)
        check(*c.rows_prove(tr, None, None))
        c.trace_destroy(tr)
        # consistency (not the yardstick): the existing path with the Python matrix uploaded gives the same bytes
        tr, keep = c.rows_begin(kinds, msgs, generated_at=lr.GEN)
        c.rows_commit(tr)
        check(*c.rows_prove(tr, cz.rn, cz.cs))
        c.trace_destroy(tr)
        assert len(proofs) == 5 and all(p == proofs[-1] for p in proofs)
        if cz.oracle is None:
            _batch_proofs[name] = proofs[0]
    finally:
        c.close()


def test_narrow_witness_rows_with_a_linear_system(amd):
    cz = case("narrow")
    c = amd.Context(cz.l, cz.k, cz.n)
    try:
        kinds, msgs = cz.shipped(amd)
        widths = amd.narrowest_widths(cz.rows, cz.kinds, cz.l)
        assert amd.ELEM_BIT in set(int(w) for w in widths) and 2 in set(int(w) for w in widths)      # bit rows and 2-byte rows
        packed = amd.pack_rows(msgs, widths, cz.l)
        sysb = cz.system.to_binding(amd)
        tr, keep = c.rows_begin(kinds, packed, generated_at=lr.GEN, elem_bytes=widths)
        c.rows_set_linear(tr, sysb)
        root, seed1 = c.rows_commit(tr)
        assert root == cz.oracle["root"] and seed1 == cz.seed1
        proof, info = c.rows_prove(tr, None, None)
        c.trace_destroy(tr)
        assert bytes(info.const_sum) == cz.cs and (info.valid_code, info.valid_linear, info.valid_quad) == (1, 1, 1)
        assert proof == cz.oracle["proof"]
        # ... which is the envelope of the full-width rows
        tr, keep = c.rows_begin(kinds, msgs, generated_at=lr.GEN)
        c.rows_set_linear(tr, sysb)
        c.rows_commit(tr)
        proof_full, _ = c.rows_prove(tr, None, None)
        c.trace_destroy(tr)
        assert proof_full == proof
    finally:
        c.close()


def test_false_statement_fails_the_linear_self_check_and_the_verifier(amd):
    cz = case("small")
    s = cz.system.single_slot                                                 # one term, coefficient +1: its randomness is r_0 != 0
    assert any(cz.rn[s // cz.l, s % cz.l])
    rows = cz.rows.copy()
    rows[s // cz.l, s % cz.l, 0] ^= 1                                         # the witness changed after b_c was fixed
    assert not lr.holds(cz.system, rows, cz.l)
    c = amd.Context(cz.l, cz.k, cz.n)
    try:
        kinds, msgs = cz.shipped(amd, rows)
        sysb = cz.system.to_binding(amd)
        tr, keep = c.rows_begin(kinds, msgs, generated_at=lr.GEN)
        c.rows_commit(tr)
        c.rows_set_linear(tr, sysb)
        proof, info = c.rows_prove(tr, None, None)
        c.trace_destroy(tr)
        assert (info.valid_code, info.valid_linear, info.valid_quad) == (1, 0, 1)
        vt, _, vi = c.rows_verify_begin(cz.kinds, proof)
        assert vt is not None and vi.parsed == 1 and vi.indices_match == 1
        c.rows_verify_set_linear(vt, sysb)
        v = c.rows_verify_finish(vt, None, None)
        assert v.valid_linear == 0 and v.valid_merkle == 1 and v.accept == 0
    finally:
        c.close()


@pytest.mark.parametrize("name", ["small", "small_batch_rows"])
def test_verifier_forms_matrix_and_constant_itself(amd, name):
    cz = case(name)
    c = amd.Context(cz.l, cz.k, cz.n)
    try:
        if cz.oracle is not None:
            proof = cz.oracle["proof"]                                        # = the proofs of the prover test, byte for byte
        else:                                                                 # batch rows: no oracle envelope (module docstring)
            if name not in _batch_proofs:
                kinds, msgs = cz.shipped(amd)
                tr, keep = c.rows_begin(kinds, msgs, generated_at=lr.GEN)
                assert c.rows_commit(tr) == (cz.root, cz.seed1)
                _batch_proofs[name] = c.rows_prove(tr, cz.rn, cz.cs)[0]
                c.trace_destroy(tr)
            proof = _batch_proofs[name]
        def verify(system, **override):
            vt, seed1, vi = c.rows_verify_begin(cz.kinds, proof)
            assert vt is not None and seed1 == cz.seed1 and vi.indices_match == 1
            c.rows_verify_set_linear(vt, system.to_binding(amd, **override))
            return c.rows_verify_finish(vt, None, None)

        v = verify(cz.system)
        assert flags(v) == [1] * 7 and v.accept == 1
        # ... and answers, predicate by predicate, what the verifier answers for the uploaded Python matrix
        vt, _, _ = c.rows_verify_begin(cz.kinds, proof)
        u = c.rows_verify_finish(vt, cz.rn, cz.cs)
        assert flags(u) == flags(v) and u.accept == v.accept
        sy = cz.system

        def rejected(v):
            assert v.accept == 0 and v.valid_merkle == 1 and (v.valid_linear == 0 or v.linear_equal == 0), flags(v)

        rejected(verify(sy, first_random=sy.first_random + 1))
        t = sy.coef_idx.index(lr.ONE, sy.term_begin[3])                       # one coefficient changed: +1 -> -1
        rejected(verify(sy, coef_idx=sy.coef_idx[:t] + [lr.NEG_ONE] + sy.coef_idx[t + 1:]))
        wrong = list(sy.rhs_coef)                                             # one right-hand side changed
        wrong[0] = 3 if wrong[0] != 3 else 4                                  # (table entries 3 and 4 are 2 and 4; b_c is neither, or the other)
        assert sy.coef(wrong[0]) != sy.coef(sy.rhs_coef[0])
        rejected(verify(sy, rhs_coef=wrong))
        for bad in (dict(first_random=sy.first_random + 1), dict(rhs_coef=wrong)):
            # predicate by predicate what the verifier says about the matrix / constant that system stands for
            other = lr.System(sy.term_begin, sy.slots, sy.coef_idx, sy.rhs_constraint, bad.get("rhs_coef", sy.rhs_coef), sy.coefs,
                              bad.get("first_random", sy.first_random))
            rn, cs = lr.expected(other, cz.seed1, len(cz.kinds), cz.l, cz.k)
            vt, _, _ = c.rows_verify_begin(cz.kinds, proof)
            assert flags(c.rows_verify_finish(vt, rn, cs)) == flags(verify(sy, **bad))
    finally:
        c.close()


def test_misuse_returns_codes(amd):
    cz = case("small")
    c = amd.Context(cz.l, cz.k, cz.n)
    try:
        kinds, msgs = cz.shipped(amd)
        sysb = cz.system.to_binding(amd)
        # a job with dense_rands_per_row
        dense = np.where(cz.kinds <= 3, cz.l, 0).astype(np.uint32)
        tr, keep = c.rows_begin(kinds, msgs, generated_at=lr.GEN, dense_rands_per_row=dense)
        assert c.L.lig_rows_set_linear(tr, sysb) == -1
        c.trace_destroy(tr)
        tr, keep = c.rows_begin(kinds, msgs, generated_at=lr.GEN)
        # a system lig_linear_check rejects: a slot beyond the rows, a slot on a row the trace does not have -- nothing is launched
        beyond = cz.system.to_binding(amd, slots=cz.system.slots[:-1] + [len(cz.kinds) * cz.l])
        assert c.linear_check(beyond, cz.kinds) == -1
        assert c.L.lig_rows_set_linear(tr, beyond) == -1
        out = c.malloc(len(cz.kinds) * cz.k * 32)
        with pytest.raises(amd.LigError):
            c.linear_form(beyond, cz.kinds, cz.seed1, out)
        c.rows_commit(tr)
        c.rows_set_linear(tr, sysb)
        # randomness rows next to a system
        with pytest.raises(amd.LigError, match=r"\(-1\)"):
            c.rows_prove(tr, cz.rn, cz.cs)
        pinned, ptr = c.host_alloc(cz.k * 32)
        pinned[:] = 0
        assert c.L.lig_rows_push_rands(tr, 0, 1, ptr) == -3
        # removing the system brings the old rule back: no randomness rows, no proof
        c.rows_set_linear(tr, None)
        with pytest.raises(amd.LigError, match=r"\(-1\)"):
            c.rows_prove(tr, None, None)
        # pushed rows first, then a system
        c.rows_push_rands(tr, 0, 1, ptr.value)
        assert c.L.lig_rows_set_linear(tr, sysb) == -3
        c.trace_destroy(tr)
        c.host_free(ptr)
        # the verifier without a system keeps its rules
        vt, _, _ = c.rows_verify_begin(cz.kinds, cz.oracle["proof"])
        assert c.L.lig_rows_verify_set_linear(vt, beyond) == -1
        assert c.L.lig_rows_verify_finish(vt, None, 0, None, None) == -1
        c.vtrace_destroy(vt)
    finally:
        c.close()
