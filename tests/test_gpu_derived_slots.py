"""GPU: derived slots (lig_rows_set_derived) -- the outputs of linear constraints formed on the device in stage 1.  Every expected byte
comes from Python integers (tests/derived_ref.py, tests/test_linear_system.py::mul_add_terms) and from the oracle's prover over rows that
carry those integers; never from the derived path itself.  All shapes are l = 320, k = 512, n = 2048."""
import json
import os

import numpy as np
import pytest

import derived_ref as dr
import hip_lib
import linear_ref as lr
import oracle_lib as ol
from test_linear_system import mul_add_terms

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
L, K, N = dr.L, dr.K, dr.N
_oracle = {}


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def oracle(amd, seed, which):
    """the oracle's envelope over the world's expected / shipped rows, computed once"""
    if (seed, which) not in _oracle:
        W = dr.world(amd, seed)
        _oracle[seed, which] = W.oracle(W.expected_rows if which == "expected" else W.shipped_rows)
    return _oracle[seed, which]


def read_targets(c, tr, W):
    return ol.from_limbs(c.rows_read_slots(tr, W.targets))


def test_recorded_mul_add_guest_with_every_eval_output_derived(amd):
    """w = eval(a * b + a - 3): the QX / QY rows narrow, the QZ rows LIG_ELEM_PRODUCT, every LINEAR row an all-zero bit row whose slots
    are derived from constraint 2i (z + a - w = 3) -- the envelope is the oracle's over the recorded rows"""
    d = np.load(os.path.join(GOLD, "ref_rows_mul_add_320.npz"))
    meta = json.loads(str(d["meta"]))
    l, k, n, reps = meta["l"], meta["k"], meta["n"], meta["reps"]
    assert (l, k, n) == (L, K, N)
    kinds, vals = d["kinds"], d["vals"]
    key = bytes.fromhex(meta["encoding_seed"])
    w = lr.witness(vals, l)
    s = mul_add_terms(reps, l, w)
    pairs = [(4 * (i // l) * l + i % l, 2 * i) for i in range(reps)]
    masks = ol.form_masks(key, len(kinds) * (k - l), l, k)
    want = lr.oracle_envelope(l, k, n, kinds, vals, masks, s)[3]
    assert want["valid"] == [1, 1, 1]
    kk = kinds | amd.ROW_DRAW_PAD                                   # the library draws the pads the recording carries
    widths = amd.narrowest_widths(vals, kinds, l, derive_products=True)
    blind = vals.copy()
    blind[kinds == 0] = 0                                           # nothing of w reaches the library
    widths[kinds == 0] = amd.ELEM_BIT
    blind[kinds == 3] = 0xDEADBEEF
    packed = amd.pack_rows(blind, widths, l)
    lin_slots = [r * l + c for r in range(len(kinds)) if kinds[r] == 0 for c in range(l)]
    c = amd.Context(l, k, n)
    try:
        sysb = s.to_binding(amd)
        assert list(amd.derived_check(sysb, kinds, l, pairs, widths)) == [1] * reps
        tr, keep = c.rows_begin(kk, packed, encoding_seed=key, generated_at=lr.GEN, elem_bytes=widths)
        c.rows_set_linear(tr, sysb)
        info = c.rows_set_derived(tr, sysb, pairs)
        assert (info.n_slots, info.n_terms, info.n_waves) == (reps, 2 * reps, 1)
        root, seed1 = c.rows_commit(tr)
        assert root == want["root"] and seed1 == want["stage1_seed"]
        assert ol.from_limbs(c.rows_read_slots(tr, lin_slots)) == [w[t] for t in lin_slots]
        proof, pi = c.rows_prove(tr, None, None)
        assert proof == want["proof"]
        assert (pi.valid_code, pi.valid_linear, pi.valid_quad) == (1, 1, 1)
        c.trace_destroy(tr)
    finally:
        c.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_hand_built_list_over_three_chunks_equals_python_integers_and_oracle(amd, where):
    """330 rows, three stage-1 chunks; targets on LINEAR / QX / QY / shipped QZ rows with 0, 1, 3, 33, 64, 65 and 700 other terms, a
    chain of 3 waves, a first-chunk target reading last-chunk rows and a LIG_ELEM_PRODUCT slot; garbage shipped at every target"""
    W = dr.world(amd)
    want = oracle(amd, 5, "expected")
    kk, packed = W.ship(amd)
    c = amd.Context(L, K, N)
    try:
        sysb = W.system.to_binding(amd)
        msgs = c.upload(packed) if where == "device" else packed
        tr, keep = c.rows_begin(kk, msgs, on_device=where == "device", generated_at=lr.GEN, elem_bytes=W.widths)
        c.rows_set_linear(tr, sysb)
        info = c.rows_set_derived(tr, sysb, W.pairs)
        assert (info.n_slots, info.n_waves) == (len(W.pairs), 3)
        root, seed1 = c.rows_commit(tr)
        got = read_targets(c, tr, W)
        assert got == [W.w[t] for t in W.targets], [t for t, g in zip(W.targets, got) if g != W.w[t]]
        assert root == want["root"] and seed1 == want["stage1_seed"]
        proof, pi = c.rows_prove(tr, None, None)
        assert proof == want["proof"]
        assert (pi.valid_code, pi.valid_linear) == (1, 1)
        # the same bytes on every run
        c.rows_restart(tr, msgs, on_device=where == "device")
        assert c.rows_commit(tr) == (root, seed1)
        assert c.rows_prove(tr, None, None)[0] == proof
        c.trace_destroy(tr)
    finally:
        c.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_restart_between_commit_and_prove_and_removing_the_list(amd, where):
    """commit(i) -> restart(i + 1) with another witness -> prove(i) -> commit(i + 1) -> prove(i + 1): the pass writes the matrix each
    commit encodes; then rows_set_derived(None): the targets hold what was shipped"""
    W1, W2 = dr.world(amd, 5), dr.world(amd, 6)
    want1, want2, plain2 = oracle(amd, 5, "expected"), oracle(amd, 6, "expected"), oracle(amd, 6, "shipped")
    assert np.array_equal(W1.kinds, W2.kinds) and np.array_equal(W1.widths, W2.widths) and W1.targets == W2.targets
    kk, p1 = W1.ship(amd)
    _, p2 = W2.ship(amd)
    c = amd.Context(L, K, N)
    try:
        s1, s2 = W1.system.to_binding(amd), W2.system.to_binding(amd)
        m1, m2 = (c.upload(p1), c.upload(p2)) if where == "device" else (p1, p2)
        dev = where == "device"
        tr, keep = c.rows_begin(kk, m1, on_device=dev, generated_at=lr.GEN, elem_bytes=W1.widths)
        c.rows_set_linear(tr, s1)
        c.rows_set_derived(tr, s1, W1.pairs)
        assert c.rows_commit(tr)[0] == want1["root"]
        c.rows_restart(tr, m2, on_device=dev)
        c.rows_set_derived(tr, s2, W2.pairs)                          # other right-hand sides: set again; in force from the NEXT commit
        assert read_targets(c, tr, W1) == [W1.w[t] for t in W1.targets]
        assert c.rows_prove(tr, None, None)[0] == want1["proof"]
        c.rows_set_linear(tr, s2)
        assert c.rows_commit(tr)[0] == want2["root"]
        assert read_targets(c, tr, W2) == [W2.w[t] for t in W2.targets]
        assert c.rows_prove(tr, None, None)[0] == want2["proof"]
        # without the list the shipped rows are committed as they are
        info = c.rows_set_derived(tr, None, None)
        assert (info.n_slots, info.n_waves) == (0, 0)
        c.rows_restart(tr, m2, on_device=dev)
        assert c.rows_commit(tr)[0] == plain2["root"]
        assert read_targets(c, tr, W2) == ol.from_limbs(np.array([W2.shipped_rows[t // L, t % L] for t in W2.targets]))
        assert c.rows_prove(tr, None, None)[0] == plain2["proof"]
        c.trace_destroy(tr)
    finally:
        c.close()


def test_diagnose_sees_the_derived_values(amd):
    """no defining constraint is ever violated; a wrong shipped INPUT of a target moves the target, and the second constraint through
    the target fails instead"""
    W = dr.world(amd)
    kk, packed = W.ship(amd)
    wrong = W.shipped_rows.copy()
    r, col = divmod(W.input_of_b, L)
    wrong[r, col, 0] ^= 1
    _, packed_wrong = W.ship(amd, wrong)
    defining = {c for _, c in W.pairs}
    c = amd.Context(L, K, N)
    try:
        sysb = W.system.to_binding(amd)
        tr, keep = c.rows_begin(kk, packed, generated_at=lr.GEN, elem_bytes=W.widths)
        c.rows_set_derived(tr, sysb, W.pairs)
        c.rows_commit(tr)
        info, lin, _ = c.rows_diagnose(tr, sysb)
        assert info.n_linear_bad == 0 and len(lin) == 0
        c.rows_prove(tr, np.zeros((len(kk), K, 8), dtype=np.uint32), None)
        c.rows_restart(tr, packed_wrong)
        c.rows_commit(tr)
        info, lin, _ = c.rows_diagnose(tr, sysb)
        bad = [int(x) for x in lin["constraint"]]
        assert bad == [W.check_of[W.t_b]] and not defining & set(bad)
        assert ol.from_limbs(c.rows_read_slots(tr, [W.t_b])) == [-int(wrong[r, col, 0]) % dr.P]      # t_b = -input, from the input as shipped
        c.trace_destroy(tr)
    finally:
        c.close()


def test_refused_lists_leave_the_trace_and_the_previous_list_as_they_were(amd):
    W = dr.world(amd)
    want, plain = oracle(amd, 5, "expected"), oracle(amd, 5, "shipped")
    kk, packed = W.ship(amd)
    l = L
    prod_row = next(r for r in range(len(W.kinds)) if W.widths[r] == amd.ELEM_PRODUCT)
    c = amd.Context(L, K, N)
    try:
        sysb = W.system.to_binding(amd)
        # a trace that never sets a list: the envelope over the rows as shipped
        tr, keep = c.rows_begin(kk, packed, generated_at=lr.GEN, elem_bytes=W.widths)
        c.rows_set_linear(tr, sysb)
        assert c.rows_commit(tr)[0] == plain["root"]
        assert c.rows_prove(tr, None, None)[0] == plain["proof"]
        c.trace_destroy(tr)

        def broken(extra_terms, pairs):
            """the world's system with one more constraint, and a list over it"""
            s = lr.System(W.system.term_begin + [W.system.term_begin[-1] + len(extra_terms)], W.system.slots + [t[0] for t in extra_terms],
                          W.system.coef_idx + [t[1] for t in extra_terms], W.system.rhs_constraint, W.system.rhs_coef, W.system.coefs, 0)
            return s.to_binding(amd), pairs

        nc = W.system.n_constraints
        free = 140 * l + 50                                          # a LINEAR slot nothing else names
        cases = [
            (sysb, W.pairs + [W.pairs[0]]),                          # a slot listed twice
            (sysb, [(W.pairs[0][0], nc)]),                           # a constraint >= n_constraints
            (sysb, [(free, W.pairs[0][1])]),                         # a target absent from its constraint
            broken([(free, lr.ONE), (free, lr.ONE)], [(free, nc)]),  # ... present twice
            broken([(free, 2), (free + 1, lr.ONE)], [(free, nc)]),   # a table index whose value is 1 (coefs[2] = 2^0)
            broken([(free, lr.ONE), (free + 1, lr.ONE)], [(free, nc), (free + 1, nc)]),      # a cycle of two through one constraint
            broken([(prod_row * l + 1, lr.NEG_ONE), (free, lr.ONE)], [(prod_row * l + 1, nc)]),          # a target on a LIG_ELEM_PRODUCT row
            broken([((prod_row - 2) * l + 1, lr.NEG_ONE), (free, lr.ONE)], [((prod_row - 2) * l + 1, nc)]),      # ... on its QX operand
            broken([((prod_row - 1) * l + 1, lr.NEG_ONE), (free, lr.ONE)], [((prod_row - 1) * l + 1, nc)]),      # ... on its QY operand
        ]
        tr, keep = c.rows_begin(kk, packed, generated_at=lr.GEN, elem_bytes=W.widths)
        c.rows_set_linear(tr, sysb)
        c.rows_set_derived(tr, sysb, W.pairs)
        for s, pairs in cases:
            with pytest.raises(amd.LigError):
                c.rows_set_derived(tr, s, pairs)
        assert c.rows_commit(tr)[0] == want["root"]                  # the previous list is still in force
        assert c.rows_prove(tr, None, None)[0] == want["proof"]
        c.trace_destroy(tr)
        # not a rows trace
        job = amd.Context.make_job(700, 330, generated_at=1)
        st = c.synth_prepare_job(job)
        with pytest.raises(amd.LigError):
            c.rows_set_derived(st, sysb, W.pairs)
        c.trace_destroy(st)
    finally:
        c.close()
