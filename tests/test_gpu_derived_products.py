"""GPU: product entries of derived slots ((slot, DERIVED_PRODUCT) in the list of lig_rows_set_derived) -- column i of a LIG_ELEM_PRODUCT
row re-formed from the expanded matrix in wave order, so that an eval output may be a multiplication operand and a product may feed the
next eval.  Every expected value is a Python integer of tests/derived_product_ref.py, every expected envelope the oracle's prover over
rows that carry those integers; never the path under test.  All shapes are l = 320, k = 512, n = 2048."""
import os
import subprocess

import numpy as np
import pytest

import derived_product_ref as dpr
import hip_lib
import linear_ref as lr
import multirank as mr
import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, K, N = dpr.L, dpr.K, dpr.N
_oracle = {}


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def oracle(amd):
    """the oracle's envelope over the world's expected rows, computed once"""
    if "expected" not in _oracle:
        W = dpr.world(amd)
        _oracle["expected"] = W.oracle(W.expected_rows)
    return _oracle["expected"]


def begin(amd, c, W, packed, where="host"):
    kk, _ = W.ship(amd)
    msgs = c.upload(packed) if where == "device" else packed
    tr, keep = c.rows_begin(kk, msgs, on_device=where == "device", generated_at=lr.GEN, elem_bytes=W.widths, wide_per_row=W.wide)
    return tr, msgs, keep


def read_listed(c, tr, W):
    return ol.from_limbs(c.rows_read_slots(tr, W.listed))


@pytest.mark.parametrize("where", ["host", "device"])
def test_products_of_derived_operands_equal_python_integers_and_oracle(amd, where):
    """330 rows, three chunks: a full-width derived x on a bit row, both operands derived, only y derived, the other operand a record of a
    mixed row, (p - 1)(p - 1), 0 * x, a last-chunk triple whose x reads first-chunk rows and a first-chunk target that reads its z, the five
    waves x -> z -> y' -> z' -> v, a product entry of shipped operands; garbage shipped at every linear target"""
    W = dpr.world(amd)
    want = oracle(amd)
    assert want["valid"] == [1, 1, 1]
    _, packed = W.ship(amd)
    c = amd.Context(L, K, N)
    try:
        sysb = W.system.to_binding(amd)
        tr, msgs, keep = begin(amd, c, W, packed, where)
        c.rows_set_linear(tr, sysb)
        info = c.rows_set_derived(tr, sysb, W.pairs)
        n_products = sum(1 for _, cn in W.pairs if cn == amd.DERIVED_PRODUCT)
        reads = dpr.reads_of(W.system, W.pairs, L)
        assert (info.n_slots, info.n_waves, info.n_terms) == (len(W.pairs), 5, sum(len(v) for v in reads.values()))
        assert n_products == 10
        root, seed1 = c.rows_commit(tr)
        got = read_listed(c, tr, W)
        assert got == [W.w[t] for t in W.listed], [t for t, g in zip(W.listed, got) if g != W.w[t]]
        assert root == want["root"] and seed1 == want["stage1_seed"]
        proof, pi = c.rows_prove(tr, None, None)
        assert proof == want["proof"]
        assert (pi.valid_code, pi.valid_linear, pi.valid_quad) == (1, 1, 1)
        # the same bytes on every run
        c.rows_restart(tr, msgs, on_device=where == "device")
        assert c.rows_commit(tr) == (root, seed1)
        assert c.rows_prove(tr, None, None)[0] == proof
        c.trace_destroy(tr)
    finally:
        c.close()


def test_readers_see_the_reformed_products(amd):
    """diagnose: nothing violated with the list set; one shipped input of a derived x flipped: x and its re-formed z move, so the CHECK
    constraints through them fail -- no defining constraint and no quadratic term.  explain / explain_slots return the Python integers"""
    W = dpr.world(amd)
    _, packed = W.ship(amd)
    wrong = W.shipped_rows.copy()
    r, col = divmod(W.input_of_a, L)
    wrong[r, col, 0] ^= 1
    _, packed_wrong = W.ship(amd, wrong)
    defining = {cn for _, cn in W.pairs if cn != amd.DERIVED_PRODUCT}
    c = amd.Context(L, K, N)
    try:
        sysb = W.system.to_binding(amd)
        tr, msgs, keep = begin(amd, c, W, packed)
        c.rows_set_linear(tr, sysb)
        c.rows_set_derived(tr, sysb, W.pairs)
        c.rows_commit(tr)
        for info, lin, quad in (c.rows_diagnose(tr, sysb), c.rows_diagnose_attached(tr)):
            assert (info.n_linear_bad, info.n_quad_bad, len(lin), len(quad)) == (0, 0, 0, 0)
        products = [W.z_a, W.z_d, W.z_e, W.c4]
        checks = sorted(W.check_of[t] for t in products)
        for _, cons, terms in (c.rows_explain(tr, sysb, checks), c.rows_explain_attached(tr, checks)):
            assert not cons["residual"].any()
            by = {(int(t["constraint"]), int(t["slot"])): ol.from_limbs(np.frombuffer(t["value"].tobytes(), dtype=np.uint32).reshape(1, 8))[0] for t in terms}
            for t in products:
                assert by[W.check_of[t], t] == W.w[t]
        asked = sorted([W.z_b, W.z_f, W.c2])
        for _, srec, sterms in (c.rows_explain_slots(tr, sysb, asked), c.rows_explain_slots_attached(tr, asked)):
            assert [int(s) for s in srec["slot"]] == asked and not sterms["residual"].any()
            assert ol.from_limbs(np.frombuffer(srec["value"].tobytes(), dtype=np.uint32).reshape(-1, 8)) == [W.w[t] for t in asked]
        c.rows_prove(tr, None, None)
        c.rows_restart(tr, packed_wrong)
        c.rows_commit(tr)
        info, lin, quad = c.rows_diagnose(tr, sysb)
        bad = [int(x) for x in lin["constraint"]]
        assert W.check_of[W.z_a] in bad and bad == sorted([W.check_of[W.x_a], W.check_of[W.z_a]])
        assert not defining & set(bad) and (info.n_linear_bad, info.n_quad_bad, len(quad)) == (2, 0, 0)
        moved = (W.w[W.x_a] + dpr.P + (W.system.coefs[1] if wrong[r, col, 0] & 1 else -W.system.coefs[1])) % dpr.P      # x_a = FULL * input + ...; y = 1
        assert ol.from_limbs(c.rows_read_slots(tr, [W.x_a, W.z_a])) == [moved, moved]
        c.trace_destroy(tr)
    finally:
        c.close()


def test_refused_lists_leave_the_previous_list_in_force(amd):
    W = dpr.world(amd)
    want = oracle(amd)
    _, packed = W.ship(amd)
    l, PR = L, amd.DERIVED_PRODUCT
    by_slot = dict(W.pairs)
    shipped_qz = next(r for r in range(len(W.kinds)) if W.kinds[r] == 3 and W.widths[r] != amd.ELEM_PRODUCT)
    without = lambda *gone: [p for p in W.pairs if p[0] not in gone]
    # x_a = z_a + ...: a cycle through the product
    cyc = lr.System(W.system.term_begin + [W.system.term_begin[-1] + 2], W.system.slots + [W.x_a, W.z_a], W.system.coef_idx + [lr.NEG_ONE, lr.ONE],
                    W.system.rhs_constraint, W.system.rhs_coef, W.system.coefs, 0)
    # z_a = w[free]: a constraint that could define z_a as a linear target, were its row not LIG_ELEM_PRODUCT
    lin_z = lr.System(W.system.term_begin + [W.system.term_begin[-1] + 2], W.system.slots + [W.z_a, 140 * l + 50], W.system.coef_idx + [lr.NEG_ONE, lr.ONE],
                      W.system.rhs_constraint, W.system.rhs_coef, W.system.coefs, 0)
    c = amd.Context(L, K, N)
    try:
        sysb = W.system.to_binding(amd)
        cases = [
            (sysb, W.pairs + [(5 * l + 50, PR)]),                        # a product entry on a LINEAR slot
            (sysb, W.pairs + [(shipped_qz * l + 50, PR)]),               # ... on a shipped QZ row
            (sysb, W.pairs + [(W.z_a, PR)]),                             # ... listed twice
            (sysb, without(W.z_a)),                                      # an operand target without its product entry
            (sysb, without(W.z_b)),                                      # ... with both operands derived
            (sysb, without(W.z_a) + [(W.z_a, by_slot[W.x_a])]),          # a linear entry on the product slot
            (sysb, W.pairs + [(W.z_a, W.check_of[W.z_a])]),              # a product entry plus a linear entry of the same slot ...
            (sysb, [(W.z_a, W.check_of[W.z_a])] + W.pairs),              # ... in either order
            (lin_z.to_binding(amd), W.pairs + [(W.z_a, W.system.n_constraints)]),           # ... the linear one well-formed on its own (-1, once)
            (lin_z.to_binding(amd), [(W.z_a, W.system.n_constraints)] + W.pairs),
            (cyc.to_binding(amd), without(W.x_a) + [(W.x_a, W.system.n_constraints)]),      # a cycle through a product
        ]
        tr, msgs, keep = begin(amd, c, W, packed)
        c.rows_set_linear(tr, sysb)
        c.rows_set_derived(tr, sysb, W.pairs)
        for s, pairs in cases:
            with pytest.raises(amd.LigError):
                c.rows_set_derived(tr, s, pairs)
        assert c.rows_commit(tr)[0] == want["root"]                      # the previous list is still in force
        assert c.rows_prove(tr, None, None)[0] == want["proof"]
        c.trace_destroy(tr)
        # a trace without elem_bytes has no LIG_ELEM_PRODUCT row: every product entry is refused
        kk, _ = W.ship(amd)
        tr, keep = c.rows_begin(kk, W.expected_rows, generated_at=lr.GEN)
        with pytest.raises(amd.LigError):
            c.rows_set_derived(tr, sysb, [(W.z_plain, PR)])
        c.trace_destroy(tr)
    finally:
        c.close()


def test_row_batcher_records_a_product_of_an_eval_output(tmp_path):
    """t = eval(a + b); u = t * c; v = eval(u + d) through hip_row_batcher::set_derived_slots and product_entry: what is checked is
    written out in tests/cpp/derived_products_batcher_prog.cpp"""
    mod = hip_lib.load()
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    odir = os.path.join(ROOT, "oracle")
    ol.build()
    src, exe = os.path.join(ROOT, "tests", "cpp", "derived_products_batcher_prog.cpp"), str(tmp_path / "derived_products_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    p = subprocess.run([exe], capture_output=True, timeout=300)
    assert p.returncode == 0, (p.stdout.decode()[-3000:], p.stderr.decode()[-3000:])
    o = mr.last_json(p.stdout.decode())
    assert o == dict(values_equal=True, valid=True, equals_oracle=True, entries=120), o
