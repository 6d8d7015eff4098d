"""CPU: the sparse linear-system format (lig_linear_check, host only -- no device call) and the Python restatement of
Rn / const_sum (tests/linear_ref.py) against the numbers the REFERENCE's witness_manager produced.

tests/golden/ref_rows_mul_add_320.npz holds the randomness rows and the constant sum the reference recorded for the guest of
oracle/ref_backend.cpp section 3 (`reps` times: a, b witnesses, w = eval(a * b + a - 3), assert_const(w, expect)).  Its term list is
restated below; this is where sign conventions and draw order are pinned to the reference rather than to a reading of it."""
import json
import os

import numpy as np
import pytest

import hip_lib
import linear_ref as lr
import oracle_lib as ol

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P = ol.P


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def small_trace(l=320, k=512, n=2048):
    return lr.build_trace(l, k, n, 3 * l + 17, l + 9)


def test_check_accepts_the_systems_of_the_gpu_tests(amd):
    l = 320
    kinds, rows, _ = small_trace()
    for nc, first in ((30000, 0), (70000, 1000)):
        s = lr.make_system(kinds, rows, l, nc, first, seed=nc)
        assert lr.holds(s, rows, l)
        assert amd.linear_check(s.to_binding(amd), kinds, l) == 0
        assert amd.linear_check(s.to_binding(amd), kinds | amd.ROW_DRAW_PAD, l) == 0
        cnt = np.bincount(np.array(s.slots), minlength=len(kinds) * l)
        assert cnt[s.hot_slot] >= 20000 and cnt[s.single_slot] == 1 and (cnt == 2).any() and (cnt == 0).any() and (cnt > 3).any()
        assert not cnt[s.untouched_row * l:(s.untouched_row + 1) * l].any()
        assert any(s.term_begin[c] == s.term_begin[c + 1] for c in range(nc))
        assert {0, 1, 2, lr.ONE, lr.NEG_ONE} <= set(s.coef_idx)
    e = lr.make_equality_system(kinds, l, 0)
    assert e.n_constraints > 10 and lr.holds(e, rows, l) and not e.coefs and not e.rhs_constraint
    assert amd.linear_check(e.to_binding(amd), kinds, l) == 0
    # an empty system is a system
    assert amd.linear_check(amd.LinearSystem.make([0], [], []), kinds, l) == 0


def test_check_rejects_every_broken_rule_on_its_own(amd):
    l = 320
    kinds = np.array([0, 1, 2, 3, 0], dtype=np.uint8)
    base = dict(term_begin=[0, 2, 2, 3], slots=[5, 4 * l + 7, l + 1], coef_idx=[0, lr.ONE, lr.NEG_ONE], rhs_constraint=[0, 2], rhs_coef=[1, 0],
                coefs=[3, P - 1], first_random=0)

    def check(kinds_=kinds, l_=l, **kw):
        d = dict(base)
        d.update(kw)
        return amd.linear_check(amd.LinearSystem.make(**d), kinds_, l_)

    assert check() == 0
    assert check(slots=[5, 5 * l, l + 1]) == -1                               # a slot beyond the rows
    assert check(slots=[5, 5 * l - 1, l + 1]) == 0                            # ... the last slot is inside
    batch = np.array([amd.ROW_KINDS["INIT"], 1, 2, 3, 0], dtype=np.uint8)
    assert check(kinds_=batch) == -1                                          # a slot on a batch-kind row
    assert check(kinds_=batch, slots=[l + 5, 4 * l + 7, l + 1]) == 0
    many = np.zeros((1 << 32) // l + 1, dtype=np.uint8)
    assert check(kinds_=many) == -1                                           # rows * l >= 2^32
    assert check(kinds_=many[:-1]) == 0
    assert check(coef_idx=[2, lr.ONE, lr.NEG_ONE]) == -1                      # a coefficient index == n_coefs
    assert check(rhs_coef=[1, 2]) == -1
    assert check(coefs=[3, P]) == -1                                          # a non-canonical table entry
    assert check(term_begin=[0, 2, 1, 3]) == -1                               # term_begin decreasing
    assert check(term_begin=[0, 2, 2, 2]) == -1                               # ... not ending at n_terms
    assert check(term_begin=[1, 2, 2, 3]) == -1                               # ... not starting at 0
    assert check(rhs_constraint=[2, 0]) == -1                                 # rhs_constraint unsorted
    assert check(rhs_constraint=[0, 0]) == -1
    assert check(rhs_constraint=[0, 3]) == -1                                 # ... >= n_constraints
    s = amd.LinearSystem.make(**base)
    s.struct_bytes -= 8
    assert amd.linear_check(s, kinds, l) == -1                                # a short struct_bytes


def mul_add_terms(reps, l, w):
    """The constraints the guest raises, in draw order, on the slots the commit order gives.  Repetition i lives in row block
    g = i // l at column i % l: w in the LINEAR row 4g, a in the QX row 4g + 1, b in 4g + 2, a * b in the QZ row 4g + 3.
      constraint 2i      eval(a * b + a - 3) = w:    a * b + a - w = 3
      constraint 2i + 1  assert_const(w, expect):    w = expect
    The table holds 3 and the public values `expect` (read from the recorded witness: the statement is about them)."""
    term_begin, slots, cidx, rhs_c, rhs_b, coefs = [0], [], [], [], [], [3]
    for i in range(reps):
        g, col = divmod(i, l)
        sw, sa, sz = 4 * g * l + col, (4 * g + 1) * l + col, (4 * g + 3) * l + col
        slots += [sz, sa, sw]
        cidx += [lr.ONE, lr.ONE, lr.NEG_ONE]
        term_begin.append(len(slots))
        rhs_c.append(2 * i)
        rhs_b.append(0)
        slots.append(sw)
        cidx.append(lr.ONE)
        term_begin.append(len(slots))
        rhs_c.append(2 * i + 1)
        rhs_b.append(len(coefs))
        coefs.append(w[sw])
    return lr.System(term_begin, slots, cidx, rhs_c, rhs_b, coefs, 0)


def test_restatement_equals_the_reference_recording_mul_add(amd):
    d = np.load(os.path.join(GOLD, "ref_rows_mul_add_320.npz"))
    meta = json.loads(str(d["meta"]))
    l, k, reps = meta["l"], meta["k"], meta["reps"]
    kinds, vals, rands = d["kinds"], d["vals"], d["rands"]
    assert not rands[:, l:].any()                                             # randomness only on the data slots
    s = mul_add_terms(reps, l, lr.witness(vals, l))
    assert lr.holds(s, vals, l)
    assert amd.linear_check(s.to_binding(amd), kinds, l) == 0
    rn, cs = lr.expected(s, bytes.fromhex(meta["oracle_stage1_seed"]), len(kinds), l, k)
    assert np.array_equal(rn, rands)                                          # every slot, zeros included
    assert cs == d["constsum"].tobytes()
