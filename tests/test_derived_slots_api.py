"""CPU: the rules of derived slots (lig_derived_check, host only -- no context, no device call) through the library, and the host planner
(ligero-prover_amd/csrc/derive_plan.hpp) as a stand-alone host program under AddressSanitizer and UBSan (tests/cpp/derive_plan_prog.cpp:
no GPU, no library, nothing loaded into python)."""
import json
import os
import subprocess

import numpy as np
import pytest

import derived_ref as dr
import hip_lib
import linear_ref as lr
from test_linear_system import mul_add_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "tests", "cpp", "derive_plan_prog.cpp")
ONE, NEG = lr.ONE, lr.NEG_ONE


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def test_derive_plan_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "derive_plan_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    assert out.strip().splitlines()[-1] == "derive plan ok", out


def test_derived_check_is_a_pure_host_entry_and_accepts_the_mul_add_list(amd):
    """every constraint 2i of the recorded guest with its eval output w as target, the QZ rows LIG_ELEM_PRODUCT: one wave.  Runs before
    any context exists (this module never makes one)."""
    d = np.load(os.path.join(GOLD, "ref_rows_mul_add_320.npz"))
    meta = json.loads(str(d["meta"]))
    l, reps = meta["l"], meta["reps"]
    kinds, vals = d["kinds"], d["vals"]
    s = mul_add_terms(reps, l, lr.witness(vals, l))
    pairs = [(4 * (i // l) * l + i % l, 2 * i) for i in range(reps)]
    widths = amd.narrowest_widths(vals, kinds, l, derive_products=True)
    assert (widths[kinds == 3] == amd.ELEM_PRODUCT).all()
    waves = amd.derived_check(s.to_binding(amd), kinds, l, pairs, widths)
    assert waves.dtype == np.uint32 and list(waves) == [1] * reps
    assert list(amd.derived_check(s.to_binding(amd), kinds | amd.ROW_DRAW_PAD, l, pairs[::-1])) == [1] * reps
    assert len(amd.derived_check(s.to_binding(amd), kinds, l, [])) == 0
    # a = the QX slot of a derived triple is an operand of the product: constraint 2i cannot define it
    with pytest.raises(amd.LigError):
        amd.derived_check(s.to_binding(amd), kinds, l, [((4 * (i // l) + 1) * l + i % l, 2 * i) for i in range(reps)], widths)


def chain_system(length, l):
    """slot i (row 0) = slot i - 1 + w[4 l + 1]: constraint i defines slot i; -> (System, pairs)"""
    tb, slots, cidx = [0], [], []
    for i in range(length):
        terms = [(4 * l + 1, ONE), (i, NEG)] + ([(i - 1, ONE)] if i else [])
        slots += [t[0] for t in terms]
        cidx += [t[1] for t in terms]
        tb.append(len(slots))
    return lr.System(tb, slots, cidx, [], [], [], 0), [(i, i) for i in range(length)]


def test_derived_check_rejects_every_broken_rule_on_its_own(amd):
    l = 320
    kinds = np.array([0, 1, 2, 3, 0], dtype=np.uint8)
    plain, prod = np.array([amd.ELEM_BIT, 1, 2, 4, 0], dtype=np.uint8), np.array([amd.ELEM_BIT, 1, 2, amd.ELEM_PRODUCT, 0], dtype=np.uint8)
    # c0: w[5] - w[4l+7] + 3 w[l+1] = p-1 (target 5)   c1: w[6] = w[5] + w[7] (target 6, -1)   c2: table index of value 1 on w[8]
    # c3: w[9] twice   c4 / c5: a cycle of two   c6 / c7 / c8: targets on the QZ / QX / QY row
    base = dict(term_begin=[0, 3, 6, 8, 11, 13, 15, 17, 19, 21],
                slots=[4 * l + 7, 5, l + 1, 5, 7, 6, 8, 10, 9, 9, 11, 12, 13, 13, 12, 3 * l + 2, 20, l + 2, 20, 2 * l + 2, 20],
                coef_idx=[NEG, ONE, 0, ONE, ONE, NEG, 2, ONE, ONE, ONE, NEG, ONE, NEG, ONE, NEG, NEG, ONE, NEG, ONE, NEG, ONE],
                rhs_constraint=[0], rhs_coef=[1], coefs=[3, dr.P - 1, 1], first_random=0)
    sysb = amd.LinearSystem.make(**base)
    assert amd.linear_check(sysb, kinds, l) == 0

    def ok(pairs, widths=None, system=sysb, kinds_=kinds):
        try:
            return list(amd.derived_check(system, kinds_, l, pairs, widths))
        except amd.LigError:
            return None

    assert ok([(5, 0), (6, 1)]) == [1, 2]                                     # the accepted base case
    assert ok([(6, 1), (5, 0)]) == [2, 1]                                     # any order
    assert ok([(5, 0), (6, 1)], prod) == [1, 2]
    assert ok([(5, 0), (5, 0)]) is None                                       # a slot listed twice
    assert ok([(5, 0), (5, 1)]) is None                                       # ... with another constraint
    assert ok([(5, 9)]) is None and ok([(5, 0xFFFFFFFF)]) is None             # a constraint >= n_constraints
    assert ok([(4, 0)]) is None                                               # a target absent from its constraint
    assert ok([(9, 3)]) is None and ok([(11, 3)]) == [1]                      # ... present twice | the other slot of that constraint
    assert ok([(8, 2)]) is None and ok([(10, 2)]) == [1]                      # a table index as the target's coefficient, even of value 1
    assert ok([(l + 1, 0)]) is None                                           # ... of another value
    assert ok([(12, 4)]) == [1] and ok([(13, 5)]) == [1] and ok([(12, 4), (13, 5)]) is None      # a cycle of two
    assert ok([(12, 4), (13, 4)]) is None                                     # a self-reference through a repeated constraint
    assert ok([(3 * l + 2, 6)], prod) is None and ok([(3 * l + 2, 6)], plain) == [1] and ok([(3 * l + 2, 6)]) == [1]      # on a LIG_ELEM_PRODUCT row
    assert ok([(l + 2, 7)], prod) is None and ok([(l + 2, 7)], plain) == [1]                      # on its QX operand row
    assert ok([(2 * l + 2, 8)], prod) is None and ok([(2 * l + 2, 8)], plain) == [1]              # on its QY operand row
    bad = amd.LinearSystem.make(**dict(base, coefs=[3, dr.P, 1]))
    assert ok([(5, 0)], system=bad) is None                                   # lig_linear_check runs first
    # waves: a chain of 16 is accepted, one of 17 refused
    s16, p16 = chain_system(amd.DERIVE_MAX_WAVES, l)
    assert ok(p16, system=s16.to_binding(amd)) == list(range(1, 17))
    assert ok(p16[::-1], system=s16.to_binding(amd)) == list(range(16, 0, -1))
    s17, p17 = chain_system(amd.DERIVE_MAX_WAVES + 1, l)
    assert ok(p17, system=s17.to_binding(amd)) is None
    assert ok(p17[:16], system=s17.to_binding(amd)) == list(range(1, 17))     # the same system with the last slot shipped


def test_waves_equal_the_python_restatement_on_a_seeded_system(amd):
    """300 derived slots on two LINEAR rows, each reading up to three slots chosen among ALL listed slots with a smaller rank (so the list
    holds chains and, once shuffled, forward references) and some that are not derived; ranks are cut so that no path exceeds 16"""
    l = 320
    kinds = np.array([0, 0, 0, 1, 2, 3], dtype=np.uint8)
    rng = np.random.default_rng(22)
    order = rng.permutation(2 * l)[:300]                                      # slot of rank i
    tb, slots, cidx, pairs, level = [0], [], [], [], {}
    for i, t in enumerate(order):
        deps = [int(order[j]) for j in rng.integers(0, i, int(rng.integers(0, 4)))] if i else []
        deps = [d for d in deps if level[d] < 16]
        deps = deps if all(level[d] < 15 for d in deps) else deps[:1]
        level[int(t)] = 1 + max([level[d] for d in deps], default=0)
        terms = [(d, ONE) for d in deps] + [(int(t), NEG if i % 2 else ONE)] + [(2 * l + int(rng.integers(0, l)), NEG)]
        slots += [x[0] for x in terms]
        cidx += [x[1] for x in terms]
        tb.append(len(slots))
        pairs.append((int(t), i))
    s = lr.System(tb, slots, cidx, [], [], [], 0)
    assert max(level.values()) > 5
    rng.shuffle(pairs)
    want = dr.waves_of(s, pairs)
    assert want == level
    got = amd.derived_check(s.to_binding(amd), kinds, l, pairs)
    assert list(got) == [want[t] for t, _ in pairs]
    W = dr.world(amd)
    assert list(amd.derived_check(W.system.to_binding(amd), W.kinds, dr.L, W.pairs, W.widths)) == [W.waves[t] for t, _ in W.pairs]
