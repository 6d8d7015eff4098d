"""CPU: product entries of derived slots ((slot, DERIVED_PRODUCT)) without a GPU -- the host planner as a stand-alone host program under
AddressSanitizer and UBSan (tests/cpp/derive_product_plan_prog.cpp: no library, nothing loaded into python), the rules through the
host-only lig_derived_check, and lig_derived_shard_count against the Python restatement of tests/derived_product_ref.py at W = 2 and 3."""
import os
import subprocess

import numpy as np
import pytest

import derived_product_ref as dpr
import hip_lib
import linear_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "derive_product_plan_prog.cpp")
ONE, NEG = lr.ONE, lr.NEG_ONE
L = 320


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def test_product_plan_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "derive_product_plan_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    assert out.strip().splitlines()[-1] == "derive product plan ok", out


# row 0 LINEAR | 1 2 3 triple A, z derived | 4 5 6 triple B, z derived | 7 8 9 triple C, z shipped | 10 LINEAR
KINDS = np.array([0, 1, 2, 3, 1, 2, 3, 1, 2, 3, 0], dtype=np.uint8)


def at(row, col):
    return row * L + col


def small_system():
    """the constraints of tests/cpp/derive_product_plan_prog.cpp at l = 320 -> (System, names)"""
    cons = dict(
        cX=[(0, ONE), (at(1, 0), NEG), (1, ONE)], cT=[(at(3, 0), ONE), (2, ONE), (at(5, 0), NEG)], cF=[(at(10, 0), NEG), (at(6, 0), ONE), (3, ONE)],
        cX1=[(at(1, 1), ONE), (4, NEG)], cY1=[(at(1, 1), ONE), (5, ONE), (at(2, 1), NEG)],
        cZ=[(at(3, 2), NEG), (6, ONE)], cCyc=[(at(1, 2), NEG), (at(3, 2), ONE), (0, ONE)], cXC=[(at(7, 3), NEG), (7, ONE)])
    tb, slots, cidx, names = [0], [], [], {}
    for name, terms in cons.items():
        names[name] = len(tb) - 1
        slots += [s for s, _ in terms]
        cidx += [c for _, c in terms]
        tb.append(len(slots))
    return lr.System(tb, slots, cidx, [], [], [], 0), names


def widths_of(amd):
    return np.array([amd.ELEM_BIT, 2, amd.ELEM_BIT, amd.ELEM_PRODUCT, 2, 2, amd.ELEM_PRODUCT, 2, 2, 4, 0], dtype=np.uint8)


def test_constant_and_accepted_lists_with_their_exact_waves(amd):
    assert amd.DERIVED_PRODUCT == 0xFFFFFFFF == dpr.PRODUCT
    PR = amd.DERIVED_PRODUCT
    s, c = small_system()
    sysb, eb = s.to_binding(amd), widths_of(amd)
    assert amd.linear_check(sysb, KINDS, L) == 0
    waves = lambda pairs: list(amd.derived_check(sysb, KINDS, L, pairs, eb))
    # x derived -> z (2) -> a linear target reading z (3), the y operand of triple B -> its z (4) -> a last linear target (5)
    chain = [(at(1, 0), c["cX"]), (at(3, 0), PR), (at(5, 0), c["cT"]), (at(6, 0), PR), (at(10, 0), c["cF"])]
    assert waves(chain) == [1, 2, 3, 4, 5]
    assert waves(chain[::-1]) == [5, 4, 3, 2, 1]
    # both operands derived in different waves; a product entry with no derived operand
    both = [(at(3, 1), PR), (at(2, 1), c["cY1"]), (at(1, 1), c["cX1"])]
    assert waves(both) == [3, 2, 1]
    assert waves([(at(3, 2), PR)]) == [1] and waves([(at(6, 7), PR), (at(3, 2), PR)]) == [1, 1]
    # any order: the wave of a slot does not depend on the order of the list
    every = chain + both + [(at(3, 2), PR)]
    want = dict(zip([t for t, _ in every], waves(every)))
    assert want == dpr.waves_of(s, every, L)
    rng = np.random.default_rng(3)
    for _ in range(5):
        order = [every[i] for i in rng.permutation(len(every))]
        assert waves(order) == [want[t] for t, _ in order]
    # ROW_DRAW_PAD on the kinds changes nothing
    assert list(amd.derived_check(sysb, KINDS | amd.ROW_DRAW_PAD, L, every, eb)) == [want[t] for t, _ in every]


def alternating_chain(length):
    """x_j = z_(j - 1) + w[0] on triple j % 2, column j // 2; z_j its product entry; entry 17 a LINEAR target that reads z_7"""
    tb, slots, cidx, pairs = [0], [], [], []
    for j in range(8):
        xrow, col = (4 if j % 2 else 1), j // 2
        terms = [(at(xrow, col), NEG), (0, ONE)] + ([(pairs[-1][0], ONE)] if j else [])
        slots += [t[0] for t in terms]
        cidx += [t[1] for t in terms]
        tb.append(len(slots))
        pairs += [(at(xrow, col), j), (at(xrow + 2, col), dpr.PRODUCT)]
    slots += [at(10, 0), pairs[-1][0]]
    cidx += [NEG, ONE]
    tb.append(len(slots))
    pairs.append((at(10, 0), 8))
    return lr.System(tb, slots, cidx, [], [], [], 0), pairs[:length]


def test_refusals_each_on_its_own_and_the_wave_limit(amd):
    PR = amd.DERIVED_PRODUCT
    s, c = small_system()
    sysb, eb = s.to_binding(amd), widths_of(amd)

    def ok(pairs, widths=eb, system=sysb):
        try:
            return list(amd.derived_check(system, KINDS, L, pairs, widths))
        except amd.LigError:
            return None

    assert ok([(at(3, 2), PR)]) == [1]
    assert ok([(at(0, 2), PR)]) is None and ok([(at(10, 2), PR)]) is None     # a product entry on a LINEAR slot
    assert ok([(at(1, 2), PR)]) is None and ok([(at(2, 2), PR)]) is None      # ... on an operand row
    assert ok([(at(9, 2), PR)]) is None                                       # on the shipped (non-PRODUCT) QZ row
    assert ok([(at(3, 2), PR)], None) is None                                 # elem_bytes == NULL
    assert ok([(at(3, 2), PR), (at(3, 2), PR)]) is None                       # listed twice
    assert ok([(at(3, 2), PR), (at(3, 2), c["cZ"])]) is None and ok([(at(3, 2), c["cZ"]), (at(3, 2), PR)]) is None      # with a linear entry of the slot
    assert ok([(at(3, 2), c["cZ"])]) is None and ok([(at(3, 2), c["cZ"])], None) == [1]      # a linear target on the product row: as ever
    assert ok([(at(1, 0), c["cX"])]) is None and ok([(at(1, 0), c["cX"]), (at(3, 0), PR)]) == [1, 2]      # an operand target without | with its product entry
    assert ok([(at(1, 0), c["cX"]), (at(3, 1), PR)]) is None and ok([(at(1, 0), c["cX"]), (at(6, 0), PR)]) is None      # another column, another triple
    assert ok([(at(2, 1), c["cY1"])]) is None and ok([(at(2, 1), c["cY1"]), (at(3, 1), PR)]) == [1, 2]
    assert ok([(at(7, 3), c["cXC"])]) == [1]                                  # the x of a triple whose z is shipped needs none
    assert ok([(at(1, 2), c["cCyc"]), (at(3, 2), PR)]) is None                # a cycle through a product
    # a chain alternating linear and product entries: 16 accepted (forwards and backwards), 17 refused
    s17, p17 = alternating_chain(17)
    b17 = s17.to_binding(amd)
    assert ok(p17[:16], system=b17) == list(range(1, 17))
    assert ok(p17[:16][::-1], system=b17) == list(range(16, 0, -1))
    assert ok(p17, system=b17) is None
    assert ok(p17[1:], system=b17) == list(range(1, 17))                      # x_0 shipped: the chain starts at z_0
    # lig_derived_shard_count decides alike, at every rank
    for pairs, widths in [([(at(3, 2), PR)], eb), ([(at(3, 2), PR)], None), ([(at(9, 2), PR)], eb), ([(at(1, 0), c["cX"])], eb),
                          ([(at(1, 0), c["cX"]), (at(3, 0), PR)], eb), ([(at(1, 2), c["cCyc"]), (at(3, 2), PR)], eb)]:
        for rank in (0, 1):
            try:
                amd.derived_shard_count(sysb, KINDS, L, pairs, widths, rank, 2)
                counted = True
            except amd.LigError:
                counted = False
            assert counted == (ok(pairs, widths) is not None), (pairs, rank)
    one = amd.derived_shard_count(sysb, KINDS, L, [(at(1, 0), c["cX"]), (at(3, 0), PR)], eb, 0, 1).as_dict()
    assert one == dict(n_slots=2, n_terms=4, n_waves=2, n_exchanges=0, local_targets=2, local_terms=4, imported_terms=0, imports=0, exports=0, exchange_bytes=0)


def test_world_waves_equal_the_python_restatement(amd):
    W = dpr.world(amd)
    got = amd.derived_check(W.system.to_binding(amd), W.kinds, L, W.pairs, W.widths)
    assert list(got) == [W.waves[t] for t, _ in W.pairs] and max(got) == 5


@pytest.mark.parametrize("world", [2, 3])
def test_shard_count_equals_the_python_restatement(amd, world):
    """the list of derived_product_ref placed against the deal: product entries never import, the re-formed z that another rank reads is in
    the block of the reader's wave, a product entry counts as one target and two local terms on the rank that holds its triple"""
    W = dpr.world(amd, world_size=world)
    sysb = W.system.to_binding(amd)
    got = [amd.derived_shard_count(sysb, W.kinds, L, W.pairs, W.widths, q, world).as_dict() for q in range(world)]
    want = [dpr.shard_info(W.system, W.pairs, W.owner, L, q, world) for q in range(world)]
    assert got == [x[0] for x in want]
    E = want[0][1]
    reads = dpr.reads_of(W.system, W.pairs, L)
    products = [t for t, c in W.pairs if c == dpr.PRODUCT]
    assert all(W.owner[s // L] == W.owner[t // L] for t in products for s in reads[t])          # the reference's deal never splits a triple ...
    # ... and the LIBRARY never imports for a product entry: a list of product entries alone (their operands as shipped) on every triple
    # whose z is derived has, on every rank, no imported term, no import, no export and no exchange, and two local terms per entry
    alone = [(r * L + 40 + i, dpr.PRODUCT) for i, r in enumerate(np.flatnonzero(W.widths == amd.ELEM_PRODUCT))]
    lone = [amd.derived_shard_count(sysb, W.kinds, L, alone, W.widths, q, world).as_dict() for q in range(world)]
    for q, x in enumerate(lone):
        assert x == dict(n_slots=len(alone), n_terms=2 * len(alone), n_waves=1, n_exchanges=0, local_targets=int(sum(W.owner[t // L] == q for t, _ in alone)),
                         local_terms=2 * int(sum(W.owner[t // L] == q for t, _ in alone)), imported_terms=0, imports=0, exports=0, exchange_bytes=0)
    assert sum(x["local_targets"] for x in lone) == len(alone) == 30 and sum(1 for x in lone if x["local_targets"]) >= 2
    assert W.z_far in E[2][W.owner[W.z_far // L]] and not any(W.z_far in v for w, e in enumerate(E) if w != 2 for v in e)
    assert sum(x["local_targets"] for x in got) == len(W.pairs) == got[0]["n_slots"]
    assert sum(x["local_terms"] + x["imported_terms"] for x in got) == got[0]["n_terms"] == sum(len(v) for v in reads.values())
    assert got[0]["n_waves"] == 5 and got[0]["n_exchanges"] >= 2 and sum(x["imported_terms"] for x in got) >= 3
    q = int(W.owner[W.z_far // L])
    only_products = [t for t in products if W.owner[t // L] == q]
    assert got[q]["local_terms"] >= 2 * len(only_products)
