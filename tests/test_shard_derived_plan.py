"""CPU: derived slots on a rows shard without a GPU -- the per-rank program and the exchange schedule (plan_derived_shard,
ligero-prover_amd/csrc/derive_plan.hpp) as a stand-alone host program under AddressSanitizer and UBSan
(tests/cpp/derive_shard_plan_prog.cpp: no library, nothing loaded into python), and the host-only lig_derived_shard_count against the
Python restatement of tests/shard_derived_ref.py (shard_rows_plan, derived_ref.waves_of)."""
import os
import subprocess

import numpy as np
import pytest

import derived_ref as dr
import hip_lib
import linear_ref as lr
import shard_derived_ref as sdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "derive_shard_plan_prog.cpp")
ONE, NEG = lr.ONE, lr.NEG_ONE
L = 320


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def test_shard_plan_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "derive_shard_plan_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    assert out.strip().splitlines()[-1] == "derive shard plan ok", out


def seeded(row_local):
    """72 LINEAR rows and 8 triples; 400 derived slots (columns < 200) on seeded LINEAR rows, each reading up to three listed slots of a
    smaller rank and two slots that are not derived (columns >= 200) -- on any row, or (row_local) the whole constraint on the target's row
    -> (kinds, System, pairs)"""
    kinds = np.array([0] * 72 + [1, 2, 3] * 8, dtype=np.uint8)
    rng = np.random.default_rng(31)
    where = rng.permutation(72 * 200)[:400]
    tb, slots, cidx, pairs, level, slot_of = [0], [], [], [], {}, []
    for i, x in enumerate(where):
        row, col = int(x) // 200, int(x) % 200
        t = row * L + col
        prior = [s for s in slot_of if not row_local or s // L == row]
        deps = [prior[int(j)] for j in rng.integers(0, len(prior), int(rng.integers(0, 4)))] if prior else []
        deps = [d for d in dict.fromkeys(deps) if level[d] < 16]
        deps = deps if all(level[d] < 15 for d in deps) else deps[:1]
        level[t] = 1 + max([level[d] for d in deps], default=0)
        plain = [(row if row_local else int(rng.integers(0, len(kinds)))) * L + int(rng.integers(200, L)) for _ in range(2)]
        terms = [(d, ONE) for d in deps] + [(t, NEG if i % 2 else ONE)] + [(s, NEG) for s in plain]
        slots += [s for s, _ in terms]
        cidx += [c for _, c in terms]
        tb.append(len(slots))
        pairs.append((t, i))
        slot_of.append(t)
    rng.shuffle(pairs)
    return kinds, lr.System(tb, slots, cidx, [], [], [], 0), pairs


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_count_equals_the_python_restatement_on_a_seeded_system(amd, world):
    kinds, s, pairs = seeded(row_local=False)
    sysb = s.to_binding(amd)
    rounds, b = amd.shard_rows_plan(kinds, world)
    owner = sdr.owner_of(b, world, len(kinds))
    for q in range(world):
        assert sorted(np.flatnonzero(owner == q)) == sorted(amd.local_rows_of(b, q, world))
    got = [amd.derived_shard_count(sysb, kinds, L, pairs, None, q, world).as_dict() for q in range(world)]
    want = [sdr.shard_info(s, pairs, owner, L, q, world)[0] for q in range(world)]
    assert got == want
    assert want[0]["n_waves"] > 3 and (world == 1 or (want[0]["n_exchanges"] > 1 and sum(x["imported_terms"] for x in want) > 100))
    assert sum(x["local_targets"] for x in got) == got[0]["n_slots"] == len(pairs)
    assert sum(x["local_terms"] + x["imported_terms"] for x in got) == got[0]["n_terms"]
    assert len({(x["n_exchanges"], x["exchange_bytes"], x["n_waves"]) for x in got}) == 1      # the schedule is the same on every rank
    if world == 1:
        assert (got[0]["n_exchanges"], got[0]["exchange_bytes"], got[0]["imports"], got[0]["exports"]) == (0, 0, 0, 0)
    # widths given: the same numbers (no row is LIG_ELEM_PRODUCT)
    assert amd.derived_shard_count(sysb, kinds, L, pairs, np.full(len(kinds), 32, dtype=np.uint8), world - 1, world).as_dict() == want[world - 1]


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_row_local_list_has_no_exchange(amd, world):
    kinds, s, pairs = seeded(row_local=True)
    rounds, b = amd.shard_rows_plan(kinds, world)
    owner = sdr.owner_of(b, world, len(kinds))
    for q in range(world):
        got = amd.derived_shard_count(s.to_binding(amd), kinds, L, pairs, None, q, world).as_dict()
        assert got == sdr.shard_info(s, pairs, owner, L, q, world)[0]
        assert got["n_waves"] > 1 and (got["n_exchanges"], got["exchange_bytes"], got["imports"], got["exports"], got["imported_terms"]) == (0, 0, 0, 0, 0)


def test_every_refusal_of_derived_check_is_refused_here_too(amd):
    """the lists of tests/test_derived_slots_api.py, accepted and refused: lig_derived_shard_count decides as lig_derived_check does, at
    every rank of W = 2; and its own argument errors"""
    l = L
    kinds = np.array([0, 1, 2, 3, 0], dtype=np.uint8)
    plain, prod = np.array([amd.ELEM_BIT, 1, 2, 4, 0], dtype=np.uint8), np.array([amd.ELEM_BIT, 1, 2, amd.ELEM_PRODUCT, 0], dtype=np.uint8)
    base = dict(term_begin=[0, 3, 6, 8, 11, 13, 15, 17, 19, 21],
                slots=[4 * l + 7, 5, l + 1, 5, 7, 6, 8, 10, 9, 9, 11, 12, 13, 13, 12, 3 * l + 2, 20, l + 2, 20, 2 * l + 2, 20],
                coef_idx=[NEG, ONE, 0, ONE, ONE, NEG, 2, ONE, ONE, ONE, NEG, ONE, NEG, ONE, NEG, NEG, ONE, NEG, ONE, NEG, ONE],
                rhs_constraint=[0], rhs_coef=[1], coefs=[3, dr.P - 1, 1], first_random=0)
    sysb = amd.LinearSystem.make(**base)
    bad = amd.LinearSystem.make(**dict(base, coefs=[3, dr.P, 1]))

    def check(pairs, widths, system):
        try:
            amd.derived_check(system, kinds, l, pairs, widths)
            return True
        except amd.LigError:
            return False

    def count(pairs, widths, system, rank=0, world=2):
        try:
            return amd.derived_shard_count(system, kinds, l, pairs, widths, rank, world)
        except amd.LigError:
            return None

    cases = [([(5, 0), (6, 1)], None), ([(6, 1), (5, 0)], None), ([(5, 0), (6, 1)], prod), ([(5, 0), (5, 0)], None), ([(5, 0), (5, 1)], None),
             ([(5, 9)], None), ([(5, 0xFFFFFFFF)], None), ([(4, 0)], None), ([(9, 3)], None), ([(11, 3)], None), ([(8, 2)], None), ([(10, 2)], None),
             ([(l + 1, 0)], None), ([(12, 4)], None), ([(13, 5)], None), ([(12, 4), (13, 5)], None), ([(12, 4), (13, 4)], None),
             ([(3 * l + 2, 6)], prod), ([(3 * l + 2, 6)], plain), ([(3 * l + 2, 6)], None), ([(l + 2, 7)], prod), ([(l + 2, 7)], plain),
             ([(2 * l + 2, 8)], prod), ([(2 * l + 2, 8)], plain)]
    refused = 0
    for pairs, widths in cases:
        ok = check(pairs, widths, sysb)
        refused += not ok
        for rank in (0, 1):
            assert (count(pairs, widths, sysb, rank) is not None) == ok, (pairs, widths)
    assert refused == 13
    assert count([(5, 0)], None, bad) is None                                 # lig_linear_check runs first
    from test_derived_slots_api import chain_system
    s16, p16 = chain_system(amd.DERIVE_MAX_WAVES, l)
    s17, p17 = chain_system(amd.DERIVE_MAX_WAVES + 1, l)
    assert count(p16, None, s16.to_binding(amd)).n_waves == 16 and count(p17, None, s17.to_binding(amd)) is None
    # its own arguments
    assert count([(5, 0)], None, sysb, rank=2) is None and count([(5, 0)], None, sysb, rank=0, world=0) is None
    info = amd.DerivedShardInfo()
    info.struct_bytes = 40
    d = np.array([[5, 0]], dtype=np.uint32)
    assert amd.load_library().lig_derived_shard_count(sysb, kinds.ctypes.data, len(kinds), l, None, d.ctypes.data, 1, 0, 1, info) == -1
    one = count([(5, 0), (6, 1)], None, sysb, rank=0, world=1).as_dict()
    assert one == dict(n_slots=2, n_terms=4, n_waves=2, n_exchanges=0, local_targets=2, local_terms=4, imported_terms=0, imports=0, exports=0, exchange_bytes=0)
    assert count([], None, sysb).as_dict()["n_waves"] == 0
