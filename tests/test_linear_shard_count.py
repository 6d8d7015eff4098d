"""CPU: lig_linear_shard_count (host only, no device call) -- the share of a sparse linear system that a rank of a sharded rows job keeps
(its terms) and samples (the constraints it needs) -- against a count made in Python from shard_rows_plan and local_rows_of
(tests/shard_linear_ref.py)."""
import numpy as np
import pytest

import hip_lib
import linear_ref as lr
import shard_linear_ref as sl

L_, K_, N_ = 320, 512, 2048
WORLDS = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


@pytest.fixture(scope="module")
def trace():
    kinds, rows, _ = lr.build_trace(L_, K_, N_, 3 * L_ + 17, L_ + 9)
    return kinds, rows


def systems(trace):
    kinds, rows = trace
    return {"seeded": lr.make_system(kinds, rows, L_, 30000, 0, seed=5), "first_random": lr.make_system(kinds, rows, L_, 7000, 1000, seed=8, hot_terms=3000),
            "equalities": lr.make_equality_system(kinds, L_, 0)}


@pytest.mark.parametrize("name", ["seeded", "first_random", "equalities"])
def test_counts_equal_the_python_count_for_every_world(amd, trace, name):
    kinds = trace[0]
    system = systems(trace)[name]
    sysb = system.to_binding(amd)
    n_terms = len(system.slots)
    for world in WORLDS:
        _, b = amd.shard_rows_plan(kinds, world)
        got = [amd.linear_shard_count(sysb, kinds, L_, rank, world) for rank in range(world)]
        want = [sl.python_count(amd, system, kinds, L_, rank, world) for rank in range(world)]
        assert got == want, (world, got, want)
        assert sum(g[0] for g in got) == n_terms
        for rank in range(world):
            if not amd.local_rows_of(b, rank, world):
                assert got[rank][0] == 0
        if world == 1:
            assert got[0] == (n_terms, sl.nonempty_constraints(system))
    # the small trace has fewer chunks than 8 ranks: the case of a rank without rows is really there
    _, b = amd.shard_rows_plan(kinds, 8)
    assert any(not amd.local_rows_of(b, rank, 8) for rank in range(8))
    # DRAW_PAD bits on the kinds change nothing
    assert amd.linear_shard_count(sysb, kinds | amd.ROW_DRAW_PAD, L_, 1, 2) == sl.python_count(amd, system, kinds, L_, 1, 2)


def test_a_row_local_system_is_sampled_once_over_all_ranks(amd):
    """the cap that shows a rank does not sample the whole stream: with every constraint on one row, a constraint is needed by the rank
    that owns the row and at most by the one whose slice holds its right-hand side -- sum over ranks <= n_constraints + n_rhs"""
    kinds, _, _ = lr.build_trace(L_, K_, N_, 40 * L_ + 5, 3 * L_)
    system = sl.row_local_system(kinds, L_)
    nc, n_rhs = system.n_constraints, len(system.rhs_constraint)
    assert nc > 250 and n_rhs > 80
    assert amd.linear_check(system.to_binding(amd), kinds, L_) == 0
    sysb = system.to_binding(amd)
    for world in WORLDS:
        want = [sl.python_count(amd, system, kinds, L_, rank, world) for rank in range(world)]
        assert sum(w[1] for w in want) <= nc + n_rhs                       # the Python count itself satisfies the cap
        got = [amd.linear_shard_count(sysb, kinds, L_, rank, world) for rank in range(world)]
        assert got == want
        assert sum(g[1] for g in got) <= nc + n_rhs
        if world > 1:
            assert max(g[1] for g in got) < nc                              # no rank samples everything


def test_broken_inputs_return_e_arg(amd, trace):
    kinds = trace[0]
    system = systems(trace)["equalities"]
    sysb = system.to_binding(amd)
    L = amd.load_library()
    import ctypes as C
    lt, nc = C.c_uint64(), C.c_uint64()
    kp = np.ascontiguousarray(kinds, dtype=np.uint8)

    def rc(s, rank, world):
        return L.lig_linear_shard_count(C.byref(s), kp.ctypes.data, len(kp), L_, rank, world, C.byref(lt), C.byref(nc))

    assert rc(sysb, 0, 1) == 0
    assert rc(sysb, 2, 2) == -1 and rc(sysb, 1, 1) == -1                    # rank >= world
    assert rc(sysb, 0, 0) == -1                                             # world = 0
    beyond = system.to_binding(amd, slots=system.slots[:-1] + [len(kinds) * L_])
    assert amd.linear_check(beyond, kinds, L_) == -1 and rc(beyond, 0, 2) == -1
    with pytest.raises(amd.LigError):
        amd.linear_shard_count(beyond, kinds, L_, 0, 2)
