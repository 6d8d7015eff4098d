"""GPU: hip_row_batcher::shard_explain_attached on a sharded batcher (shard_over + set_linear_system -> lig_shard_rows_explain_attached):
tests/cpp/sharded_explain_attached_batcher_prog.cpp as 2 ranks on the one GPU over comm_ipc, built the way
tests/test_gpu_shard_explain_batcher.py builds its program.  Both ranks print every record; the parent compares them with
tests/explain_ref.py over its own copy of the rows, under the system's own table and under the values of set_linear_values."""
import os
import subprocess

import pytest

import explain_ref as er
import hip_lib
import linear_ref as lr
import multirank as mr
import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROOT = hip_lib.ROOT


def build_prog():
    mod = hip_lib.load()
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    odir = os.path.join(ROOT, "oracle")
    ol.build()
    src = os.path.join(ROOT, "tests", "cpp", "sharded_explain_attached_batcher_prog.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "sharded_explain_attached_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def test_sharded_row_batcher_explains_the_attached_constraint_it_named():
    """2 ranks, one wrong witness slot on a row of the last rank's share: shard_explain_attached() of what diagnose_attached() reported (and
    of two satisfied constraints, one on a row of each share) gives the reference's records and the bytes of explain() on every rank,
    follows set_linear_values(), and returns the same bytes after prove(); the three std::logic_error cases"""
    exe = build_prog()
    world = 2
    shm = "/lig_seab_%s" % mr.fresh_tag()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = [mr.last_json(o) for o, _ in mr.run_ranks(lambda r: [exe, str(r), str(world), shm], world, env, timeout=300)]
    # the same stream here: the oracle's rows, the statement w[s] = b_s fixed before the slot is changed
    l, k, n = 320, 512, 2048
    job = ol.make_job(l, k, n, 192, 320 * 5, 320 * 2, synth_seed=11, generated_at=777, threads=4)
    rows = ol.form_rows(job)[0].copy()
    kinds = ol.row_kinds(job).copy()
    S = len(kinds) * l
    table = lr.witness(rows, l)
    system = lr.System(range(S + 1), range(S), [lr.ONE] * S, range(S), range(S), table, 0)
    other = list(table)
    other[3] ^= 2                                    # the program flips bit 1 of the first byte of entry 3
    system_v = lr.System(range(S + 1), range(S), [lr.ONE] * S, range(S), range(S), other, 0)
    bad_slot = max(r for r in range(len(kinds)) if int(kinds[r]) == 1) * l + 7
    rows[bad_slot // l, bad_slot % l, 0] ^= 1
    asked = [3, bad_slot, S - 1]
    want = {"first": er.explain(system, rows, l, asked, 8), "with_values": er.explain(system_v, rows, l, asked, 8)}
    res = {nm: {c: r for c, _, _, _, r in w[2]} for nm, w in want.items()}
    assert res["first"][3] == res["first"][S - 1] == bytes(32) and res["first"][bad_slot] != bytes(32)
    assert res["with_values"][3] != bytes(32) and res["with_values"][bad_slot] == res["first"][bad_slot], "the other values violate constraint 3 as well"
    for rank, out in enumerate(outs):
        assert out["rank"] == rank and out["rows"] == len(kinds) and 0 < out["local_rows"] < len(kinds), out
        assert out["bad_slot"] == bad_slot and out["n_linear_bad"] == 1 and out["asked"] == asked, out
        for nm, (total, rep, want_c, want_t) in want.items():
            got = out[nm]
            assert (total, rep) == (3, 3) and (got["n_terms_total"], got["n_terms_reported"]) == (total, rep)
            assert [(c, nt, ft, bytes.fromhex(b), bytes.fromhex(r)) for c, nt, ft, b, r in got["constraints"]] == want_c, (rank, nm)
            assert [(c, s, ci, bytes.fromhex(a), bytes.fromhex(w)) for c, s, ci, a, w in got["terms"]] == want_t, (rank, nm)
        assert (out["raised_before_commit"], out["raised_attached"], out["raised_unsharded"]) == (True, True, True), out
        assert (out["same_as_explain"], out["values_same_as_explain"], out["same_after_values_removed"], out["same_after_prove"]) == (True, True, True, True), out
    assert outs[0]["first"] == outs[1]["first"] and outs[0]["with_values"] == outs[1]["with_values"]
