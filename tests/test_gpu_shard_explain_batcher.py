"""GPU: hip_row_batcher::explain / read_slots on a sharded batcher (shard_over + set_linear_system -> lig_shard_rows_explain /
lig_shard_rows_read_slots): tests/cpp/sharded_explain_batcher_prog.cpp as 2 ranks on the one GPU over comm_ipc, built the way
tests/test_gpu_shard_diagnose_batcher.py builds its program.  Both ranks print every record; the parent compares them with
tests/explain_ref.py over its own copy of the rows."""
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
    src, exe = os.path.join(ROOT, "tests", "cpp", "sharded_explain_batcher_prog.cpp"), os.path.join(ROOT, "tests", "cpp", "sharded_explain_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def test_sharded_row_batcher_explains_the_constraint_it_named():
    """2 ranks, one wrong witness slot on a row of the last rank's share: explain() of what diagnose() reported (and of two satisfied
    constraints, one on a row of each share) and read_slots() give the reference's records on every rank, before and after prove()"""
    exe = build_prog()
    world = 2
    shm = "/lig_seb_%s" % mr.fresh_tag()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = [mr.last_json(o) for o, _ in mr.run_ranks(lambda r: [exe, str(r), str(world), shm], world, env, timeout=300)]
    # the same stream here: the oracle's rows, the statement w[s] = b_s fixed before the slot is changed
    l, k, n = 320, 512, 2048
    job = ol.make_job(l, k, n, 192, 320 * 5, 320 * 2, synth_seed=11, generated_at=777, threads=4)
    rows = ol.form_rows(job)[0].copy()
    kinds = ol.row_kinds(job).copy()
    S = len(kinds) * l
    system = lr.System(range(S + 1), range(S), [lr.ONE] * S, range(S), range(S), lr.witness(rows, l), 0)
    bad_slot = max(r for r in range(len(kinds)) if int(kinds[r]) == 1) * l + 7
    rows[bad_slot // l, bad_slot % l, 0] ^= 1
    asked = [3, bad_slot, S - 1]
    total, rep, want_c, want_t = er.explain(system, rows, l, asked, 8)
    assert (total, rep) == (3, 3)
    res = {c: r for c, _, _, _, r in want_c}
    assert res[3] == res[S - 1] == bytes(32) and res[bad_slot] != bytes(32)
    slots = [bad_slot, 3, S - 1, bad_slot]
    want_v = er.slot_values(rows, l, slots)
    for rank, out in enumerate(outs):
        assert out["rank"] == rank and out["rows"] == len(kinds) and 0 < out["local_rows"] < len(kinds), out
        assert out["bad_slot"] == bad_slot and out["n_linear_bad"] == 1 and out["asked"] == asked, out
        assert (out["n_terms_total"], out["n_terms_reported"]) == (total, rep)
        assert [(c, nt, ft, bytes.fromhex(b), bytes.fromhex(r)) for c, nt, ft, b, r in out["constraints"]] == want_c
        assert [(c, s, ci, bytes.fromhex(a), bytes.fromhex(w)) for c, s, ci, a, w in out["terms"]] == want_t
        assert [s for s, _ in out["slots"]] == slots and [bytes.fromhex(h) for _, h in out["slots"]] == [v.tobytes() for v in want_v]
        assert (out["raised_before_commit"], out["raised_attached"], out["same_after_prove"]) == (True, True, True), out
    assert outs[0]["constraints"] == outs[1]["constraints"] and outs[0]["terms"] == outs[1]["terms"] and outs[0]["slots"] == outs[1]["slots"]
