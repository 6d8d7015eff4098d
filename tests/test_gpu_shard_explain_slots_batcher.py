"""GPU: hip_row_batcher::shard_explain_slots* / shard_untouched_slots* on a sharded batcher (shard_over + set_linear_system ->
lig_shard_rows_explain_slots*, lig_shard_rows_untouched_slots*): tests/cpp/sharded_explain_slots_batcher_prog.cpp as 2 ranks on the one GPU
over comm_ipc, built the way tests/test_gpu_shard_explain_attached_batcher.py builds its program.  Both ranks print every record; the
parent compares them with tests/slots_ref.py over its own copy of the rows, under the system's own table and under the values of
set_linear_values."""
import os
import subprocess

import pytest

import hip_lib
import linear_ref as lr
import multirank as mr
import oracle_lib as ol
import slots_ref as sr

pytestmark = pytest.mark.gpu
ROOT = hip_lib.ROOT


def build_prog():
    mod = hip_lib.load()
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    odir = os.path.join(ROOT, "oracle")
    ol.build()
    src = os.path.join(ROOT, "tests", "cpp", "sharded_explain_slots_batcher_prog.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "sharded_explain_slots_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def test_sharded_row_batcher_explains_slots_and_lists_the_untouched_ones():
    """2 ranks, one wrong witness slot on a row of the last rank's share: shard_explain_slots_attached() of slots of both shares (one without
    a term, one on two constraints, the wrong one, the last of the trace) gives the reference's records and the bytes of the term-list form
    on every rank, follows set_linear_values(), and returns the same bytes after prove(); shard_untouched_slots*() list the slots the
    statement skips; the std::logic_error cases"""
    exe = build_prog()
    world = 2
    shm = "/lig_sesb_%s" % mr.fresh_tag()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = [mr.last_json(o) for o, _ in mr.run_ranks(lambda r: [exe, str(r), str(world), shm], world, env, timeout=300)]
    # the same stream here: the oracle's rows, the statement fixed before the slot is changed
    l, k, n = 320, 512, 2048
    job = ol.make_job(l, k, n, 192, 320 * 5, 320 * 2, synth_seed=11, generated_at=777, threads=4)
    rows = ol.form_rows(job)[0].copy()
    kinds = ol.row_kinds(job).copy()
    S = len(kinds) * l
    w = lr.witness(rows, l)
    slot_of = [s + 1 if s % 64 == 7 else s for s in range(S)]
    table = [w[s] for s in slot_of]
    system = lr.System(range(S + 1), slot_of, [lr.ONE] * S, range(S), range(S), table, 0)
    other = list(table)
    other[8] ^= 2                                    # the program flips bit 1 of the first byte of entry 8
    system_v = lr.System(range(S + 1), slot_of, [lr.ONE] * S, range(S), range(S), other, 0)
    bad_slot = max(r for r in range(len(kinds)) if int(kinds[r]) == 1) * l + 9
    rows[bad_slot // l, bad_slot % l, 0] ^= 1
    asked = [7, 8, 9, bad_slot, bad_slot + 1, S - 1]
    want = {"first": sr.explain_slots(system, kinds, rows, l, asked, 16), "with_values": sr.explain_slots(system_v, kinds, rows, l, asked, 16)}
    zero = bytes(32)
    for nm, (total, rep, distinct, recs, terms) in want.items():
        assert (total, rep, distinct) == (6, 6, 6) and [r[2] for r in recs] == [0, 2, 1, 1, 1, 1]
        res = {(t[0], t[1]): t[5] for t in terms}
        assert res[(bad_slot, bad_slot)] != zero and res[(9, 9)] == zero and res[(8, 7)] == zero
        assert (res[(8, 8)] != zero) == (nm == "with_values"), "the other values violate constraint 8 on slot 8, not constraint 7"
    un = sr.untouched(system, kinds, rows, l, False, 6)
    un_nz = sr.untouched(system, kinds, rows, l, True, 2)
    assert un[0] == S // 64 and [s for s, _, _ in un[3]] == [7 + 64 * i for i in range(6)]
    for rank, out in enumerate(outs):
        assert out["rank"] == rank and out["rows"] == len(kinds) and 0 < out["local_rows"] < len(kinds), out
        assert out["bad_slot"] == bad_slot and out["asked"] == asked, out
        for nm, (total, rep, distinct, recs, terms) in want.items():
            got = out[nm]
            assert got["counts"] == [total, rep, distinct], (rank, nm)
            assert [(s, kd, nt, ft, bytes.fromhex(v)) for s, kd, nt, ft, v in got["slots"]] == recs, (rank, nm)
            assert [(s, c, ci, ct, bytes.fromhex(a), bytes.fromhex(r)) for s, c, ci, ct, a, r in got["terms"]] == terms, (rank, nm)
        for nm, (n_un, n_nz, rep, vals) in (("untouched", un), ("untouched_nonzero", un_nz)):
            got = out[nm]
            assert got["counts"] == [n_un, n_nz, rep], (rank, nm)
            assert [(s, kd, bytes.fromhex(v)) for s, kd, v in got["values"]] == vals, (rank, nm)
        assert (out["raised_before_commit"], out["raised_unsharded_members"], out["raised_unsharded"]) == (4, 4, 4), out
        assert (out["same_as_list"], out["values_same_as_list"], out["untouched_same_as_list"], out["same_after_values_removed"], out["same_after_prove"]) == (True,) * 5, out
    for nm in ("first", "with_values", "untouched", "untouched_nonzero"):
        assert outs[0][nm] == outs[1][nm]
