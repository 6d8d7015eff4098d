"""GPU: hip_row_batcher::diagnose on a sharded batcher (shard_over + set_linear_system -> lig_shard_rows_diagnose):
tests/cpp/sharded_diagnose_batcher_prog.cpp as 2 ranks on the one GPU over comm_ipc, built the way
tests/test_gpu_shard_linear_batcher.py builds its program."""
import os
import subprocess

import pytest

import hip_lib
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
    src, exe = os.path.join(ROOT, "tests", "cpp", "sharded_diagnose_batcher_prog.cpp"), os.path.join(ROOT, "tests", "cpp", "sharded_diagnose_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def test_sharded_row_batcher_diagnose_equals_the_unsharded_batcher():
    """2 ranks, one wrong witness slot on a row of the last rank's share: diagnose() on every rank gives the bytes of the unsharded
    batcher -- the constraint on that slot, its triple's column, global rows -- with records, with counts only, and after prove()"""
    exe = build_prog()
    world = 2
    shm = "/lig_sdb_%s" % mr.fresh_tag()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = mr.run_ranks(lambda r: [exe, str(r), str(world), shm], world, env, timeout=300)
    for rank, (o, _) in enumerate(outs):
        out = mr.last_json(o)
        assert out["rank"] == rank
        assert out["unsharded_names_the_slot"] is True, out
        assert out["equal_unsharded"] is True and out["counts_only_equal"] is True and out["proved_after"] is True and out["local_rows"] > 0, out
