"""GPU: the C++ row-batching shim, sharded AND with a sparse linear system (hip_row_batcher::shard_over + set_linear_system):
tests/cpp/sharded_linear_batcher_prog.cpp as 2 ranks on the one GPU over comm_ipc, built the way tests/test_gpu_linear_batcher.py
builds its program."""
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
    src, exe = os.path.join(ROOT, "tests", "cpp", "sharded_linear_batcher_prog.cpp"), os.path.join(ROOT, "tests", "cpp", "sharded_linear_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def test_sharded_row_batcher_with_a_linear_system_needs_no_second_pass():
    """2 ranks, one pass of the guest each, the term list of the whole trace on both: every rank's envelope is the unsharded batcher's
    (and the oracle's), the constant is the system's own, the next proof after reset() gives the same bytes"""
    exe = build_prog()
    world = 2
    shm = "/lig_slb_%s" % mr.fresh_tag()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = mr.run_ranks(lambda r: [exe, str(r), str(world), shm], world, env, timeout=300)
    for rank, (o, _) in enumerate(outs):
        out = mr.last_json(o)
        assert out["rank"] == rank
        assert out["equal_unsharded"] is True and out["equal_oracle"] is True and out["const_equal"] is True, out
        assert out["valid"] is True and out["second_proof_equal"] is True and out["local_rows"] > 0, out
