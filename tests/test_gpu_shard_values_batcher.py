"""GPU: hip_row_batcher::set_linear_values and ::diagnose_attached on a sharded batcher (shard_over + set_linear_system ->
lig_shard_rows_set_linear_values, lig_shard_rows_diagnose_attached): tests/cpp/sharded_values_batcher_prog.cpp as 2 ranks on the one GPU
over comm_ipc, built the way tests/test_gpu_shard_diagnose_batcher.py builds its program."""
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
    src, exe = os.path.join(ROOT, "tests", "cpp", "sharded_values_batcher_prog.cpp"), os.path.join(ROOT, "tests", "cpp", "sharded_values_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def test_sharded_row_batcher_values_and_diagnose_attached_equal_the_unsharded_batcher():
    """2 ranks, a system given with the table T0 and then the values T1: prove() on every rank gives the envelope of the unsharded batcher
    given the system with coefs = T1, again after reset(); diagnose_attached() gives zero counts under T1 and, with the values taken back,
    the bytes of the unsharded batcher under T0 -- the three constraints the tables differ in; set_linear_program is still refused"""
    exe = build_prog()
    world = 2
    shm = "/lig_svb_%s" % mr.fresh_tag()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = mr.run_ranks(lambda r: [exe, str(r), str(world), shm], world, env, timeout=300)
    for rank, (o, _) in enumerate(outs):
        out = mr.last_json(o)
        assert out["rank"] == rank
        assert out["unsharded_names_the_three"] is True, out
        assert out["values_envelope_equal"] is True and out["after_reset_equal"] is True, out
        assert out["attached_zero_under_T1"] is True and out["attached_equal_under_T0"] is True, out
        assert out["program_refused"] is True and out["local_rows"] > 0, out
