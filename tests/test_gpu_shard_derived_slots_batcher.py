"""GPU: hip_row_batcher::shard_set_derived_slots on a sharded batcher (shard_over -> lig_shard_rows_set_derived):
tests/cpp/shard_derived_slots_batcher_prog.cpp as 2 ranks on the one GPU over comm_ipc, built the way
tests/test_gpu_shard_explain_slots_batcher.py builds its program.  What is checked is written out in the program; every expected byte is
the oracle's."""
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
    src = os.path.join(ROOT, "tests", "cpp", "shard_derived_slots_batcher_prog.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "shard_derived_slots_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def test_sharded_row_batcher_forms_the_eval_outputs_of_its_own_rows():
    """2 ranks, 40 machine words on rank 0's bit row, half of them recomposed from bits rank 1 holds: the envelope of every rank is the
    oracle's over the true rows, the list is kept over reset(), a moved bit on the other rank moves its word (valid_linear == 0), and an
    unsharded batcher refuses the member"""
    exe = build_prog()
    world = 2
    shm = "/lig_sdsb_%s" % mr.fresh_tag()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = [mr.last_json(o) for o, _ in mr.run_ranks(lambda r: [exe, str(r), str(world), shm], world, env, timeout=300)]
    for rank, out in enumerate(outs):
        assert out == {"rank": rank, "counted": True, "honest_valid": True, "equals_oracle": True, "kept_over_reset": True, "false_valid_linear": 0,
                       "unsharded_refusals": 1, "local_rows": 10, "exchange_bytes": 32 * 2 * 52}, out
