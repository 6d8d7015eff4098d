"""GPU: the C++ row-batching shim with a prepared linear program (hip_row_batcher::set_linear_program / set_linear_values and the same on
hip_row_verifier): tests/cpp/linear_program_batcher_prog.cpp, built the way tests/test_gpu_linear_batcher.py builds its program."""
import os
import subprocess

import pytest

import hip_lib
import multirank as mr
import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROOT = hip_lib.ROOT


def build_program_batcher():
    mod = hip_lib.load()
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    odir = os.path.join(ROOT, "oracle")
    ol.build()
    src, exe = os.path.join(ROOT, "tests", "cpp", "linear_program_batcher_prog.cpp"), os.path.join(ROOT, "tests", "cpp", "linear_program_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def test_one_program_feeds_batcher_and_verifier_through_two_statements():
    """one lig_linear_program: two proofs around a reset(), the second with set_linear_values, both envelopes those of the
    set_linear_system path; the verifier shim accepts both (the second with its values) and rejects the second without them"""
    p = subprocess.run([build_program_batcher()], capture_output=True, timeout=300)
    assert p.returncode == 0, (p.stdout.decode()[-3000:], p.stderr.decode()[-3000:])
    out = mr.last_json(p.stdout.decode())
    assert out["first_equal"] is True and out["second_equal"] is True and out["valid"] is True, out
    assert out["verifier_accepts"] is True and out["wrong_values_rejected"] is True, out
