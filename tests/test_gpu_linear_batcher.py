"""GPU: the C++ row-batching shim with a sparse linear system (hip_row_batcher::set_linear_system, hip_row_verifier::set_linear_system):
tests/cpp/linear_batcher_prog.cpp, built the way tests/test_context_cpp.py builds the other tests/cpp programs."""
import os
import subprocess

import pytest

import hip_lib
import multirank as mr
import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROOT = hip_lib.ROOT


def build_linear_batcher():
    mod = hip_lib.load()
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    odir = os.path.join(ROOT, "oracle")
    ol.build()
    src, exe = os.path.join(ROOT, "tests", "cpp", "linear_batcher_prog.cpp"), os.path.join(ROOT, "tests", "cpp", "linear_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def test_row_batcher_with_a_linear_system_needs_no_second_pass():
    """one pass + the term list = the envelope of the two-pass shim over the dense rows of the same system; the constant is the
    system's own; the next proof reuses the resident structure; the verifier shim accepts from the envelope and the structure alone"""
    p = subprocess.run([build_linear_batcher()], capture_output=True, timeout=300)
    assert p.returncode == 0, (p.stdout.decode()[-3000:], p.stderr.decode()[-3000:])
    out = mr.last_json(p.stdout.decode())
    assert out["equal_envelopes"] is True and out["const_equal"] is True and out["valid_linear"] is True, out
    assert out["second_proof_equal"] is True and out["verifier_accepts"] is True, out
