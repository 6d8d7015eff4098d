"""GPU: the row-batching shim with derived slots (hip_row_batcher::set_derived_slots, include/lig_hip_row_batcher.hpp) -- what is checked
is written out in tests/cpp/derived_slots_batcher_prog.cpp; every expected byte is the oracle's."""
import os
import subprocess

import pytest

import hip_lib
import multirank as mr
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def build_prog():
    mod = hip_lib.load()
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    odir = os.path.join(ROOT, "oracle")
    ol.build()
    src, exe = os.path.join(ROOT, "tests", "cpp", "derived_slots_batcher_prog.cpp"), os.path.join(ROOT, "tests", "cpp", "derived_slots_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def test_row_batcher_forms_the_eval_outputs_of_a_bit_row():
    """40 machine words recomposed from bits on a bit row: the row ships as a pure bit row, the envelope is the oracle's over the true
    rows, the list survives reset(), a moved bit moves its words (valid_linear == 0), a sharded batcher refuses the list"""
    p = subprocess.run([build_prog()], capture_output=True, timeout=300)
    assert p.returncode == 0, (p.stdout.decode()[-3000:], p.stderr.decode()[-3000:])
    o = mr.last_json(p.stdout.decode())
    assert o["equals_oracle"] is True and o["derived_slots"] == 40, o
    assert o["shipped_bytes"] == o["computed_bytes"] and o["shipped_bytes"] < o["underived_bytes"], o
    assert o["linear_honest_valid"] is True and o["linear_equals_oracle"] is True and o["kept_over_reset"] is True, o
    assert o["linear_false_valid_linear"] == 0 and o["sharded_refusals"] == 2, o
