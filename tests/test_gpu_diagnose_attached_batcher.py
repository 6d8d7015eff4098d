"""GPU: hip_row_batcher::diagnose_attached (include/lig_hip_row_batcher.hpp) on a batcher that was given a prepared program and this
statement's values names the constraint the Python reference names; the present diagnose() on the same batcher still evaluates the
quadratic part only: tests/cpp/diagnose_attached_batcher_prog.cpp, built the way tests/test_gpu_diagnose_batcher.py builds its program."""
import os
import subprocess

import pytest

import diagnose_ref as dr
import hip_lib
import linear_ref as lr
import multirank as mr
import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROOT = hip_lib.ROOT


def build_diagnose_attached_batcher():
    mod = hip_lib.load()
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    odir = os.path.join(ROOT, "oracle")
    ol.build()
    src, exe = os.path.join(ROOT, "tests", "cpp", "diagnose_attached_batcher_prog.cpp"), os.path.join(ROOT, "tests", "cpp", "diagnose_attached_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def test_row_batcher_with_a_program_names_the_violated_constraint():
    p = subprocess.run([build_diagnose_attached_batcher()], capture_output=True, timeout=300)
    assert p.returncode == 0, (p.stdout.decode()[-3000:], p.stderr.decode()[-3000:])
    out = mr.last_json(p.stdout.decode())
    # the same stream here: the oracle's rows, the statement w[s] = b_s with the TRUE values (set_linear_values), fixed before the slots
    # are changed; the program's own table is wrong at out["stale"], where the witness is not
    l, k, n = 320, 512, 2048
    job = ol.make_job(l, k, n, 192, 320 * 5, 320 * 2, synth_seed=11, generated_at=777, threads=4)
    rows = ol.form_rows(job)[0].copy()
    kinds = ol.row_kinds(job).copy()
    assert out["rows"] == len(kinds)
    S = len(kinds) * l
    table = lr.witness(rows, l)
    system = lr.System(range(S + 1), range(S), [lr.ONE] * S, range(S), range(S), table, 0)
    for s in out["changed"]:
        rows[s // l, s % l, 0] ^= 1
    want_l, want_q = dr.linear_violations(system, rows, l), dr.quad_violations(kinds, rows, l)
    assert len(out["changed"]) == 2 and [c for c, _ in want_l] == sorted(out["changed"]) and len(want_q) == 1
    assert len(out["stale"]) == 3 and not set(out["stale"]) & set(out["changed"])
    assert (out["n_linear_bad"], out["n_quad_bad"]) == (len(want_l), len(want_q))
    assert [(c, bytes.fromhex(h)) for c, h in out["linear"]] == dr.linear_records(want_l)
    assert [(x, y, z, i, bytes.fromhex(h)) for x, y, z, i, h in out["quad"]] == dr.quad_records(want_q)
    assert out["same_after_prove"] is True and out["valid_linear"] == 0 and out["valid_quad"] == 0
    assert out["plain_diagnose_quadratic_only"] is True
    assert (out["raised_before_commit"], out["raised_without_linear"], out["raised_sharded"]) == (True, True, True)
