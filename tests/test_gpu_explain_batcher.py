"""GPU: hip_row_batcher::explain / explain_attached / read_slots (include/lig_hip_row_batcher.hpp) show the constraints diagnose_attached()
named as the Python reference (tests/explain_ref.py) computes them, with the values of set_linear_values in force; a batcher that holds a
prepared program only returns the same bytes through explain_attached(): tests/cpp/explain_batcher_prog.cpp, built the way
tests/test_gpu_diagnose_attached_batcher.py builds its program."""
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


def build_explain_batcher():
    mod = hip_lib.load()
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    odir = os.path.join(ROOT, "oracle")
    ol.build()
    src, exe = os.path.join(ROOT, "tests", "cpp", "explain_batcher_prog.cpp"), os.path.join(ROOT, "tests", "cpp", "explain_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def test_row_batcher_explains_the_constraints_it_named():
    p = subprocess.run([build_explain_batcher()], capture_output=True, timeout=300)
    assert p.returncode == 0, (p.stdout.decode()[-3000:], p.stderr.decode()[-3000:])
    out = mr.last_json(p.stdout.decode())
    # the same stream here: the oracle's rows, the statement w[s] = b_s with the TRUE values (set_linear_values), fixed before the slots
    # are changed; the table the system was given with is wrong at out["stale"], where the witness is not
    l, k, n = 320, 512, 2048
    job = ol.make_job(l, k, n, 192, 320 * 5, 320 * 2, synth_seed=11, generated_at=777, threads=4)
    rows = ol.form_rows(job)[0].copy()
    kinds = ol.row_kinds(job).copy()
    assert out["rows"] == len(kinds)
    S = len(kinds) * l
    system = lr.System(range(S + 1), range(S), [lr.ONE] * S, range(S), range(S), lr.witness(rows, l), 0)
    for s in out["changed"]:
        rows[s // l, s % l, 0] ^= 1
    asked = sorted([out["stale"]] + out["changed"])
    assert out["asked"] == asked and len(set(asked)) == 3
    total, rep, want_c, want_t = er.explain(system, rows, l, asked, 8)
    assert (out["n_terms_total"], out["n_terms_reported"]) == (total, rep) == (3, 3)
    assert [(c, nt, ft, bytes.fromhex(b), bytes.fromhex(r)) for c, nt, ft, b, r in out["constraints"]] == want_c
    assert [(c, s, ci, bytes.fromhex(a), bytes.fromhex(w)) for c, s, ci, a, w in out["terms"]] == want_t
    res = {c: r for c, _, _, _, r in want_c}
    assert res[out["stale"]] == bytes(32) and all(res[s] != bytes(32) for s in out["changed"])       # the values in force, not the stale table
    want_v = er.slot_values(rows, l, [s for s, _ in out["slots"]])
    assert [bytes.fromhex(h) for _, h in out["slots"]] == [v.tobytes() for v in want_v]
    assert [s for s, _ in out["slots"]] == [out["changed"][1], 0, out["changed"][0], out["changed"][1]]
    assert out["list_equals_attached"] is True and out["same_after_prove"] is True and out["program_equals_system"] is True
    assert out["read_without_statement"] is True and out["valid_linear"] == 0
    assert (out["raised_before_commit"], out["raised_without_terms"], out["raised_without_linear"], out["raised_sharded"]) == (True, True, True, 3)
