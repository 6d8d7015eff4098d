"""GPU: hip_row_batcher::explain_slots / explain_slots_attached / untouched_slots / untouched_slots_attached
(include/lig_hip_row_batcher.hpp) return the bytes the Python binding returns for the same statement on the same trace -- with the values
of set_linear_values in force, from a system and from a prepared program alike: tests/cpp/explain_slots_batcher_prog.cpp, built the way
tests/test_gpu_explain_batcher.py builds its program, run once."""
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


def build_explain_slots_batcher():
    mod = hip_lib.load()
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    odir = os.path.join(ROOT, "oracle")
    ol.build()
    src, exe = os.path.join(ROOT, "tests", "cpp", "explain_slots_batcher_prog.cpp"), os.path.join(ROOT, "tests", "cpp", "explain_slots_batcher_prog")
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-L" + os.path.dirname(mod.LIB_PATH), "-llig_hip", "-L" + odir, "-llig_oracle",
                           "-Wl,-rpath," + os.path.dirname(mod.LIB_PATH), "-Wl,-rpath," + odir, "-o", exe])
    return exe


def test_row_batcher_explains_slots_as_the_binding_does():
    p = subprocess.run([build_explain_slots_batcher()], capture_output=True, timeout=300)
    assert p.returncode == 0, (p.stdout.decode()[-3000:], p.stderr.decode()[-3000:])
    out = mr.last_json(p.stdout.decode())
    # the same stream here: the oracle's rows, the driver's statement with the TRUE table (the one it set with set_linear_values)
    amd = hip_lib.load()
    l, k, n = 320, 512, 2048
    job = ol.make_job(l, k, n, 192, 320 * 5, 320 * 2, synth_seed=11, generated_at=777, threads=4)
    rows = ol.form_rows(job)[0].copy()
    kinds = ol.row_kinds(job).copy()
    assert out["rows"] == len(kinds)
    S, NC, hot = len(kinds) * l, 3000, 123
    term_begin, slots, cidx = [0], [], []
    for c in range(NC):
        slots += [37 * c % S, (101 * c + 5) % S] + ([hot] if c % 2 == 0 else [])
        cidx += [lr.ONE, c % 3] + ([lr.NEG_ONE] if c % 2 == 0 else [])
        term_begin.append(len(slots))
    system = lr.System(term_begin, slots, cidx, [], [], [5, 7, 11], 0)
    asked = [0, 5, 37, hot, 3000, S - 1]
    assert out["asked"] == asked
    c = amd.Context(l, k, n)
    try:
        tr, keep = c.rows_begin(kinds, rows, generated_at=777)
        c.rows_set_linear(tr, system.to_binding(amd))
        c.rows_commit(tr)
        info, rec, terms = c.rows_explain_slots_attached(tr, asked, term_cap=48)
        uinfo, un = c.rows_untouched_slots_attached(tr, nonzero_only=True, cap=24)
        c.trace_destroy(tr)
    finally:
        c.close()
    assert (out["n_terms_total"], out["n_terms_reported"], out["n_constraints_distinct"]) == (info.n_terms_total, info.n_terms_reported, info.n_constraints_distinct)
    assert info.n_terms_reported == 48 < info.n_terms_total and info.n_constraints_distinct >= NC // 2
    assert [(s, kd, nt, ft, bytes.fromhex(v)) for s, kd, nt, ft, v in out["slots"]] == sr.got_slots(rec)
    assert [(s, cn, ci, ct, bytes.fromhex(a), bytes.fromhex(r)) for s, cn, ci, ct, a, r in out["terms"]] == sr.got_terms(terms)
    assert (out["n_untouched"], out["n_untouched_nonzero"], out["n_reported"]) == (uinfo.n_untouched, uinfo.n_untouched_nonzero, uinfo.n_reported)
    assert uinfo.n_reported == 24 and [(s, kd, bytes.fromhex(v)) for s, kd, v in out["untouched"]] == sr.got_values(un)
    # ... and both are the reference's
    total, rep, distinct, want_s, want_t = sr.explain_slots(system, kinds, rows, l, asked, 48)
    assert (info.n_terms_total, info.n_terms_reported, info.n_constraints_distinct) == (total, rep, distinct)
    assert sr.got_slots(rec) == want_s and sr.got_terms(terms) == want_t
    assert dict((s, nt) for s, _, nt, _, _ in want_s)[hot] >= NC // 2 and any(r != bytes(32) for *_, r in want_t)
    n_un, n_nz, n_rep, want_u = sr.untouched(system, kinds, rows, l, True, 24)
    assert (uinfo.n_untouched, uinfo.n_untouched_nonzero, uinfo.n_reported) == (n_un, n_nz, n_rep) and sr.got_values(un) == want_u
    assert out["list_equals_attached"] is True and out["same_after_prove"] is True and out["program_equals_system"] is True
    assert (out["raised_before_commit"], out["raised_without_terms"], out["raised_without_linear"], out["raised_sharded"]) == (4, 2, 4, 4)
