"""GPU: lig_shard_rows_explain_attached -- the asked constraints of a SHARDED rows job from the share of the system ATTACHED to every rank,
with the values of lig_shard_rows_set_linear_values in force (csrc/diagnose.hip, csrc/shard.hip): every rank selects the asked terms of
its own rows on its device, reads their values where they live, and every rank receives all records.  W ranks as W processes on the one
GPU, collectives over comm_ipc or gloo callbacks; traces, deal, Builder and cases are those of tests/test_gpu_shard_diagnose.py and
tests/test_gpu_shard_diagnose_attached.py, imported, not copied.

Expected bytes never come from the library: tests/explain_ref.py restates the records in Python integers over the WHOLE row matrix, with
the system under the table in force, here in the parent, and the parent compares every field of every rank's output with it.  Two more
checks by byte digest, made in the worker: lig_shard_rows_explain with the term list and the same table in the same world, and on rank 0
lig_rows_explain_attached on a one-GPU trace of the same rows.  Every world makes several calls, so the file stays at six world launches.
No test hands a kernel an invalid index (the misuse calls launch nothing) and none provokes a communicator failure; every rank process is
bounded by run_ranks' timeout."""
import json
import os
import textwrap

import pytest

import diagnose_ref as dr
import explain_ref as er
import multirank as mr
import oracle_lib as ol
import test_gpu_shard_diagnose as tsd
import test_gpu_shard_diagnose_attached as tda
from test_gpu_shard_explain import BIG, owners, terms_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

P = ol.P
L = tsd.L
ZERO = bytes(32).hex()
_cache = {}


def case_of(name):
    """att / narrow / w4 of tests/test_gpu_shard_diagnose_attached.py -- att with the `heavy` system of test_gpu_shard_diagnose's corrupted
    case (the same rows) under the name heavy2100 --, gloo of tests/test_gpu_shard_diagnose.py"""
    if name not in _cache:
        if name == "att":
            att = tda.CASES["att"]()
            _cache[name] = dict(att, systems=dict(att["systems"], heavy2100=tsd.CASES["corrupted"]()["systems"]["heavy"]))
        elif name in tda.CASES:
            _cache[name] = tda.CASES[name]()
        else:
            _cache[name] = dict(tsd.CASES[name](), tables={})
    return _cache[name]


WORKER = textwrap.dedent('''
    import ctypes as C, hashlib, importlib.util, json, os, sys
    import numpy as np
    root, plan = sys.argv[1], json.loads(sys.argv[2])
    l, k, n = 320, 512, 2048
    sys.path.insert(0, os.path.join(root, "tests"))
    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, "ligero-prover_amd", rel))
        m = importlib.util.module_from_spec(spec); sys.modules[name] = m; spec.loader.exec_module(m); return m
    pkg = load("ligero_prover_amd", "__init__.py")
    dist = load("lig_dist", "dist.py")
    import explain_ref as er
    import linear_ref as lr
    import test_gpu_shard_diagnose as tsd
    import test_gpu_shard_explain_attached as tea
    g = dist.Group("gloo")
    ctx = pkg.Context(l, k, n, device=0)
    comm = g.make_comm(pkg, ctx)
    out = {"rank": g.rank, "shards": []}
    hp = pkg._hptr

    def ship(case):
        """-> (kinds | DRAW_PAD, all rows as shipped, this rank's rows as shipped, keyword arguments of both begin calls, this rank's rows)"""
        kinds, rows = case["kinds"], case["rows"]
        kk, msgs = np.asarray(kinds, dtype=np.uint8).copy(), rows.copy()
        draws = (kk <= 3) | (kk == pkg.ROW_KINDS["INIT"])
        msgs[draws, l:] = 0xDEADBEEF
        kk[draws] |= pkg.ROW_DRAW_PAD
        rounds, b = pkg.shard_rows_plan(kinds, g.world)
        mine = pkg.local_rows_of(b, g.rank, g.world)
        assert [int(r) for r in mine] == tsd.deal(kinds, g.world)[g.rank]
        if "widths" in case:
            import test_gpu_mixed_rows as tm
            w, wd = case["widths"], case["wide"]
            local = tm.pack(pkg, msgs[mine], w[mine], wd[mine], l)
            return kk, tm.pack(pkg, msgs, w, wd, l), local, dict(elem_bytes=w, wide_per_row=wd), mine
        local = msgs[mine] if len(mine) else np.zeros((0, k, 8), dtype=np.uint32)
        return kk, msgs, local, {}, mine

    def info_():
        i = pkg.ExplainInfo(); i.struct_bytes = C.sizeof(pkg.ExplainInfo); return i

    def digest(info, con, terms):
        raw = con.tobytes() + terms.tobytes() + bytes([0]) + str((int(info.n_terms_total), int(info.n_terms_reported))).encode()
        return hashlib.sha256(raw).hexdigest()

    def record(info, con, terms):
        """every field of every record (explain_ref's form, the 32-byte fields as hex), and a digest of the raw bytes"""
        return {"counts": [int(info.n_terms_total), int(info.n_terms_reported)],
                "con": [[c, nt, ft, b.hex(), r.hex()] for c, nt, ft, b, r in er.got_constraints(con)],
                "terms": [[c, s, ci, a.hex(), w.hex()] for c, s, ci, a, w in er.got_terms(terms)],
                "reserved_zero": not bool(con["reserved"].any()) and not bool(terms["reserved"].any()),
                "digest": digest(info, con, terms)}

    for step in plan:            # one shard per step: {"case", "calls": [[attached system, table name or null, asked, term_cap]], "misuse", "after_prove"}
        case = tea.case_of(step["case"])
        binds = {nm: s.to_binding(pkg) for nm, s in case["systems"].items()}
        kk, msgs, local, kw, mine = ship(case)
        sh = ctx.shard_rows_begin(kk, local, g.rank, g.world, comm, generated_at=lr.GEN, **kw)
        res = {"case": step["case"], "local_rows": len(mine), "calls": [], "with_system": []}
        main = binds[case["prove"]]
        two = np.array([0, 1], dtype=np.uint32)
        con2, terms8 = np.zeros(2, dtype=pkg.EXPLAIN_CONSTRAINT), np.zeros(8, dtype=pkg.EXPLAIN_TERM)
        X = lambda *a: ctx.L.lig_shard_rows_explain_attached(sh, *a)
        ctx.shard_rows_set_linear(sh, main)
        attached, table = case["prove"], None
        if step.get("misuse"):
            res["before_commit"] = X(hp(two), 2, hp(con2), hp(terms8), 8, C.byref(info_()))
        ctx.shard_rows_commit(sh)
        if step.get("misuse"):       # refused on the host before any launch and any collective: the calls below would hang or fail otherwise
            ctx.shard_rows_set_linear(sh, None)
            no_system = X(hp(two), 2, hp(con2), hp(terms8), 8, C.byref(info_()))
            ctx.shard_rows_set_linear(sh, main)
            down, top = np.array([3, 2], dtype=np.uint32), np.array([0, case["systems"][case["prove"]].n_constraints], dtype=np.uint32)
            short = info_(); short.struct_bytes -= 8
            i0 = info_(); i0.n_terms_total = 7; i0.n_terms_reported = 7
            res["misuse"] = {
                "no_system": no_system,
                "not_ascending": X(hp(down), 2, hp(con2), hp(terms8), 8, C.byref(info_())),
                "equal_to_n_constraints": X(hp(top), 2, hp(con2), hp(terms8), 8, C.byref(info_())),
                "null_con": X(hp(two), 2, None, hp(terms8), 8, C.byref(info_())),
                "null_terms": X(hp(two), 2, hp(con2), None, 8, C.byref(info_())),
                "null_info": X(hp(two), 2, hp(con2), hp(terms8), 8, None),
                "short_info": X(hp(two), 2, hp(con2), hp(terms8), 8, C.byref(short)),
                "nothing_asked": [X(None, 0, None, None, 0, C.byref(i0)), int(i0.n_terms_total), int(i0.n_terms_reported)]}
        def run_calls(calls):
            global attached, table
            got, with_system = [], []
            for nm, tab, asked, cap in calls:
                if nm != attached:
                    ctx.shard_rows_set_linear(sh, binds[nm])
                    attached, table = nm, None
                if tab != table:
                    ctx.shard_rows_set_linear_values(sh, case["tables"][tab] if tab is not None else None)
                    table = tab
                got.append(record(*ctx.shard_rows_explain_attached(sh, asked, term_cap=cap)))
                with_system.append(digest(*ctx.shard_rows_explain(sh, binds[tab if tab is not None else nm], asked, term_cap=cap)))
            return got, with_system
        touch = bool(step.get("calls"))     # no calls: a shard that is never explained (its envelope is the yardstick of the others')
        if touch:
            res["calls"], res["with_system"] = run_calls(step["calls"])
        if attached != case["prove"]:
            ctx.shard_rows_set_linear(sh, main)
            attached, table = case["prove"], None
        if table is not None:
            ctx.shard_rows_set_linear_values(sh, None)
            table = None
        proof, pinfo = ctx.shard_rows_prove(sh, None, None)
        res["proof"] = hashlib.sha256(proof).hexdigest()
        res["valid"] = [pinfo.valid_code, pinfo.valid_linear, pinfo.valid_quad]
        if touch and step.get("after_prove"):       # the calls against the proved statement once more
            again = [(i, c) for i, c in enumerate(step["calls"]) if c[0] == case["prove"] and c[1] is None]
            ex, _ = run_calls([c for _, c in again])
            res["after_prove_same"] = bool(again) and [a["digest"] for a in ex] == [res["calls"][i]["digest"] for i, _ in again]
        ctx.shard_destroy(sh)
        if g.rank == 0 and touch:      # the third check: lig_rows_explain_attached on a one-GPU trace of the same rows, one trace per attached system
            one = []
            traces = {}
            for nm, tab, asked, cap in step["calls"]:
                if nm not in traces:
                    tr, keep = ctx.rows_begin(kk, msgs, generated_at=lr.GEN, **kw)
                    ctx.rows_set_linear(tr, binds[nm])
                    ctx.rows_commit(tr)
                    traces[nm] = [tr, keep, None]
                if traces[nm][2] != tab:
                    ctx.rows_set_linear_values(traces[nm][0], case["tables"][tab] if tab is not None else None)
                    traces[nm][2] = tab
                one.append(digest(*ctx.rows_explain_attached(traces[nm][0], asked, term_cap=cap)))
            res["one_gpu"] = one
            for tr, _, _ in traces.values():
                ctx.trace_destroy(tr)
        out["shards"].append(res)
    print(json.dumps(out))
    ctx.close()
    g.close()
''')


def run_world(tmp_path, world, comm, plan, **env):
    script = tmp_path / "shard_explain_attached_worker.py"
    script.write_text(WORKER)
    outs = mr.run_ranks(mr.python_argv(script, ROOT, json.dumps(plan)), world, mr.rendezvous_env(world, comm, **env), timeout=300)
    outs = sorted((mr.last_json(o) for o, _ in outs), key=lambda d: d["rank"])
    assert [o["rank"] for o in outs] == list(range(world))
    return outs


_want = {}


def expected(case_name, nm, tab, asked, cap):
    """the Python restatement over the whole matrix with the system under the table in force, in the worker's JSON form"""
    sysname = tab if tab is not None else nm
    key = (case_name, sysname, tuple(asked), cap)
    if key not in _want:
        case = case_of(case_name)
        total, rep, cons, terms = er.explain(case["systems"][sysname], case["rows"], L, asked, cap)
        _want[key] = {"counts": [total, rep], "con": [[c, nt, ft, b.hex(), r.hex()] for c, nt, ft, b, r in cons],
                      "terms": [[c, s, ci, a.hex(), w.hex()] for c, s, ci, a, w in terms]}
    return _want[key]


def check_step(outs, si, step):
    """every rank's output of every call of the step == the reference, field by field; == the digest of lig_shard_rows_explain with the term
    list on the same rank; rank 0's one-GPU lig_rows_explain_attached == the same digest; every rank the same bytes"""
    for o in outs:
        got = o["shards"][si]
        assert len(got["calls"]) == len(step["calls"])
        for ci, (nm, tab, asked, cap) in enumerate(step["calls"]):
            want = expected(step["case"], nm, tab, asked, cap)
            g = got["calls"][ci]
            print("rank", o["rank"], step["case"], nm, tab, "cap", cap, "counts", g["counts"], "want", want["counts"])
            assert g["counts"] == want["counts"], (o["rank"], nm, tab, cap, g["counts"], want["counts"])
            assert g["con"] == want["con"], "rank %d, call %d (%s / %s, cap %d): constraint records differ from the reference" % (o["rank"], ci, nm, tab, cap)
            assert g["terms"] == want["terms"], "rank %d, call %d (%s / %s, cap %d): term records differ from the reference" % (o["rank"], ci, nm, tab, cap)
            assert g["reserved_zero"] is True
            assert g["digest"] == got["with_system"][ci], "rank %d, call %d: lig_shard_rows_explain with the term list returns other bytes" % (o["rank"], ci)
            assert g["digest"] == outs[0]["shards"][si]["calls"][ci]["digest"], "rank %d, call %d: other bytes than rank 0" % (o["rank"], ci)
        if step.get("after_prove"):
            assert got["after_prove_same"] is True, "rank %d: the calls after the proof return other bytes" % o["rank"]
    s0 = outs[0]["shards"][si]
    assert s0["one_gpu"] == [c["digest"] for c in s0["calls"]], "lig_rows_explain_attached on a one-GPU trace of the same rows returns other bytes"


def held(system, asked, own, world):
    """m_r: the terms of the asked constraints on rows of rank r"""
    m = [0] * world
    for c in asked:
        for t in terms_of(system, c):
            m[own[system.slots[t] // L]] += 1
    return m


def att_asked():
    """every violated constraint of `main` (the one with a right-hand side and no term among them) and as many satisfied ones: a satisfied
    one that spans both ranks, one with and one without a right-hand side, one held entirely by rank 1, the satisfied neighbours of the
    violated ones; then more satisfied ones until the larger m_r exceeds 3 * 64, is no multiple of 64, and the two m_r differ"""
    case = case_of("att")
    system, own = case["systems"]["main"], owners(case, 2)
    bad = [int(c) for c, _ in dr.linear_violations(system, case["rows"], L)]
    rows_of = lambda c: {own[system.slots[t] // L] for t in terms_of(system, c)}
    spans = lambda c: len(rows_of(c)) > 1
    good = [c for c in range(system.n_constraints) if c not in set(bad)]
    rhs = set(system.rhs_constraint)
    pick = [next(c for c in good if spans(c)), next(c for c in good if c in rhs and len(terms_of(system, c))),
            next(c for c in good if c not in rhs and len(terms_of(system, c))), next(c for c in good if rows_of(c) == {1})]
    for c in bad:
        if len(set(pick)) >= len(bad):
            break
        pick.append(next(g for g in good if g > c and g not in pick))
    asked = sorted(set(bad) | set(pick))
    spare = iter(c for c in good if c not in set(pick))
    m = held(system, asked, own, 2)
    while max(m) <= 3 * 64 or max(m) % 64 == 0 or m[0] == m[1]:
        asked = sorted(set(asked) | {next(spare)})
        m = held(system, asked, own, 2)
    return case, system, bad, asked, spans, rows_of, m


def test_two_ranks_many_pieces_caps_heavy_values_and_misuse(tmp_path):
    """ipc, W = 2, pieces of 64 records: violated and satisfied constraints that span ranks, with and without b_c, a right-hand side without
    terms, a constraint of rank 1 alone; all records, counts only with NULL terms, a cap that cuts inside a constraint; constraints of 2100
    terms; another table in force and the system's own again; the misuse calls, which launch nothing and leave no collective half-issued;
    the same bytes after the proof; the envelope of an untouched shard"""
    case, system, bad, asked, spans, rows_of, m = att_asked()
    rhs = set(system.rhs_constraint)
    assert bad and set(bad) <= set(asked) and len(asked) >= 2 * len(bad)
    assert any(spans(c) for c in bad) and any(spans(c) for c in asked if c not in bad), "a violated and a satisfied asked constraint must span both ranks"
    assert any(c in rhs for c in asked) and any(c not in rhs for c in asked)
    assert case["no_terms"] in asked and case["no_terms"] in rhs and not len(terms_of(system, case["no_terms"]))
    assert any(rows_of(c) == {1} for c in asked), "a constraint held entirely by rank 1"
    assert max(m) > 3 * 64 and max(m) % 64 and m[0] != m[1], m
    _, _, cons, _ = er.explain(system, case["rows"], L, asked, 0)
    cut = next(ft + 1 for _, nt, ft, _, _ in cons if nt >= 2 and ft > 0)                  # one record of a constraint in, the rest out
    heavy = case["systems"]["heavy2100"]
    assert [len(terms_of(heavy, c)) for c in (0, 1, 2)] == [2100, 1, 2100]
    assert len({tuple(case["systems"]["main_v"].coefs), tuple(system.coefs)}) == 2
    calls = [["main", None, asked, BIG], ["main", None, asked, 0], ["main", None, asked, cut], ["heavy2100", None, [0, 1, 2], BIG],
             ["main", "main_v", asked, BIG], ["main", None, asked, BIG]]
    plan = [dict(case="att", calls=calls, misuse=True, after_prove=True), dict(case="att", calls=[])]
    outs = run_world(tmp_path, 2, "ipc", plan, LIG_DIAG_SLICE=64)
    for o in outs:
        s = o["shards"][0]
        assert s["before_commit"] == -3, s["before_commit"]
        mis = s["misuse"]
        assert mis.pop("no_system") == -3 and mis.pop("nothing_asked") == [0, 0, 0], s
        assert set(mis.values()) == {-1} and len(mis) == 6, mis
        assert s["valid"] == [1, 0, 0], s["valid"]
        assert s["proof"] == o["shards"][1]["proof"] == outs[0]["shards"][0]["proof"], "an explained shard must produce the envelope of one that was not"
        assert s["calls"][5]["digest"] == s["calls"][0]["digest"] != s["calls"][4]["digest"], "the system's own values again after None"
    check_step(outs, 0, plan[0])
    want = expected("att", "main", None, asked, BIG)
    assert {c for c, _, _, _, r in want["con"] if r != ZERO} == set(bad)
    no_terms = next(rec for rec in want["con"] if rec[0] == case["no_terms"])
    b = system.coefs[system.rhs_coef[system.rhs_constraint.index(case["no_terms"])]]
    assert no_terms[1] == 0 and no_terms[4] == dr.residual_bytes(P - b).hex(), "a right-hand side without terms: n_terms = 0, the residual is -b_c"
    assert expected("att", "main", None, asked, cut)["counts"] == [sum(m), cut] and expected("att", "main", None, asked, 0)["terms"] == []
    other = expected("att", "main", "main_v", asked, BIG)
    assert other["con"] != want["con"] and other["terms"] != want["terms"], "the other table gives other coefficient values, rhs and residuals"
    assert [r != ZERO for _, _, _, _, r in expected("att", "heavy2100", None, [0, 1, 2], BIG)["con"]] == [False, False, True]


def test_narrow_rows_values_of_a_derived_row_and_of_record_slots(tmp_path):
    """the values no host holds: the product the device formed on rank 1's derived QZ row, the record-carried slots of both ranks' mixed rows"""
    case = case_of("narrow")
    pin_z, pin_rec, pin_x = case["expect_lin"]
    asked = sorted([pin_z, pin_rec, case["spans_ok"], pin_x])
    plan = [dict(case="narrow", calls=[["main", None, asked, BIG], ["main", None, asked, 2]])]
    outs = run_world(tmp_path, 2, "ipc", plan, LIG_DIAG_SLICE=64)
    check_step(outs, 0, plan[0])
    want = expected("narrow", "main", None, asked, BIG)
    value = {s: int.from_bytes(bytes.fromhex(w), "little") for _, s, _, _, w in want["terms"]}
    rows = case["rows"]
    assert owners(case, 2)[17] == 1 and value[17 * L + 17] == tsd.wit(rows, 15 * L + 17) * tsd.wit(rows, 16 * L + 17) % P, "the term on the derived row is x' * y"
    assert (value[12 * L + 100], value[3 * L], value[12 * L + L - 1]) == ((1 << 70) + 1, 1 << 16, P - 1 - 9), "record-carried slots of both ranks"
    res = {c: r for c, _, _, _, r in want["con"]}
    assert res[case["spans_ok"]] == ZERO and all(res[c] != ZERO for c in case["expect_lin"])


def test_four_ranks_one_without_rows(tmp_path):
    """slice 16; rank 3 has no rows, hence m_r = 0, and holds the b_c of asked constraints all the same"""
    case = case_of("w4")
    system, own = case["systems"]["main"], owners(case, 4)
    bad = [int(c) for c, _ in dr.linear_violations(system, case["rows"], L)]
    m = held(system, bad, own, 4)
    n_rhs = len(system.rhs_constraint)
    assert sum(m) > 16 and m[3] == 0, m
    assert set(system.rhs_constraint[3 * n_rhs // 4:]) & set(bad), "rank 3 holds the right-hand side of an asked constraint"
    plan = [dict(case="w4", calls=[["main", None, bad, BIG], ["main", None, bad[:2], 1], ["main", "main_v", bad, BIG]])]
    outs = run_world(tmp_path, 4, "ipc", plan, LIG_DIAG_SLICE=16)
    assert [o["shards"][0]["local_rows"] for o in outs] == [1, 1, 1, 0]
    check_step(outs, 0, plan[0])


def test_host_synchronous_collectives_over_gloo(tmp_path):
    case = case_of("gloo")
    asked = list(range(case["systems"]["main"].n_constraints))
    assert len(asked) == 40
    plan = [dict(case="gloo", calls=[["main", None, asked, BIG], ["main", None, asked, 0]])]
    outs = run_world(tmp_path, 2, None, plan, LIG_DIAG_SLICE=8)
    check_step(outs, 0, plan[0])
    assert sum(1 for _, _, _, _, r in expected("gloo", "main", None, asked, BIG)["con"] if r != ZERO) == 1


def test_one_rank_without_and_with_the_forced_exchange(tmp_path):
    """W = 1: the passes over the rank's compactly numbered share without a collective; once more with LIG_SHARD_FORCE_EXCHANGE, through the
    exchange path with one rank: the same bytes"""
    case, system, bad, asked, spans, rows_of, m = att_asked()
    calls = [["main", None, asked, BIG], ["main", None, asked, 5], ["heavy2100", None, [0, 1, 2], BIG], ["main", "main_v", asked, BIG]]
    plan = [dict(case="att", calls=calls, after_prove=True)]
    digests = []
    for env in (dict(LIG_DIAG_SLICE=64), dict(LIG_DIAG_SLICE=64, LIG_SHARD_FORCE_EXCHANGE=1)):
        outs = run_world(tmp_path, 1, "ipc", plan, **env)
        check_step(outs, 0, plan[0])
        digests.append([c["digest"] for c in outs[0]["shards"][0]["calls"]])
    assert digests[0] == digests[1]
