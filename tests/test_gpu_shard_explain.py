"""GPU: lig_shard_rows_explain / lig_shard_rows_read_slots -- the asked constraints and committed slots of a SHARDED rows job
(csrc/diagnose.hip, csrc/shard.hip): W ranks as W processes on the one GPU, collectives over comm_ipc or gloo callbacks (the worker
pattern of tests/test_gpu_shard_diagnose.py, whose CASES, deal and Builder are imported, not copied).

Expected bytes never come from the library: tests/explain_ref.py restates the records in Python integers over the WHOLE row matrix
(derived rows: x * y mod p in Python), here in the parent, and the parent compares every field of every rank's output with it.  Equality
with Context.rows_explain / rows_read_slots of the same rows on rank 0 is a second check (made in the worker, byte for byte).  Every world
makes several calls, so the file stays at six world launches.  No test hands a kernel an invalid index (the misuse calls launch
nothing) and none provokes a communicator failure; every rank process is bounded by run_ranks' timeout."""
import json
import os
import textwrap

import numpy as np
import pytest

import diagnose_ref as dr
import explain_ref as er
import multirank as mr
import oracle_lib as ol
from test_gpu_shard_diagnose import CASES, L, deal, wit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

P = ol.P
BIG = 1 << 16                      # a term cap nothing here reaches (the binding allocates the records)


WORKER = textwrap.dedent('''
    import ctypes as C, hashlib, importlib.util, json, os, sys
    import numpy as np
    root, name, plan = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
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

    def record(info, con, terms):
        """every field of every record (explain_ref's form, the 32-byte fields as hex), and a digest of the raw bytes"""
        raw = con.tobytes() + terms.tobytes() + bytes([0]) + str((int(info.n_terms_total), int(info.n_terms_reported))).encode()
        return {"counts": [int(info.n_terms_total), int(info.n_terms_reported)],
                "con": [[c, nt, ft, b.hex(), r.hex()] for c, nt, ft, b, r in er.got_constraints(con)],
                "terms": [[c, s, ci, a.hex(), w.hex()] for c, s, ci, a, w in er.got_terms(terms)],
                "digest": hashlib.sha256(raw).hexdigest()}

    for step in plan:            # one shard per step: {"case", "explain": [[system name, asked, term_cap]], "slots": [[slot, ...]], "misuse", "after_prove", "touch"}
        case = tsd.CASES[step["case"]]()
        binds = {nm: s.to_binding(pkg) for nm, s in case["systems"].items()}
        kk, msgs, local, kw, mine = ship(case)
        sh = ctx.shard_rows_begin(kk, local, g.rank, g.world, comm, generated_at=lr.GEN, **kw)
        res = {"case": step["case"], "local_rows": len(mine)}
        main = binds[case["prove"]]
        n_slots_all = len(case["kinds"]) * l
        two = np.array([0, 1], dtype=np.uint32)
        con2, terms8 = np.zeros(2, dtype=pkg.EXPLAIN_CONSTRAINT), np.zeros(8, dtype=pkg.EXPLAIN_TERM)
        X = ctx.L.lig_shard_rows_explain
        if step.get("misuse"):
            res["before_commit"] = [X(sh, C.byref(main), hp(two), 2, hp(con2), hp(terms8), 8, C.byref(info_())),
                                    ctx.L.lig_shard_rows_read_slots(sh, hp(two), 2, hp(np.zeros((2, 8), dtype=np.uint32)))]
        ctx.shard_rows_set_linear(sh, main)
        ctx.shard_rows_commit(sh)
        if step.get("misuse"):       # refused on the host before any launch and any collective: the calls below would hang or fail otherwise
            system = case["systems"][case["prove"]]
            beyond = system.to_binding(pkg, slots=system.slots[:-1] + [n_slots_all])
            down, top = np.array([3, 2], dtype=np.uint32), np.array([0, system.n_constraints], dtype=np.uint32)
            short = info_(); short.struct_bytes -= 8
            res["misuse"] = {
                "null_sys": X(sh, None, hp(two), 2, hp(con2), hp(terms8), 8, C.byref(info_())),
                "slot_out_of_range": X(sh, C.byref(beyond), hp(two), 2, hp(con2), hp(terms8), 8, C.byref(info_())),
                "not_ascending": X(sh, C.byref(main), hp(down), 2, hp(con2), hp(terms8), 8, C.byref(info_())),
                "beyond_n_constraints": X(sh, C.byref(main), hp(top), 2, hp(con2), hp(terms8), 8, C.byref(info_())),
                "null_con": X(sh, C.byref(main), hp(two), 2, None, hp(terms8), 8, C.byref(info_())),
                "null_terms": X(sh, C.byref(main), hp(two), 2, hp(con2), None, 8, C.byref(info_())),
                "short_info": X(sh, C.byref(main), hp(two), 2, hp(con2), hp(terms8), 8, C.byref(short)),
                "null_info": X(sh, C.byref(main), hp(two), 2, hp(con2), hp(terms8), 8, None)}
        if step.get("slots"):
            past = np.array([0, n_slots_all], dtype=np.uint32)
            res["slot_past_the_end"] = ctx.L.lig_shard_rows_read_slots(sh, hp(past), 2, hp(np.zeros((2, 8), dtype=np.uint32)))
            res["no_slots"] = list(ctx.shard_rows_read_slots(sh, []).shape)
            i0 = info_()
            res["no_constraints"] = [X(sh, C.byref(main), None, 0, None, None, 0, C.byref(i0)), int(i0.n_terms_total)]
        touch = step.get("touch", True)     # False: a shard that is never explained or read (its envelope is the yardstick of the others')
        def run_calls():
            ex = [record(*ctx.shard_rows_explain(sh, binds[nm], asked, term_cap=cap)) for nm, asked, cap in step.get("explain", [])]
            rd = [ctx.shard_rows_read_slots(sh, sl).tobytes().hex() for sl in step.get("slots", [])]
            return ex, rd
        if touch:
            res["explain"], res["slots"] = run_calls()
        proof, pinfo = ctx.shard_rows_prove(sh, None, None)
        res["proof"] = hashlib.sha256(proof).hexdigest()
        res["valid"] = [pinfo.valid_code, pinfo.valid_linear, pinfo.valid_quad]
        if touch and step.get("after_prove"):
            ex, rd = run_calls()
            res["after_prove_same"] = [a["digest"] for a in ex] == [a["digest"] for a in res["explain"]] and rd == res["slots"]
        ctx.shard_destroy(sh)
        if g.rank == 0 and touch:      # the second check: the one-GPU entries on the same rows
            tr, keep = ctx.rows_begin(kk, msgs, generated_at=lr.GEN, **kw)
            ctx.rows_commit(tr)
            ex = [record(*ctx.rows_explain(tr, binds[nm], asked, term_cap=cap))["digest"] for nm, asked, cap in step.get("explain", [])]
            rd = [ctx.rows_read_slots(tr, sl).tobytes().hex() for sl in step.get("slots", [])]
            res["one_gpu_same"] = ex == [a["digest"] for a in res["explain"]] and rd == res["slots"]
            ctx.trace_destroy(tr)
        out["shards"].append(res)
    print(json.dumps(out))
    ctx.close()
    g.close()
''')


def run_world(tmp_path, world, comm, plan, **env):
    script = tmp_path / "shard_explain_worker.py"
    script.write_text(WORKER)
    outs = mr.run_ranks(mr.python_argv(script, ROOT, "w", json.dumps(plan)), world, mr.rendezvous_env(world, comm, **env), timeout=300)
    outs = sorted((mr.last_json(o) for o, _ in outs), key=lambda d: d["rank"])
    assert [o["rank"] for o in outs] == list(range(world))
    return outs


_want = {}


def expected(case_name, sysname, asked, cap):
    """the Python restatement over the whole matrix, in the worker's JSON form (computed once per call of the plan)"""
    key = (case_name, sysname, tuple(asked), cap)
    if key not in _want:
        case = CASES[case_name]()
        total, rep, cons, terms = er.explain(case["systems"][sysname], case["rows"], L, asked, cap)
        _want[key] = {"counts": [total, rep], "con": [[c, nt, ft, b.hex(), r.hex()] for c, nt, ft, b, r in cons],
                      "terms": [[c, s, ci, a.hex(), w.hex()] for c, s, ci, a, w in terms]}
    return _want[key]


def check_step(outs, si, step):
    """every rank's output of every call of the step == the reference, field by field; rank 0's one-GPU output == the same bytes"""
    case = CASES[step["case"]]()
    for o in outs:
        got = o["shards"][si]
        for ci, (nm, asked, cap) in enumerate(step.get("explain", [])):
            want = expected(step["case"], nm, asked, cap)
            g = {f: got["explain"][ci][f] for f in ("counts", "con", "terms")}
            assert g["counts"] == want["counts"], (o["rank"], nm, cap, g["counts"], want["counts"])
            assert g["con"] == want["con"], "rank %d, call %d (%s, cap %d): constraint records differ from the reference" % (o["rank"], ci, nm, cap)
            assert g["terms"] == want["terms"], "rank %d, call %d (%s, cap %d): term records differ from the reference" % (o["rank"], ci, nm, cap)
        for ci, sl in enumerate(step.get("slots", [])):
            assert got["slots"][ci] == er.slot_values(case["rows"], L, sl).tobytes().hex(), "rank %d: slot list %d differs from the reference" % (o["rank"], ci)
        if step.get("after_prove"):
            assert got["after_prove_same"] is True, "rank %d: the calls after the proof return other bytes" % o["rank"]
    assert outs[0]["shards"][si]["one_gpu_same"] is True, "the one-GPU entries on the same rows return other bytes"
    assert len({json.dumps(o["shards"][si]["explain"]) for o in outs}) == 1


def owners(case, world):
    return {r: rk for rk, rws in enumerate(deal(case["kinds"], world)) for r in rws}


def terms_of(system, c):
    return range(system.term_begin[c], system.term_begin[c + 1])


def corrupted_asked():
    """every violated constraint of `main` and as many satisfied ones: a satisfied one that spans both ranks, one with and one without a
    right-hand side first, then the satisfied neighbours of the violated ones; more satisfied ones until m > 3 * 64 and the last piece
    of 64 is ragged"""
    case = CASES["corrupted"]()
    system, own = case["systems"]["main"], owners(case, 2)
    bad = [int(c) for c, _ in dr.linear_violations(system, case["rows"], L)]
    spans = lambda c: len({own[system.slots[t] // L] for t in terms_of(system, c)}) > 1
    good = [c for c in range(system.n_constraints) if c not in set(bad)]
    rhs = set(system.rhs_constraint)
    pick = [next(c for c in good if spans(c)), next(c for c in good if c in rhs), next(c for c in good if c not in rhs and len(terms_of(system, c)))]
    for c in bad:
        if len(set(pick)) >= len(bad):
            break
        pick.append(next(g for g in good if g > c and g not in pick))
    asked = sorted(set(bad) | set(pick))
    m = lambda: sum(len(terms_of(system, c)) for c in asked)
    spare = iter(c for c in good if c not in set(pick))
    while m() <= 3 * 64 or m() % 64 == 0:
        asked = sorted(set(asked) | {next(spare)})
    return case, system, bad, asked, spans, m()


def test_two_ranks_many_pieces_caps_heavy_constraints_slots_and_misuse(tmp_path):
    """ipc, W = 2, pieces of 64 terms: violated and satisfied constraints that span ranks, with and without b_c; all records, counts
    only, a cap that cuts inside a constraint; constraints of 2100 terms (33 pieces each); 200 slots in random order; the misuse calls,
    which launch nothing and leave no collective half-issued; the same bytes after the proof; the envelope of an untouched shard"""
    case, system, bad, asked, spans, m = corrupted_asked()
    rhs = set(system.rhs_constraint)
    assert bad and set(bad) <= set(asked) and len(asked) >= 2 * len(bad)
    assert any(spans(c) for c in bad) and any(spans(c) for c in asked if c not in bad), "a violated and a satisfied asked constraint must span both ranks"
    assert any(c in rhs for c in asked) and any(c not in rhs for c in asked)
    assert m > 3 * 64 and m % 64, "at least four pieces, the last one ragged"
    _, _, cons, _ = er.explain(system, case["rows"], L, asked, 0)
    cut = next(ft + 1 for _, nt, ft, _, _ in cons if nt >= 2 and ft > 0)                  # one record of a constraint in, the rest out
    heavy = case["systems"]["heavy"]
    assert [len(terms_of(heavy, c)) for c in (0, 1, 2)] == [2100, 1, 2100] and case["expect_heavy"] == [2]
    own = owners(case, 2)
    assert {own[s // L] for s in case["victims"] if s in {heavy.slots[t] for t in terms_of(heavy, 2)}} == {0, 1}
    # 200 slots in random order: repeats, the first and the last slot, rows of both ranks, a QZ row
    R = len(case["kinds"])
    rng = np.random.default_rng(17)
    slots = [0, R * L - 1, 5 * L + 11, 5 * L + 11] + [int(s) for s in rng.integers(0, R * L, 190)] + case["victims"][:6]
    slots = [slots[i] for i in rng.permutation(len(slots))]
    assert len(slots) == 200 and len(set(slots)) < 200 and {own[s // L] for s in slots} == {0, 1} and int(case["kinds"][5]) == 3
    plan = [dict(case="corrupted", explain=[["main", asked, BIG], ["main", asked, 0], ["main", asked, cut], ["heavy", [0, 1, 2], BIG]],
                 slots=[slots], misuse=True, after_prove=True),
            dict(case="corrupted", touch=False)]
    outs = run_world(tmp_path, 2, "ipc", plan, LIG_DIAG_SLICE=64)
    for o in outs:
        s = o["shards"][0]
        assert s["before_commit"] == [-3, -3], s["before_commit"]
        assert set(s["misuse"].values()) == {-1} and len(s["misuse"]) == 8, s["misuse"]
        assert s["slot_past_the_end"] == -1 and s["no_slots"] == [0, 8] and s["no_constraints"] == [0, 0]
        assert s["valid"] == [1, 0, 0], s["valid"]
        assert s["proof"] == o["shards"][1]["proof"] == outs[0]["shards"][0]["proof"], "an explained shard must produce the envelope of one that was not"
    check_step(outs, 0, plan[0])
    want = expected("corrupted", "main", asked, BIG)
    assert {c for c, _, _, _, r in want["con"] if r != bytes(32).hex()} == set(bad)
    assert expected("corrupted", "main", asked, cut)["counts"] == [m, cut] and expected("corrupted", "main", asked, 0)["terms"] == []
    assert [r != bytes(32).hex() for _, _, _, _, r in expected("corrupted", "heavy", [0, 1, 2], BIG)["con"]] == [False, False, True]


def test_narrow_rows_values_of_a_derived_row_and_of_record_slots(tmp_path):
    """the values no host holds: the product the device formed on rank 1's derived QZ row, the record-carried slots of both ranks' mixed rows"""
    case = CASES["narrow"]()
    pin_z, pin_rec, pin_x = case["expect_lin"]
    asked = sorted([pin_z, pin_rec, case["spans_ok"], pin_x])
    slots = [17 * L + c for c in range(L)] + [12 * L, 12 * L + 100, 12 * L + L - 1]
    plan = [dict(case="narrow", explain=[["main", asked, BIG], ["main", asked, 2]], slots=[slots])]
    outs = run_world(tmp_path, 2, "ipc", plan, LIG_DIAG_SLICE=64)
    check_step(outs, 0, plan[0])
    want = expected("narrow", "main", asked, BIG)
    value = {s: int.from_bytes(bytes.fromhex(w), "little") for _, s, _, _, w in want["terms"]}
    rows = case["rows"]
    assert value[17 * L + 17] == wit(rows, 15 * L + 17) * wit(rows, 16 * L + 17) % P, "the term on the derived row is x' * y"
    assert (value[12 * L + 100], value[3 * L], value[12 * L + L - 1]) == ((1 << 70) + 1, 1 << 16, P - 1 - 9), "record-carried slots of both ranks"
    res = {c: r for c, _, _, _, r in want["con"]}
    assert res[case["spans_ok"]] == bytes(32).hex() and all(res[c] != bytes(32).hex() for c in case["expect_lin"])


def test_four_ranks_one_without_rows(tmp_path):
    case = CASES["w4"]()
    system = case["systems"]["main"]
    bad = [int(c) for c, _ in dr.linear_violations(system, case["rows"], L)]
    assert {system.slots[t] // L for c in bad for t in terms_of(system, c)} >= {0, 2} and len(bad) >= 6
    slots = [0, L - 1, L + 5, 2 * L + 7, 3 * L - 1, L + 5]
    plan = [dict(case="w4", explain=[["main", bad, BIG], ["main", bad[:2], 1]], slots=[slots])]
    outs = run_world(tmp_path, 4, "ipc", plan, LIG_DIAG_SLICE=16)
    assert [o["shards"][0]["local_rows"] for o in outs] == [1, 1, 1, 0]
    assert expected("w4", "main", bad, BIG)["counts"][0] > 16
    check_step(outs, 0, plan[0])


def test_host_synchronous_collectives_over_gloo(tmp_path):
    case = CASES["gloo"]()
    asked = list(range(case["systems"]["main"].n_constraints))
    assert len(asked) == 40
    plan = [dict(case="gloo", explain=[["main", asked, BIG], ["main", asked, 0]], slots=[[9 * L + 3, 0, 6 * L + 1]])]
    outs = run_world(tmp_path, 2, None, plan, LIG_DIAG_SLICE=8)
    check_step(outs, 0, plan[0])
    assert sum(1 for _, _, _, _, r in expected("gloo", "main", asked, BIG)["con"] if r != bytes(32).hex()) == 1


@pytest.mark.parametrize("force", [False, True])
def test_one_rank(tmp_path, force):
    """W = 1: the one-GPU call (no collective); once more with LIG_SHARD_FORCE_EXCHANGE, through the exchange path with one rank"""
    case, system, bad, asked, spans, m = corrupted_asked()
    R = len(case["kinds"])
    plan = [dict(case="corrupted", explain=[["main", asked, BIG], ["main", asked, 5], ["heavy", [0, 1, 2], BIG]], slots=[[R * L - 1, 0, 7, 7, 6 * L]],
                 after_prove=True)]
    env = dict(LIG_DIAG_SLICE=64)
    if force:
        env["LIG_SHARD_FORCE_EXCHANGE"] = 1
    outs = run_world(tmp_path, 1, "ipc", plan, **env)
    check_step(outs, 0, plan[0])
