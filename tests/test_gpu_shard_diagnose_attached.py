"""GPU: lig_shard_rows_diagnose_attached -- the violated constraints of a SHARDED rows job, evaluated against the share of the system
ATTACHED to every rank with the values of lig_shard_rows_set_linear_values in force (csrc/diagnose.hip, csrc/shard.hip).  W ranks as W
processes on the one GPU over comm_ipc; traces, deal and the Builder are those of tests/test_gpu_shard_diagnose.py.

Expected records never come from the library: tests/diagnose_ref.py restates both residuals in Python integers over the WHOLE row matrix,
here in the parent, and the parent compares them with every rank's bytes for every pair of caps.  Equality with
lig_shard_rows_diagnose(system) in the same world is a second check.  A system is attached with lig_shard_rows_set_linear (a second call
replaces it), so one shard serves several systems and several tables and the file stays at six world launches.  No test hands a kernel
an invalid index (the refused calls launch nothing) and none provokes a communicator failure."""
import json
import os
import textwrap

import numpy as np
import pytest

import diagnose_ref as dr
import linear_ref as lr
import multirank as mr
import oracle_lib as ol
import test_gpu_shard_diagnose as tsd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

P = ol.P
L = tsd.L
ONE, NEG_ONE = lr.ONE, lr.NEG_ONE
BIG = tsd.BIG
SLICE = tsd.SLICE                  # 3000 constraints = 6 slices of 2 sub-blocks of 256, the last ragged
CAPS = [[BIG, BIG], [0, 0], [1, 3], [3, 1]]
HEAVY_MIN = 2048                   # csrc/lin_common.hpp: a constraint with more local terms takes one workgroup

_cache = {}


def copy_of(s, coefs=None):
    return lr.System(s.term_begin, s.slots, s.coef_idx, s.rhs_constraint, s.rhs_coef, s.coefs if coefs is None else coefs, s.first_random)


def rows_of(system, c):
    return {system.slots[t] // L for t in range(system.term_begin[c], system.term_begin[c + 1])}


def rhs_on_an_empty_constraint(system, entry):
    """b_c = table entry `entry` on the first constraint that has neither a term nor a right-hand side -> its number; the NEXT such
    constraint stays empty"""
    empty = [c for c in range(system.n_constraints) if system.term_begin[c] == system.term_begin[c + 1] and c not in set(system.rhs_constraint)]
    assert len(empty) >= 2 and system.coefs[entry] % P
    at = int(np.searchsorted(system.rhs_constraint, empty[0]))
    system.rhs_constraint.insert(at, empty[0])
    system.rhs_coef.insert(at, entry)
    return empty[0], empty[1]


def other_values(system, term_entry):
    """-> a table that differs from the system's own in one entry terms use and in one entry a right-hand side uses"""
    assert term_entry in system.coef_idx
    tab = list(system.coefs)
    tab[term_entry] = (tab[term_entry] + 1) % P
    e = system.rhs_coef[len(system.rhs_coef) // 3]
    tab[e] = (tab[e] + 9) % P
    return tab


def case_att():
    """the corrupted trace of tests/test_gpu_shard_diagnose.py (changed witness slots on LINEAR rows of rank 0 and of rank 1, a changed z
    slot, a changed right-hand side) and on top of it
      - a changed right-hand side in rank 1's slice of the right-hand sides on a constraint whose terms all lie on rows of rank 0, and one
        in rank 0's slice on a constraint whose terms all lie on rows of rank 1
      - a right-hand side b_c != 0 on a constraint without terms (violated: -b_c), next to a constraint that stays empty
      - "main_v": the same structure under another table (lig_shard_rows_set_linear_values)
      - "heavy": two constraints of 2300 terms, 2100 of them on rows of rank 0 (more than HEAVY_MIN LOCAL terms there) and 200 on a row of
        rank 1, the second through changed slots of both ranks"""
    if "att" in _cache:
        return _cache["att"]
    base = tsd.case_corrupted()
    kinds, rows, truth = base["kinds"], base["rows"], tsd.std_trace()[1]
    ranks = tsd.deal(kinds, 2)
    main = copy_of(base["systems"]["main"])
    n_rhs = len(main.rhs_constraint)
    crossed = []
    for holder, lo, hi in ((1, n_rhs // 2, n_rhs), (0, 0, n_rhs // 2)):          # lig_shard_rows_set_linear: rank g holds [g n_rhs / W, (g + 1) n_rhs / W)
        other = set(ranks[1 - holder])
        i = next(i for i in range(lo, hi) if rows_of(main, main.rhs_constraint[i]) and rows_of(main, main.rhs_constraint[i]) <= other
                 and main.rhs_constraint[i] != base["rhs_changed"])
        new = 3 if main.coefs[main.rhs_coef[i]] != main.coefs[3] else 4
        main.rhs_coef[i] = new
        crossed.append(main.rhs_constraint[i])
    no_terms, still_empty = rhs_on_an_empty_constraint(main, 5)
    main_v = copy_of(main, other_values(main, 20))
    rng = np.random.default_rng(14)
    victims = base["victims"]
    on0 = np.array(sorted(set(r * L + c for r in (0, 1, 2) for c in range(L)) - set(victims)))
    on1 = np.array(sorted(set(6 * L + c for c in range(L)) - set(victims)))
    b = tsd.Builder(truth)
    b.coefs = [3, P - 4, (1 << 200) + 9]
    expect_heavy = []
    for violated in (False, True):
        slots = list(rng.choice(on0, 2100)) + list(rng.choice(on1, 200))
        terms = [(int(s), [ONE, NEG_ONE, 0, 1, 2][int(ci)]) for s, ci in zip(slots, rng.integers(0, 5, 2300))]
        if violated:
            terms[1000] = (victims[0], ONE)                          # a changed slot of rank 0 ...
            terms[2200] = (victims[-1], ONE)                         # ... and one of rank 1
        cn = b.add(terms)
        assert sum(1 for s, _ in terms if s // L in ranks[0]) > HEAVY_MIN
        if violated:
            expect_heavy.append(cn)
        b.add([(int(rng.choice(on1)), ONE)])
    _cache["att"] = dict(kinds=kinds, rows=rows, systems={"main": main, "main_v": main_v, "heavy": b.system()}, tables={"main_v": main_v.coefs},
                         prove="main", crossed=crossed, no_terms=no_terms, still_empty=still_empty, expect_heavy=expect_heavy)
    return _cache["att"]


def case_satisfied():
    if "satisfied" not in _cache:
        kinds, rows, system = tsd.std_trace()
        _cache["satisfied"] = dict(kinds=kinds, rows=rows, systems={"main": system}, tables={}, prove="main")
    return _cache["satisfied"]


def case_w4():
    """three LINEAR rows, one each for ranks 0-2, none for rank 3 -- which still holds a quarter of the right-hand sides; violations on
    rows 0 and 2, a right-hand side without terms, another table"""
    if "w4" not in _cache:
        base = tsd.case_w4()
        main = copy_of(base["systems"]["main"])
        no_terms, still_empty = rhs_on_an_empty_constraint(main, 5)
        main_v = copy_of(main, other_values(main, 20))
        _cache["w4"] = dict(kinds=base["kinds"], rows=base["rows"], systems={"main": main, "main_v": main_v}, tables={"main_v": main_v.coefs}, prove="main",
                            no_terms=no_terms, still_empty=still_empty)
    return _cache["w4"]


def case_narrow():
    if "narrow" not in _cache:
        _cache["narrow"] = dict(tsd.case_narrow(), tables={})
    return _cache["narrow"]


CASES = {"att": case_att, "satisfied": case_satisfied, "w4": case_w4, "narrow": case_narrow}

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
    import linear_ref as lr
    import test_gpu_shard_diagnose as tsd
    import test_gpu_shard_diagnose_attached as tda
    g = dist.Group("gloo")
    ctx = pkg.Context(l, k, n, device=0)
    comm = g.make_comm(pkg, ctx)
    out = {"rank": g.rank, "shards": []}

    def ship(case):
        """-> (kinds | DRAW_PAD, this rank's rows as shipped, keyword arguments of begin, this rank's global rows)"""
        kinds, rows = case["kinds"], case["rows"]
        kk, msgs = np.asarray(kinds, dtype=np.uint8).copy(), rows.copy()
        draws = kk <= 3
        msgs[draws, l:] = 0xDEADBEEF
        kk[draws] |= pkg.ROW_DRAW_PAD
        rounds, b = pkg.shard_rows_plan(kinds, g.world)
        mine = pkg.local_rows_of(b, g.rank, g.world)
        assert [int(r) for r in mine] == tsd.deal(kinds, g.world)[g.rank]
        if "widths" in case:
            import test_gpu_mixed_rows as tm
            w, wd = case["widths"], case["wide"]
            return kk, tm.pack(pkg, msgs[mine], w[mine], wd[mine], l), dict(elem_bytes=w, wide_per_row=wd), mine
        return kk, (msgs[mine] if len(mine) else np.zeros((0, k, 8), dtype=np.uint32)), {}, mine

    def record(info, lin, quad):
        return {"counts": [int(info.n_linear_bad), int(info.n_linear_reported), int(info.n_quad_bad), int(info.n_quad_reported)],
                "lin": [[int(r["constraint"]), bytes(r["residual"]).hex()] for r in lin],
                "quad": [[int(r["row_x"]), int(r["row_y"]), int(r["row_z"]), int(r["column"]), bytes(r["residual"]).hex()] for r in quad]}

    def info_():
        i = pkg.DiagInfo(); i.struct_bytes = C.sizeof(pkg.DiagInfo); return i

    for step in plan:            # one shard per step: {"case", "calls": [[attached system, table name or null, lin_cap, quad_cap]], "misuse"}
        case = tda.CASES[step["case"]]()
        binds = {nm: s.to_binding(pkg) for nm, s in case["systems"].items()}
        kk, local, kw, mine = ship(case)
        sh = ctx.shard_rows_begin(kk, local, g.rank, g.world, comm, generated_at=lr.GEN, **kw)
        res = {"case": step["case"], "local_rows": len(mine), "calls": [], "with_system": []}
        main = binds[case["prove"]]
        ctx.shard_rows_set_linear(sh, main)
        attached, table = case["prove"], None
        call = lambda *a: ctx.L.lig_shard_rows_diagnose_attached(sh, *a)
        if step.get("misuse"):
            res["before_commit"] = call(None, 0, None, 0, C.byref(info_()))
        ctx.shard_rows_commit(sh)
        if step.get("misuse"):       # refused on the host before any collective: the calls below would hang or fail otherwise
            ctx.shard_rows_set_linear(sh, None)
            res["no_system"] = call(None, 0, None, 0, C.byref(info_()))
            ctx.shard_rows_set_linear(sh, main)
            res["null_lin"] = call(None, 5, None, 0, C.byref(info_()))
            res["null_quad"] = call(None, 0, None, 5, C.byref(info_()))
            short = info_(); short.struct_bytes -= 8
            res["short_info"] = call(None, 0, None, 0, C.byref(short))
        for nm, tab, lc, qc in step["calls"]:
            if nm != attached:
                ctx.shard_rows_set_linear(sh, binds[nm])
                attached, table = nm, None
            if tab != table:
                ctx.shard_rows_set_linear_values(sh, case["tables"][tab] if tab is not None else None)
                table = tab
            res["calls"].append(record(*ctx.shard_rows_diagnose_attached(sh, lin_cap=min(lc, 1 << 16), quad_cap=min(qc, 1 << 16))))
            res["with_system"].append(record(*ctx.shard_rows_diagnose(sh, binds[tab if tab is not None else nm], lin_cap=min(lc, 1 << 16), quad_cap=min(qc, 1 << 16))))
        if attached != case["prove"] or table is not None:
            ctx.shard_rows_set_linear(sh, main)
        proof, pinfo = ctx.shard_rows_prove(sh, None, None)
        res["proof"] = hashlib.sha256(proof).hexdigest()
        res["valid"] = [pinfo.valid_code, pinfo.valid_linear, pinfo.valid_quad]
        ctx.shard_destroy(sh)
        out["shards"].append(res)
    print(json.dumps(out))
    ctx.close()
    g.close()
''')


def expected(case, nm, tab, lc, qc):
    return tsd.expected(case, tab if tab is not None else nm, lc, qc)


def run_world(tmp_path, world, plan, **env):
    script = tmp_path / "shard_diagnose_attached_worker.py"
    script.write_text(WORKER)
    outs = mr.run_ranks(mr.python_argv(script, ROOT, json.dumps(plan)), world, mr.rendezvous_env(world, "ipc", **env), timeout=300)
    outs = sorted((mr.last_json(o) for o, _ in outs), key=lambda d: d["rank"])
    assert [o["rank"] for o in outs] == list(range(world))
    return outs


def check_calls(outs, plan):
    """every rank's bytes of every call == the Python restatement == lig_shard_rows_diagnose with the term list in the same world"""
    for si, step in enumerate(plan):
        case = CASES[step["case"]]()
        for ci, (nm, tab, lc, qc) in enumerate(step["calls"]):
            want = expected(case, nm, tab, lc, qc)
            print(step["case"], nm, tab, (lc, qc), "counts", want["counts"])
            for o in outs:
                got = o["shards"][si]["calls"][ci]
                assert got["counts"] == want["counts"], (o["rank"], nm, tab, lc, qc, got["counts"], want["counts"])
                assert got == want, "rank %d, call %d (%s / %s, caps %d / %d): records differ from the reference" % (o["rank"], ci, nm, tab, lc, qc)
                assert o["shards"][si]["with_system"][ci] == want, "rank %d, call %d: lig_shard_rows_diagnose differs from the reference" % (o["rank"], ci)


def calls_of(systems):
    return [[nm, tab, lc, qc] for nm, tab in systems for lc, qc in CAPS]


ATT_CALLS = calls_of([("main", None), ("main", "main_v"), ("heavy", None), ("main", None)])


def check_att_case():
    """what the case was built to contain is there, by the Python restatement"""
    case = case_att()
    bad = [c for c, _ in expected(case, "main", None, BIG, BIG)["lin"]]
    want = dict((c, r) for c, r in expected(case, "main", None, BIG, BIG)["lin"])
    main = case["systems"]["main"]
    assert set(case["crossed"]) <= set(bad) and case["no_terms"] in bad and case["still_empty"] not in bad
    b = main.coefs[main.rhs_coef[main.rhs_constraint.index(case["no_terms"])]]
    assert want[case["no_terms"]] == dr.residual_bytes(P - b).hex(), "a right-hand side without terms: the residual is -b_c"
    assert expected(case, "main", None, BIG, BIG)["counts"][2] == 1
    assert [c for c, _ in expected(case, "heavy", None, BIG, BIG)["lin"]] == case["expect_heavy"] == [2]
    assert expected(case, "main", "main_v", BIG, BIG)["lin"] != expected(case, "main", None, BIG, BIG)["lin"], "the other table gives another answer"
    return bad


def test_two_ranks_six_slices_every_case_and_the_refused_calls(tmp_path):
    """ipc, W = 2, LIG_DIAG_SLICE = 512: six slices of two sub-blocks of 256, the last ragged.  Changed slots on rows of both ranks, a changed
    z slot, right-hand sides held by the rank that holds none of the constraint's terms, b_c != 0 without terms, an empty constraint, the
    heavy path, another table in force; all caps; the refused calls leave the shard usable; a shard that was never diagnosed proves the
    same envelope"""
    plan = [dict(case="att", calls=ATT_CALLS, misuse=True), dict(case="att", calls=[])]
    outs = run_world(tmp_path, 2, plan, LIG_DIAG_SLICE=SLICE)
    bad = check_att_case()
    B = SLICE // 2
    assert len({c // SLICE for c in bad}) >= 3 and {c % SLICE // B for c in bad} == {0, 1}, "violations in several slices and in the sub-blocks of both owners"
    assert -(-case_att()["systems"]["main"].n_constraints // SLICE) == 6 and case_att()["systems"]["main"].n_constraints % SLICE
    check_calls(outs, plan)
    for o in outs:
        s = o["shards"][0]
        assert (s["before_commit"], s["no_system"], s["null_lin"], s["null_quad"], s["short_info"]) == (-3, -3, -1, -1, -1), s
        assert s["valid"] == [1, 0, 0], s
        assert s["proof"] == o["shards"][1]["proof"] == outs[0]["shards"][0]["proof"], "the envelope of a diagnosed shard differs from that of one that was not"


def test_two_ranks_one_slice_a_satisfied_trace_and_narrow_rows(tmp_path):
    """the slice knob at its default (one slice): a satisfied trace gives zero counts and its envelope is that of an undiagnosed shard;
    then 18 narrow rows with a derived LIG_ELEM_PRODUCT row and a mixed row among the slots the violated constraints touch"""
    plan = [dict(case="satisfied", calls=calls_of([("main", None)])), dict(case="satisfied", calls=[]),
            dict(case="narrow", calls=calls_of([("main", None)])), dict(case="att", calls=ATT_CALLS[:8])]
    outs = run_world(tmp_path, 2, plan)
    assert expected(case_satisfied(), "main", None, BIG, BIG)["counts"] == [0, 0, 0, 0]
    narrow = case_narrow()
    got = [c for c, _ in expected(narrow, "main", None, BIG, BIG)["lin"]]
    assert set(narrow["expect_lin"]) <= set(got) and narrow["spans_ok"] not in got
    check_calls(outs, plan)
    for o in outs:
        assert o["shards"][0]["valid"] == [1, 1, 1] and o["shards"][0]["proof"] == o["shards"][1]["proof"] == outs[0]["shards"][0]["proof"], o["rank"]


def test_four_ranks_one_without_rows(tmp_path):
    plan = [dict(case="w4", calls=calls_of([("main", None), ("main", "main_v")]))]
    outs = run_world(tmp_path, 4, plan, LIG_DIAG_SLICE=256)
    assert [o["shards"][0]["local_rows"] for o in outs] == [1, 1, 1, 0]
    case = case_w4()
    bad = [c for c, _ in expected(case, "main", None, BIG, BIG)["lin"]]
    assert len(bad) >= 7 and case["no_terms"] in bad and case["still_empty"] not in bad
    assert expected(case, "main", "main_v", BIG, BIG)["lin"] != expected(case, "main", None, BIG, BIG)["lin"]
    check_calls(outs, plan)


@pytest.mark.parametrize("force", [False, True])
def test_one_rank(tmp_path, force):
    """W = 1: lig_rows_diagnose_attached on the rank's matrix, its compact numbers read through the need list (no collective); once more
    with LIG_SHARD_FORCE_EXCHANGE, through the exchange path"""
    plan = [dict(case="att", calls=ATT_CALLS, misuse=True), dict(case="att", calls=[])]
    env = dict(LIG_DIAG_SLICE=SLICE)
    if force:
        env["LIG_SHARD_FORCE_EXCHANGE"] = 1
    outs = run_world(tmp_path, 1, plan, **env)
    check_att_case()
    check_calls(outs, plan)
    s = outs[0]["shards"][0]
    assert (s["before_commit"], s["no_system"], s["null_lin"], s["null_quad"], s["short_info"]) == (-3, -3, -1, -1, -1), s
    assert s["proof"] == outs[0]["shards"][1]["proof"]
