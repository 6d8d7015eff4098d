"""GPU: lig_shard_rows_explain_slots* / lig_shard_rows_untouched_slots* -- from a slot of a SHARDED rows job to the constraints through it, and
the witness slots no term touches (csrc/diagnose.hip, csrc/shard.hip): the rank that was dealt a slot's row collects its terms from its own
compactly numbered share, every rank receives all of them, and the sizes and residuals come from lig_shard_rows_explain_attached itself.
W ranks as W processes on the one GPU, collectives over comm_ipc or gloo callbacks; traces, the deal, the Builders and the cases are those
of tests/test_gpu_shard_diagnose*.py and tests/test_gpu_explain_slots.py, imported, not copied -- `slots` below is a sibling of slots_case
with a second hot slot on a row of the other rank.

Expected bytes never come from the library: tests/slots_ref.py restates the records in Python integers over the WHOLE row matrix, with the
system under the table in force, here in the parent, and the parent compares every field of every rank's output with it.  Three more
checks by byte digest, made in the worker: the term-list form in the same world, on rank 0 the one-GPU call on a trace of the same rows,
and the residuals against lig_shard_rows_explain_attached in the same world.  Every world makes several calls, so the file stays at six
world launches.  No test hands a kernel an invalid index (the misuse calls launch nothing) and none provokes a communicator failure;
every rank process is bounded by run_ranks' timeout."""
import collections
import json
import os
import textwrap

import numpy as np
import pytest

import linear_ref as lr
import multirank as mr
import oracle_lib as ol
import slots_ref as sr
import test_gpu_shard_diagnose as tsd
import test_gpu_shard_diagnose_attached as tda
from test_gpu_explain import HEAVY_MIN, Builder, base_trace, bump, shapes_case, wit, with_table
from test_gpu_explain_slots import slots_case
from test_gpu_shard_explain import owners

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

P = ol.P
L = tsd.L
ONE, NEG_ONE = lr.ONE, lr.NEG_ONE
BIG = 1 << 15                      # a term cap nothing here reaches (the binding allocates the records)
E_ARG, E_STATE = -1, -3
_cache = {}


def slots_trace_case():
    """slots_case on the 12-row base trace [L L L L L | X Y Z | L | X Y Z] (two ranks: rows 0-7 and 8-11; four: rows 0-2, 3-7, 8-11 and
    none), with one more hot slot: `exact` (HEAVY_MIN terms) lies on a LINEAR row of rank 0, `over1` (HEAVY_MIN + 1 terms over three
    constraints) on the QX row 9 of rank 1; `over` and `hot` of slots_case stay.  Untouched slots of rows of both ranks are zeroed (no
    constraint sees them).
    "T2": another table; "other": another statement on the same rows (shapes_case)"""
    kinds, truth = base_trace()
    assert [int(kd) for kd in kinds] == [0, 0, 0, 0, 0, 1, 2, 3, 0, 1, 2, 3] and tsd.deal(kinds, 2) == [list(range(8)), list(range(8, 12))]
    assert tsd.deal(kinds, 4) == [[0, 1, 2], [3, 4, 5, 6, 7], [8, 9, 10, 11], []]
    base, names = slots_case()
    rhs = dict(zip(base.rhs_constraint, base.rhs_coef))
    b = Builder(truth)
    for c in range(base.n_constraints):                           # replayed as it stands
        b.add([(base.slots[t], base.coef_idx[t]) for t in range(base.term_begin[c], base.term_begin[c + 1])], b=base.coef(rhs[c]) if c in rhs else 0)
    used = collections.Counter(base.slots)
    over1 = next(s for s in range(9 * L, 10 * L - 40) if s not in used and s + 40 not in used)
    picks = [ONE, NEG_ONE, 3, 4, 5, 7]
    rng = np.random.default_rng(78)
    for n in (1000, 700, HEAVY_MIN + 1 - 1700):                   # three constraints, each with a neighbour slot in the middle
        b.add([(over1, picks[int(ci)]) for ci in rng.integers(0, 6, n // 2)] + [(over1 + 40, 2)] + [(over1, picks[int(ci)]) for ci in rng.integers(0, 6, n - n // 2)])
    system = b.system()
    count = collections.Counter(system.slots)
    names = dict(names, over1=over1)
    assert count[names["exact"]] == HEAVY_MIN and count[over1] == HEAVY_MIN + 1 and count[names["over"]] == HEAVY_MIN + 1 and count[names["none"]] == 0
    rows = truth.copy()
    free = [s for s in range(12 * L) if not count[s]]
    zeroed = [s for s in free if s // L == 1][:20] + [s for s in free if s // L == 9][:15] + [s for s in free if s // L == 11][:3]
    for s in zeroed:
        rows[s // L, s % L] = 0
    T2 = list(system.coefs)
    T2[4] = (T2[4] + 6) % P                                       # a term coefficient (index 4: slot 700 among others) ...
    T2[system.rhs_coef[0]] = (T2[system.rhs_coef[0]] + 1) % P     # ... and one right-hand side
    other, _ = shapes_case()
    return dict(kinds=kinds, rows=rows, systems={"main": system, "T2": with_table(system, T2), "other": other}, tables={"T2": T2}, prove="main",
                names=names, zeroed=zeroed)


def bumped_case():
    """the same statement on a witness with four changed slots: 700, a hot slot of each rank, and one no constraint touches"""
    base = case_of("slots")
    rows = base["rows"].copy()
    nm = base["names"]
    for s, d in ((700, 5), (nm["over"], 3), (nm["over1"], 4), (nm["none"], 9)):
        bump(rows, s, d)
    return dict(base, rows=rows)


def case_of(name):
    """slots / bumped made here; att, w4, narrow of tests/test_gpu_shard_diagnose_attached.py; gloo, batch of tests/test_gpu_shard_diagnose.py"""
    if name not in _cache:
        if name == "slots":
            _cache[name] = slots_trace_case()
        elif name == "bumped":
            _cache[name] = bumped_case()
        elif name in tda.CASES:
            _cache[name] = tda.CASES[name]()
        else:
            _cache[name] = dict(tsd.CASES[name](), tables={})
    return _cache[name]


WORKER = textwrap.dedent('''
    import ctypes as C, hashlib, importlib.util, json, os, sys
    import numpy as np
    root, plan = sys.argv[1], json.load(open(sys.argv[2]))
    l, k, n = 320, 512, 2048
    sys.path.insert(0, os.path.join(root, "tests"))
    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, "ligero-prover_amd", rel))
        m = importlib.util.module_from_spec(spec); sys.modules[name] = m; spec.loader.exec_module(m); return m
    pkg = load("ligero_prover_amd", "__init__.py")
    dist = load("lig_dist", "dist.py")
    import linear_ref as lr
    import test_gpu_shard_diagnose as tsd
    import test_gpu_shard_explain_slots as tes
    g = dist.Group("gloo")
    ctx = pkg.Context(l, k, n, device=0)
    comm = g.make_comm(pkg, ctx)
    out = {"rank": g.rank, "shards": []}
    hp = pkg._hptr
    E_STATE = -3

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

    def sinfo(short=0):
        i = pkg.SlotInfo(); i.struct_bytes = C.sizeof(pkg.SlotInfo) - short; return i
    def uinfo(short=0):
        i = pkg.UntouchedInfo(); i.struct_bytes = C.sizeof(pkg.UntouchedInfo) - short; return i

    def slots_digest(info, rec, terms):
        raw = rec.tobytes() + terms.tobytes() + bytes([0]) + str((int(info.n_terms_total), int(info.n_terms_reported), int(info.n_constraints_distinct))).encode()
        return hashlib.sha256(raw).hexdigest()
    def untouched_digest(info, vals):
        raw = vals.tobytes() + bytes([1]) + str((int(info.n_untouched), int(info.n_untouched_nonzero), int(info.n_reported))).encode()
        return hashlib.sha256(raw).hexdigest()

    def slots_record(info, rec, terms):
        """every field of every record, the 32-byte fields as indices into a table of hex strings, and a digest of the raw bytes"""
        table, at = [], {}
        def ix(b):
            h = bytes(b).hex()
            if h not in at:
                at[h] = len(table); table.append(h)
            return at[h]
        return {"counts": [int(info.n_terms_total), int(info.n_terms_reported), int(info.n_constraints_distinct)],
                "slots": [[int(r["slot"]), int(r["row_kind"]), int(r["n_terms"]), int(r["first_term"]), ix(r["value"])] for r in rec],
                "terms": [[int(t["slot"]), int(t["constraint"]), int(t["coef_index"]), int(t["constraint_terms"]), ix(t["coef"]), ix(t["residual"])] for t in terms],
                "hex": table, "digest": slots_digest(info, rec, terms)}
    def untouched_record(info, vals):
        return {"counts": [int(info.n_untouched), int(info.n_untouched_nonzero), int(info.n_reported)],
                "values": [[int(v["slot"]), int(v["row_kind"]), bytes(v["value"]).hex()] for v in vals], "digest": untouched_digest(info, vals)}

    for step in plan:            # one shard per step: {"case", "calls": [{op, att, tab, asked / nz, cap, list}], "misuse", "synthetic", "after_prove"}
        case = tes.case_of(step["case"])
        binds = {nm: s.to_binding(pkg) for nm, s in case["systems"].items()}
        kk, msgs, local, kw, mine = ship(case)
        S = len(case["kinds"]) * l
        sh = ctx.shard_rows_begin(kk, local, g.rank, g.world, comm, generated_at=lr.GEN, **kw)
        res = {"case": step["case"], "local_rows": len(mine), "calls": []}
        main = binds[case["prove"]]
        two = np.array([0, 1], dtype=np.uint32)
        rec2, terms8, vals8 = np.zeros(2, dtype=pkg.SLOT_RECORD), np.zeros(8, dtype=pkg.SLOT_TERM), np.zeros(8, dtype=pkg.SLOT_VALUE)
        X = lambda *a: ctx.L.lig_shard_rows_explain_slots_attached(sh, *a)
        XL = lambda sysb, *a: ctx.L.lig_shard_rows_explain_slots(sh, C.byref(sysb) if sysb is not None else None, *a)
        U = lambda *a: ctx.L.lig_shard_rows_untouched_slots_attached(sh, *a)
        UL = lambda sysb, *a: ctx.L.lig_shard_rows_untouched_slots(sh, C.byref(sysb) if sysb is not None else None, *a)
        def all_four():
            return [X(hp(two), 2, hp(rec2), hp(terms8), 8, C.byref(sinfo())), XL(main, hp(two), 2, hp(rec2), hp(terms8), 8, C.byref(sinfo())),
                    U(0, hp(vals8), 8, C.byref(uinfo())), UL(main, 1, hp(vals8), 8, C.byref(uinfo()))]
        ctx.shard_rows_set_linear(sh, main)
        attached, table = case["prove"], None
        if step.get("misuse"):
            res["before_commit"] = all_four()
        ctx.shard_rows_commit(sh)
        if step.get("misuse"):       # refused on the host before any launch and any collective: the calls below would hang or fail otherwise
            ctx.shard_rows_set_linear(sh, None)
            no_system = [X(hp(two), 2, hp(rec2), hp(terms8), 8, C.byref(sinfo())), U(0, hp(vals8), 8, C.byref(uinfo()))]
            ctx.shard_rows_set_linear(sh, main)
            system = case["systems"][case["prove"]]
            bad_sys = system.to_binding(pkg, slots=[S] + list(system.slots[1:]))      # a slot out of range: lig_linear_check rejects it
            i0 = sinfo(); i0.n_terms_total = 7; i0.n_terms_reported = 7; i0.n_constraints_distinct = 7
            arg = {}
            for name, asked in (("not_ascending", [3, 2]), ("repeated", [2, 2]), ("equal_to_rows_times_l", [0, S]), ("beyond", [0xFFFFFFFF])):
                a = np.array(asked, dtype=np.uint32)
                arg[name] = [X(hp(a), len(a), hp(rec2), hp(terms8), 8, C.byref(sinfo())), XL(main, hp(a), len(a), hp(rec2), hp(terms8), 8, C.byref(sinfo()))]
            arg["null_slots"] = [X(None, 2, hp(rec2), hp(terms8), 8, C.byref(sinfo())), XL(main, None, 2, hp(rec2), hp(terms8), 8, C.byref(sinfo()))]
            arg["null_slot_out"] = [X(hp(two), 2, None, hp(terms8), 8, C.byref(sinfo())), XL(main, hp(two), 2, None, hp(terms8), 8, C.byref(sinfo()))]
            arg["null_terms"] = [X(hp(two), 2, hp(rec2), None, 8, C.byref(sinfo())), XL(main, hp(two), 2, hp(rec2), None, 8, C.byref(sinfo()))]
            arg["null_info"] = [X(hp(two), 2, hp(rec2), hp(terms8), 8, None), XL(main, hp(two), 2, hp(rec2), hp(terms8), 8, None), U(0, hp(vals8), 8, None),
                                UL(main, 0, hp(vals8), 8, None)]
            arg["short_info"] = [X(hp(two), 2, hp(rec2), hp(terms8), 8, C.byref(sinfo(8))), XL(main, hp(two), 2, hp(rec2), hp(terms8), 8, C.byref(sinfo(8))),
                                 U(0, hp(vals8), 8, C.byref(uinfo(8))), UL(main, 0, hp(vals8), 8, C.byref(uinfo(8)))]
            arg["null_out"] = [U(0, None, 8, C.byref(uinfo())), UL(main, 0, None, 8, C.byref(uinfo()))]
            arg["null_sys"] = [XL(None, hp(two), 2, hp(rec2), hp(terms8), 8, C.byref(sinfo())), XL(None, None, 0, None, None, 0, C.byref(sinfo())),
                               UL(None, 0, hp(vals8), 8, C.byref(uinfo()))]
            arg["rejected_sys"] = [XL(bad_sys, hp(two), 2, hp(rec2), hp(terms8), 8, C.byref(sinfo())), XL(bad_sys, None, 0, None, None, 0, C.byref(sinfo())),
                                   UL(bad_sys, 0, hp(vals8), 8, C.byref(uinfo()))]
            res["misuse"] = {"no_system": no_system, "arg": arg,
                             "nothing_asked": [X(None, 0, None, None, 0, C.byref(i0)), int(i0.n_terms_total), int(i0.n_terms_reported), int(i0.n_constraints_distinct),
                                               XL(main, None, 0, None, None, 0, C.byref(sinfo()))]}
        if step.get("synthetic"):    # a shard not made by lig_shard_rows_begin (one rank only: nothing collective is involved)
            syn = ctx.shard_prepare(pkg.Context.make_job(700, 0, generated_at=77), 0, 1, comm)
            res["synthetic"] = [ctx.L.lig_shard_rows_explain_slots_attached(syn, hp(two), 2, hp(rec2), hp(terms8), 8, C.byref(sinfo())),
                                ctx.L.lig_shard_rows_explain_slots(syn, C.byref(main), hp(two), 2, hp(rec2), hp(terms8), 8, C.byref(sinfo())),
                                ctx.L.lig_shard_rows_untouched_slots_attached(syn, 0, hp(vals8), 8, C.byref(uinfo())),
                                ctx.L.lig_shard_rows_untouched_slots(syn, C.byref(main), 0, hp(vals8), 8, C.byref(uinfo()))]
            ctx.shard_destroy(syn)

        def in_force(call):
            global attached, table
            if call["att"] != attached:
                ctx.shard_rows_set_linear(sh, binds[call["att"]])
                attached, table = call["att"], None
            if call["tab"] != table:
                ctx.shard_rows_set_linear_values(sh, case["tables"][call["tab"]] if call["tab"] is not None else None)
                table = call["tab"]
            return binds[call["list"] or call["tab"] or call["att"]]

        def run_calls(calls):
            got = []
            for call in calls:
                sysb = in_force(call)
                if call["op"] == "slots":
                    info, rec, terms = ctx.shard_rows_explain_slots_attached(sh, call["asked"], term_cap=call["cap"])
                    r = slots_record(info, rec, terms)
                    # the residuals and sizes in the slot terms against lig_shard_rows_explain_attached of the same constraints in the same world
                    distinct = sorted({int(t["constraint"]) for t in terms})
                    if distinct:
                        _, con, _ = ctx.shard_rows_explain_attached(sh, distinct, term_cap=0)
                        shown = {int(c["constraint"]): (int(c["n_terms"]), bytes(c["residual"])) for c in con}
                        r["residuals_are_explain_attached"] = all((int(t["constraint_terms"]), bytes(t["residual"])) == shown[int(t["constraint"])] for t in terms)
                    with_list = ctx.shard_rows_explain_slots(sh, sysb, call["asked"], term_cap=call["cap"])
                    r["with_list"] = slots_record(*with_list) if call["list"] else slots_digest(*with_list)
                else:
                    info, vals = ctx.shard_rows_untouched_slots_attached(sh, nonzero_only=call["nz"], cap=call["cap"])
                    r = untouched_record(info, vals)
                    with_list = ctx.shard_rows_untouched_slots(sh, sysb, nonzero_only=call["nz"], cap=call["cap"])
                    r["with_list"] = untouched_record(*with_list) if call["list"] else untouched_digest(*with_list)
                got.append(r)
            return got

        touch = bool(step.get("calls"))     # no calls: a shard that is never asked (its envelope is the yardstick of the others')
        if touch:
            res["calls"] = run_calls(step["calls"])
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
            again = [(i, c) for i, c in enumerate(step["calls"]) if c["att"] == case["prove"] and c["tab"] is None and not c["list"]]
            ex = run_calls([c for _, c in again])
            res["after_prove_same"] = bool(again) and [a["digest"] for a in ex] == [res["calls"][i]["digest"] for i, _ in again]
        if step.get("misuse"):
            ctx.shard_rows_restart(sh, local)
            res["after_restart"] = all_four()
        ctx.shard_destroy(sh)
        if g.rank == 0 and touch:      # the third check: the one-GPU calls on a trace of the same rows, one trace per attached system
            one, traces = [], {}
            for call in step["calls"]:
                nm, tab = call["att"], call["tab"]
                if nm not in traces:
                    tr, keep = ctx.rows_begin(kk, msgs, generated_at=lr.GEN, **kw)
                    ctx.rows_set_linear(tr, binds[nm])
                    ctx.rows_commit(tr)
                    traces[nm] = [tr, keep, None]
                if traces[nm][2] != tab:
                    ctx.rows_set_linear_values(traces[nm][0], case["tables"][tab] if tab is not None else None)
                    traces[nm][2] = tab
                if call["op"] == "slots":
                    one.append(slots_digest(*ctx.rows_explain_slots_attached(traces[nm][0], call["asked"], term_cap=call["cap"])))
                else:
                    one.append(untouched_digest(*ctx.rows_untouched_slots_attached(traces[nm][0], nonzero_only=call["nz"], cap=call["cap"])))
            res["one_gpu"] = one
            for tr, _, _ in traces.values():
                ctx.trace_destroy(tr)
        out["shards"].append(res)
    print(json.dumps(out))
    ctx.close()
    g.close()
''')


def slots_call(att, asked, cap=BIG, tab=None, list_=None):
    return dict(op="slots", att=att, tab=tab, asked=[int(s) for s in asked], cap=int(cap), list=list_)


def untouched_call(att, nz, cap, tab=None, list_=None):
    return dict(op="untouched", att=att, tab=tab, nz=bool(nz), cap=int(cap), list=list_)


def run_world(tmp_path, world, comm, plan, **env):
    script, plan_file = tmp_path / "shard_explain_slots_worker.py", tmp_path / "plan.json"
    script.write_text(WORKER)
    plan_file.write_text(json.dumps(plan))
    outs = mr.run_ranks(mr.python_argv(script, ROOT, plan_file), world, mr.rendezvous_env(world, comm, **env), timeout=300)
    outs = sorted((mr.last_json(o) for o, _ in outs), key=lambda d: d["rank"])
    assert [o["rank"] for o in outs] == list(range(world))
    return outs


_want = {}


def want_slots(case_name, sysname, asked, cap):
    """the Python restatement over the whole matrix with the system under the table in force: computed once per asked list, cut at cap"""
    key = (case_name, sysname, tuple(asked))
    if key not in _want:
        case = case_of(case_name)
        _want[key] = sr.explain_slots(case["systems"][sysname], case["kinds"], case["rows"], L, asked, 1 << 40)
    total, _, distinct, recs, terms = _want[key]
    return [total, min(total, cap), distinct], recs, terms[:cap]


def want_untouched(case_name, sysname, nz, cap):
    key = (case_name, sysname, "untouched", bool(nz))
    if key not in _want:
        case = case_of(case_name)
        _want[key] = sr.untouched(case["systems"][sysname], case["kinds"], case["rows"], L, nz, 1 << 40)
    n, nonzero, _, vals = _want[key]
    return [n, nonzero, min(len(vals), cap)], vals[:cap]


def decoded_slots(r):
    h = [bytes.fromhex(x) for x in r["hex"]]
    return r["counts"], [(s, kd, nt, ft, h[v]) for s, kd, nt, ft, v in r["slots"]], [(s, c, ci, ct, h[a], h[res]) for s, c, ci, ct, a, res in r["terms"]]


def decoded_untouched(r):
    return r["counts"], [(s, kd, bytes.fromhex(v)) for s, kd, v in r["values"]]


def check_step(outs, si, step):
    """every rank's output of every call of the step == the reference, field by field; the term-list form on the same rank returns the same
    bytes (or, with `list`, the reference of THAT system); the residuals are those of lig_shard_rows_explain_attached; rank 0's one-GPU
    call returns the same bytes; every rank the same bytes"""
    name = step["case"]
    for o in outs:
        got = o["shards"][si]
        assert len(got["calls"]) == len(step["calls"])
        for ci, call in enumerate(step["calls"]):
            g = got["calls"][ci]
            in_force = call["tab"] or call["att"]
            where = "rank %d, call %d (%s %s / %s, cap %d)" % (o["rank"], ci, call["op"], call["att"], call["tab"], call["cap"])
            if call["op"] == "slots":
                want = want_slots(name, in_force, call["asked"], call["cap"])
                counts, recs, terms = decoded_slots(g)
                print(where, "counts", counts, "want", want[0])
                assert counts == want[0], where
                assert recs == want[1], where + ": slot records differ from the reference"
                assert terms == want[2], where + ": term records differ from the reference"
                assert g.get("residuals_are_explain_attached", True) is True, where + ": residuals differ from lig_shard_rows_explain_attached"
                if call["list"]:
                    lc, lrecs, lterms = decoded_slots(g["with_list"])
                    lwant = want_slots(name, call["list"], call["asked"], call["cap"])
                    assert (lc, lrecs, lterms) == lwant, where + ": the term-list form differs from the reference of its own system"
            else:
                want = want_untouched(name, in_force, call["nz"], call["cap"])
                counts, vals = decoded_untouched(g)
                print(where, "counts", counts, "want", want[0])
                assert counts == want[0], where
                assert vals == want[1], where + ": untouched records differ from the reference"
                if call["list"]:
                    assert decoded_untouched(g["with_list"]) == want_untouched(name, call["list"], call["nz"], call["cap"]), where
            if not call["list"]:
                assert g["with_list"] == g["digest"], where + ": the term-list form returns other bytes"
            assert g["digest"] == outs[0]["shards"][si]["calls"][ci]["digest"], where + ": other bytes than rank 0"
        if step.get("after_prove"):
            assert got["after_prove_same"] is True, "rank %d: the calls after the proof return other bytes" % o["rank"]
    s0 = outs[0]["shards"][si]
    assert s0["one_gpu"] == [c["digest"] for c in s0["calls"]], "the one-GPU call on a trace of the same rows returns other bytes"


def m_of(case, sysname, asked, world):
    """m_r: the terms through the asked slots on rows of rank r"""
    own, count = owners(case, world), collections.Counter(case["systems"][sysname].slots)
    m = [0] * world
    for s in asked:
        m[own[s // L]] += count[s]
    return m


def untouched_by_rank(case_name, sysname, world, nz=False):
    own = owners(case_of(case_name), world)
    _, vals = want_untouched(case_name, sysname, nz, 1 << 40)
    return [sum(1 for s, _, _ in vals if own[s // L] == r) for r in range(world)]


def hottest(system):
    return collections.Counter(system.slots).most_common(1)[0][0]


def slots_lists():
    case = case_of("slots")
    nm, own = case["names"], owners(case, 2)
    every = sorted(nm.values())
    on0 = [s for s in every if own[s // L] == 0]
    return case, nm, own, every, on0


def test_two_ranks_lists_caps_pieces_values_forms_untouched_envelope_and_misuse(tmp_path):
    """ipc, W = 2, pieces of 1024 items.  Asked lists: slots on both ranks with both hot slots (exactly HEAVY_MIN terms on rank 0, HEAVY_MIN + 1
    on rank 1), all on one rank, a slot without a term, the last slot of the trace; every term_cap; three pieces and more with a ragged last
    one, and M an exact multiple of P; another table in force and the system's own again; the term-list form with another system attached;
    untouched slots with every cap; the misuse calls, which launch nothing and leave no collective half-issued; the same bytes after the
    proof; the envelope of an untouched shard; a bumped witness"""
    case, nm, own, every, on0 = slots_lists()
    assert own[nm["exact"] // L] == 0 and own[nm["over1"] // L] == 1 and own[nm["hot"] // L] == 1 and own[nm["last"] // L] == 1
    assert {own[s // L] for s in every} == {0, 1} and len(on0) >= 4
    m = m_of(case, "main", every, 2)
    P_ = 1024
    assert -(-max(m) // P_) >= 3 and max(m) % P_ and min(m) > 0, m                     # at least three pieces, the last one ragged
    assert m_of(case, "main", [nm["exact"]], 2) == [HEAVY_MIN, 0] and HEAVY_MIN % P_ == 0     # M an exact multiple of P; rank 1 sends nothing but padding
    counts, recs, _ = want_slots("slots", "main", every, BIG)
    total = counts[0]
    first = {s: ft for s, _, _, ft, _ in recs}
    assert total == sum(m) < BIG
    caps = [0, 1, first[nm["exact"]] + 1000, first[nm["over1"]] + HEAVY_MIN, total - 1, total, total + 5]      # inside two heavy segments
    calls = [slots_call("main", every, cap) for cap in caps]
    calls += [slots_call("main", on0), slots_call("main", [nm["none"]]), slots_call("main", [nm["last"]]), slots_call("main", [nm["exact"]]),
              slots_call("main", [nm["none"], nm["last"]], 0)]
    t2 = len(calls)
    calls += [slots_call("main", every, tab="T2"), slots_call("main", every)]                                    # other values in force, and back
    other_at = len(calls)
    calls += [slots_call("other", every, list_="main"), slots_call("other", every)]                              # the term list of `main` with `other` attached
    n, nz, _ = want_untouched("slots", "main", False, 0)[0]
    per_rank = untouched_by_rank("slots", "main", 2)
    assert per_rank[0] > 10 and per_rank[1] > 10 and sum(per_rank) == n and 0 < nz < n
    u_at = len(calls)
    for nzo in (False, True):
        sel = nz if nzo else n
        for cap in (0, 1, per_rank[0] // 2, per_rank[0] + 5, sel, sel + 5):          # inside rank 0's list, inside rank 1's
            calls.append(untouched_call("main", nzo, cap))
    calls += [untouched_call("main", True, 50, tab="T2"), untouched_call("other", False, 100, list_="main")]
    bumped = case_of("bumped")
    bumped_asked = sorted({700, nm["over"], nm["over1"], nm["none"], nm["hot"], 9, nm["last"]})
    plan = [dict(case="slots", calls=calls, misuse=True, after_prove=True), dict(case="slots", calls=[]),
            dict(case="bumped", calls=[slots_call("main", bumped_asked), slots_call("main", bumped_asked, 7)])]
    outs = run_world(tmp_path, 2, "ipc", plan, LIG_DIAG_SLICE=P_)
    for o in outs:
        s = o["shards"][0]
        assert s["before_commit"] == [E_STATE] * 4 and s["after_restart"] == [E_STATE] * 4, s
        mis = s["misuse"]
        assert mis["no_system"] == [E_STATE, E_STATE] and mis["nothing_asked"] == [0, 0, 0, 0, 0], mis
        assert len(mis["arg"]) == 12 and all(set(v) == {E_ARG} for v in mis["arg"].values()), mis["arg"]
        assert s["proof"] == o["shards"][1]["proof"] == outs[0]["shards"][0]["proof"], "an asked shard must produce the envelope of one that was not"
        assert s["valid"] == o["shards"][1]["valid"]
        d = [c["digest"] for c in s["calls"]]
        assert d[t2 + 1] == d[caps.index(total)] != d[t2], "the system's own values again after None"
        assert d[other_at + 1] != d[t2 + 1], "another statement attached gives other bytes"
    for si in range(3):
        if plan[si]["calls"]:
            check_step(outs, si, plan[si])
    full = want_slots("slots", "main", every, BIG)
    by = {s: (kd, nt) for s, kd, nt, _, _ in full[1]}
    assert [by[nm[k]][1] for k in ("none", "exact", "over", "over1", "hot")] == [0, HEAVY_MIN, HEAVY_MIN + 1, HEAVY_MIN + 1, HEAVY_MIN + 3]
    assert [by[nm[k]][0] for k in ("first", "qx", "qy", "qz", "over1", "last")] == [0, 1, 2, 3, 1, 3]
    other = want_slots("slots", "T2", every, BIG)
    assert other[2] != full[2] and other[1] == full[1], "the other table gives other coefficient values and residuals, the same slot records"
    # untouched: the counts are complete whatever cap is; the zeroed slots drop out of nonzero_only alone
    zeroed = set(case["zeroed"])
    assert zeroed <= {s for s, _, _ in want_untouched("slots", "main", False, 1 << 40)[1]}
    assert not zeroed & {s for s, _, _ in want_untouched("slots", "main", True, 1 << 40)[1]}
    for o in outs:
        for c in o["shards"][0]["calls"][u_at:u_at + 12]:
            assert c["counts"][:2] == [n, nz]
    # the bumped witness: every constraint through a changed slot is violated, the slot no constraint touches changes nothing
    _, recs, terms = want_slots("bumped", "main", bumped_asked, BIG)
    through = lambda s: [t for t in terms if t[0] == s]
    zero = bytes(32)
    assert through(700) and all(t[5] != zero for t in through(700) + through(nm["over"]) + through(nm["over1"]))
    assert len({t[5] for t in through(nm["over1"])}) == 3 and not through(nm["none"])
    assert [t[5] != zero for t in through(9)] == [True], "slot 9 shares the violated constraint of slot 700"
    value = {s: v for s, _, _, _, v in recs}
    assert value[700] == sr.le32(wit(bumped["rows"], 700)) != sr.le32(wit(case["rows"], 700))
    assert all(c.get("residuals_are_explain_attached") is True for o in outs for c in o["shards"][2]["calls"])


def test_four_ranks_and_one_without_rows(tmp_path):
    """W = 4 over ipc, pieces of 300: the 12-row trace (rows 0-2, 3-7, 8-11: the hot slots on ranks 0 and 2) and the three-row trace; in both
    rank 3 was dealt no row: m_r = 0, no untouched slot, its share is empty -- and it returns the same bytes as everybody"""
    case = case_of("slots")
    nm = case["names"]
    every = sorted(nm.values())
    own = owners(case, 4)
    assert sorted({own[s // L] for s in every}) == [0, 1, 2] and (own[nm["exact"] // L], own[nm["over1"] // L], own[nm["hot"] // L]) == (0, 2, 2)
    n, nz, _ = want_untouched("slots", "main", False, 0)[0]
    per_rank = untouched_by_rank("slots", "main", 4)
    w4 = case_of("w4")
    system = w4["systems"]["main"]
    used = sorted(set(system.slots))
    rng = np.random.default_rng(5)
    free = next(s for s in range(3 * L) if s not in set(used))
    asked4 = sorted({int(s) for s in rng.choice(used, 40, replace=False)} | {hottest(system), free, 0, 3 * L - 1})
    assert tsd.deal(w4["kinds"], 4)[3] == [] and m_of(w4, "main", asked4, 4)[3] == 0
    n4 = want_untouched("w4", "main", False, 0)[0][0]
    plan = [dict(case="slots", calls=[slots_call("main", every), slots_call("main", every, 3000), untouched_call("main", False, per_rank[0] + per_rank[1] + 3),
                                      untouched_call("main", True, n)]),
            dict(case="w4", calls=[slots_call("main", asked4), slots_call("main", asked4, 5), slots_call("main", asked4, tab="main_v"), slots_call("main", [free]),
                                   untouched_call("main", False, n4 + 5), untouched_call("main", False, 7), untouched_call("main", True, 0)], after_prove=True)]
    outs = run_world(tmp_path, 4, "ipc", plan, LIG_DIAG_SLICE=300)
    assert [o["shards"][0]["local_rows"] for o in outs] == [3, 5, 4, 0] and [o["shards"][1]["local_rows"] for o in outs] == [1, 1, 1, 0]
    check_step(outs, 0, plan[0])
    check_step(outs, 1, plan[1])
    assert want_slots("w4", "main", [free], BIG)[0] == [0, 0, 0], "no term anywhere: no item all-gather and no inner call on any rank"
    assert n4 > 0


def test_host_synchronous_collectives_over_gloo(tmp_path):
    """the callbacks of a gloo group, pieces of 8: the corrupted trace of tests/test_gpu_shard_diagnose_attached.py -- changed slots on rows of
    both ranks, the hottest slot, slots nothing touches"""
    case = case_of("att")
    system = case["systems"]["main"]
    used = sorted(set(system.slots))
    rng = np.random.default_rng(9)
    free = [s for s in range(10 * L) if s not in set(used)]
    asked = sorted({int(s) for s in rng.choice(used, 30, replace=False)} | {hottest(system), free[0], free[-1], 0, 10 * L - 1})
    m = m_of(case, "main", asked, 2)
    assert min(m) > 8 and m[0] != m[1], m
    n = want_untouched("att", "main", False, 0)[0][0]
    plan = [dict(case="att", calls=[slots_call("main", asked), slots_call("main", asked, 3), slots_call("main", asked, 0), slots_call("main", asked, tab="main_v"),
                                    untouched_call("main", False, n), untouched_call("main", True, 11)], after_prove=True)]
    outs = run_world(tmp_path, 2, None, plan, LIG_DIAG_SLICE=8)
    check_step(outs, 0, plan[0])
    zero = bytes(32)
    terms = want_slots("att", "main", asked, BIG)[2]
    assert any(t[5] != zero for t in terms) and any(t[5] == zero for t in terms), "violated and satisfied constraints through the asked slots"


def test_one_rank_without_and_with_the_forced_exchange(tmp_path):
    """W = 1: the passes over the rank's compactly numbered share without a collective; once more with LIG_SHARD_FORCE_EXCHANGE, through the
    exchange path with one rank: the same bytes.  A shard of lig_shard_prepare is refused"""
    case, nm, own, every, on0 = slots_lists()
    total = want_slots("slots", "main", every, BIG)[0][0]
    n, nz, _ = want_untouched("slots", "main", False, 0)[0]
    calls = [slots_call("main", every), slots_call("main", every, total - 1), slots_call("main", [nm["over1"]]), slots_call("main", every, tab="T2"),
             slots_call("other", every, list_="main"), untouched_call("main", False, n + 5), untouched_call("main", True, 9), untouched_call("main", False, 0)]
    plan = [dict(case="slots", calls=calls, after_prove=True, synthetic=True)]
    digests = []
    for env in (dict(LIG_DIAG_SLICE=1024), dict(LIG_DIAG_SLICE=1024, LIG_SHARD_FORCE_EXCHANGE=1)):
        outs = run_world(tmp_path, 1, "ipc", plan, **env)
        check_step(outs, 0, plan[0])
        assert outs[0]["shards"][0]["synthetic"] == [E_STATE] * 4
        digests.append([c["digest"] for c in outs[0]["shards"][0]["calls"]])
    assert digests[0] == digests[1]


def test_narrow_rows_derived_values_and_batch_rows(tmp_path):
    """the values no host holds: the product the device formed on rank 1's derived QZ row, the record-carried slots of both ranks' mixed rows;
    then a trace with batch-kind rows in front: a slot of a BIT row of each rank has no term and is never listed as untouched"""
    case = case_of("narrow")
    pin_z, pin_rec, pin_x = case["expect_lin"]
    asked = sorted([17 * L + 17, 17 * L + 18, 12 * L + 100, 1 * L + 5, 3 * L, 12 * L + L - 1, 8 * L + 4, 15 * L + 17, 16 * L + 17, 18 * L - 1])
    n = want_untouched("narrow", "main", False, 0)[0][0]
    batch = case_of("batch")
    bkinds = batch["kinds"]
    bsys = batch["systems"]["main"]
    bit_rows = [r for r, _, _, _ in batch["planted"][:2]]
    used = sorted(set(bsys.slots))
    asked_b = sorted({bit_rows[0] * L + 3, bit_rows[1] * L + L - 1, 0, len(bkinds) * L - 1, hottest(bsys)} | set(used[::97]))
    nb = want_untouched("batch", "main", False, 0)[0][0]
    plan = [dict(case="narrow", calls=[slots_call("main", asked), slots_call("main", asked, 2), untouched_call("main", True, n), untouched_call("main", False, 33)]),
            dict(case="batch", calls=[slots_call("main", asked_b), untouched_call("main", False, nb + 1), untouched_call("main", True, 40)])]
    outs = run_world(tmp_path, 2, "ipc", plan, LIG_DIAG_SLICE=64)
    check_step(outs, 0, plan[0])
    check_step(outs, 1, plan[1])
    _, recs, terms = want_slots("narrow", "main", asked, BIG)
    value = {s: int.from_bytes(v, "little") for s, _, _, _, v in recs}
    rows = case["rows"]
    assert owners(case, 2)[17] == 1 and value[17 * L + 17] == tsd.wit(rows, 15 * L + 17) * tsd.wit(rows, 16 * L + 17) % P, "the value on the derived row is x' * y"
    assert (value[12 * L + 100], value[3 * L], value[12 * L + L - 1]) == ((1 << 70) + 1, 1 << 16, P - 1 - 9), "record-carried slots of both ranks"
    zero = bytes(32)
    res = {c: r for _, c, _, _, _, r in terms}
    assert res[case["spans_ok"]] == zero and all(res[c] != zero for c in (pin_z, pin_rec, pin_x))
    _, brecs, _ = want_slots("batch", "main", asked_b, BIG)
    by = {s: (kd, nt) for s, kd, nt, _, _ in brecs}
    assert by[bit_rows[0] * L + 3] == (tsd.BIT, 0) and by[bit_rows[1] * L + L - 1] == (tsd.BIT, 0)
    listed = {s // L for s, _, _ in want_untouched("batch", "main", False, 1 << 40)[1]}
    assert listed and all(int(bkinds[r]) & 0x7F <= 3 for r in listed)
