"""GPU: lig_shard_rows_diagnose -- the violated constraints of a SHARDED rows job (csrc/diagnose.hip, csrc/shard.hip): W ranks as W
processes on the one GPU, collectives over comm_ipc or gloo callbacks (the worker pattern of tests/test_gpu_shard_linear.py).

Expected records never come from the library: tests/diagnose_ref.py restates both residuals in Python integers over the WHOLE row matrix
(derived rows: x * y mod p in Python), here in the parent, and the parent compares them with every rank's output -- constraint numbers,
GLOBAL rows, columns, residual bytes, order, counts, for every pair of caps.  Equality with Context.rows_diagnose of the same rows on
rank 0 is a second check.  Every world makes several diagnose calls, so the file stays at eight world launches.  No test hands a kernel
an invalid index (the misuse calls launch nothing) and none provokes a communicator failure."""
import os
import textwrap

import numpy as np
import pytest

import diagnose_ref as dr
import linear_ref as lr
import multirank as mr
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

P = ol.P
L, K, N = 320, 512, 2048
ONE, NEG_ONE = lr.ONE, lr.NEG_ONE
LINEAR, QX, QY, QZ, BIT, EQY, BQZ = 0, 1, 2, 3, 5, 7, 10
BIG = 1 << 40                      # caps nothing reaches
SLICE = 512                        # LIG_DIAG_SLICE of the multi-slice worlds: 3000 constraints = 6 slices of 2 sub-blocks of 256


def wit(rows, s):
    return ol.from_limbs(rows[s // L, s % L])[0]


def set_wit(rows, s, v):
    rows[s // L, s % L] = ol.to_limbs([v % P])[0]


class Builder:
    """a linear_ref.System constraint by constraint; b_c is computed from `rows` (the witness BEFORE any corruption) unless given"""

    def __init__(self, rows):
        self.rows = rows
        self.term_begin, self.slots, self.cidx, self.rhs_c, self.rhs_b, self.coefs = [0], [], [], [], [], []

    def coef(self, v):
        if v not in self.coefs:
            self.coefs.append(v)
        return self.coefs.index(v)

    def value(self, ci):
        return 1 if ci == ONE else P - 1 if ci == NEG_ONE else self.coefs[ci]

    def add(self, terms):
        for s, ci in terms:
            self.slots.append(s)
            self.cidx.append(ci)
        self.term_begin.append(len(self.slots))
        b = sum(self.value(ci) * wit(self.rows, s) for s, ci in terms) % P
        c = len(self.term_begin) - 2
        if b:
            self.rhs_c.append(c)
            self.rhs_b.append(self.coef(b))
        return c

    def system(self):
        return lr.System(self.term_begin, self.slots, self.cidx, self.rhs_c, self.rhs_b, self.coefs, 0)


def deal(kinds, world):
    """-> the global rows of every rank (lig_shard_rows_plan restated: one round at these sizes, chunks never split a triple or a pair)"""
    R = len(kinds)
    assert R <= 512 * world
    target = max(1, -(-R // world))
    b = [0]
    for g in range(1, world):
        e = min(R, b[-1] + target)
        while e < R and int(kinds[e]) & 0x7F in (2, 3, 7, 9, 10):
            e += 1
        b.append(e)
    b.append(R)
    return [list(range(b[g], b[g + 1])) for g in range(world)]


_cache = {}


def std_trace():
    """10 rows [L L L X Y Z | L X Y Z]: rank 0 of two holds rows 0-5, rank 1 rows 6-9; a seeded system of 3000 constraints that holds"""
    if "std" not in _cache:
        kinds, rows, _ = lr.build_trace(L, K, N, 3 * L + 17, L + 9)
        assert [int(v) for v in kinds] == [0, 0, 0, 1, 2, 3, 0, 1, 2, 3] and deal(kinds, 2) == [[0, 1, 2, 3, 4, 5], [6, 7, 8, 9]]
        system = lr.make_system(kinds, rows, L, 3000, 0, seed=11, hot_terms=60)
        _cache["std"] = (kinds, rows, system)
    return _cache["std"]


def case_satisfied():
    kinds, rows, system = std_trace()
    return dict(kinds=kinds, rows=rows, systems={"main": system}, prove="main")


def victims_of(system, rows_of_rank, kinds, count, seed):
    """`count` slots on LINEAR rows of one rank that the system uses (not the hot slot)"""
    rng = np.random.default_rng(seed)
    mine = sorted(set(s for s in system.slots if s // L in rows_of_rank and kinds[s // L] == LINEAR and s != system.hot_slot))
    return [int(s) for s in rng.choice(mine, size=count, replace=False)]


def case_corrupted():
    """the satisfied trace, then: witness slots on LINEAR rows of rank 0 and of rank 1 change, a z slot of a triple changes (a quadratic
    violation), one right-hand side changes; a second system holds two constraints of 2100 terms over rows of both ranks, one of them
    through a changed slot"""
    if "corrupted" in _cache:
        return _cache["corrupted"]
    kinds, truth, good = std_trace()
    ranks = deal(kinds, 2)
    rows = truth.copy()
    victims = victims_of(good, ranks[0], kinds, 5, 2) + victims_of(good, ranks[1], kinds, 4, 3)
    for s in victims:
        set_wit(rows, s, wit(rows, s) + 1 + s)
    rows[5, 11, 0] ^= 1                                              # z of the first triple, column 11
    system = lr.System(good.term_begin, good.slots, good.coef_idx, good.rhs_constraint, good.rhs_coef, good.coefs, 0)
    i = len(system.rhs_constraint) // 2                              # one right-hand side: another table entry
    system.rhs_coef[i] = 3 if system.rhs_coef[i] != 3 else 4
    rhs_changed = system.rhs_constraint[i]
    # heavy constraints: more than 2048 terms each (one workgroup per constraint), slots on LINEAR rows of both ranks
    rng = np.random.default_rng(4)
    clean = np.array(sorted(set(r * L + c for r in (0, 1, 2, 6) for c in range(L)) - set(victims)))
    b = Builder(truth)
    b.coefs = [3, P - 4, (1 << 200) + 9]
    expect_heavy = []
    for violated in (False, True):
        terms = [(int(s), [ONE, NEG_ONE, 0, 1, 2][int(ci)]) for s, ci in zip(rng.choice(clean, 2100), rng.integers(0, 5, 2100))]
        if violated:
            terms[1000] = (victims[0], ONE)                          # a changed slot of rank 0 ...
            terms[2000] = (victims[-1], ONE)                         # ... and one of rank 1
        cn = b.add(terms)
        assert {s // L for s, _ in terms} >= {0, 6}
        if violated:
            expect_heavy.append(cn)
        b.add([(int(rng.choice(clean)), ONE)])                       # a small constraint in between
    heavy = b.system()
    assert [heavy.term_begin[c + 1] - heavy.term_begin[c] for c in (0, 2)] == [2100, 2100]
    _cache["corrupted"] = dict(kinds=kinds, rows=rows, systems={"main": system, "heavy": heavy}, prove="main", victims=victims,
                               rhs_changed=rhs_changed, expect_heavy=expect_heavy)
    return _cache["corrupted"]


def case_gloo():
    """the smallest system: the 40 equalities of make_equality_system, one of them broken"""
    kinds, truth, _ = std_trace()
    eq = lr.make_equality_system(kinds, L, 0)
    rows = truth.copy()
    set_wit(rows, eq.slots[6], wit(rows, eq.slots[6]) + 5)
    rows[9, 3, 0] ^= 2                                               # z of the second triple (rank 1), column 3
    return dict(kinds=kinds, rows=rows, systems={"main": eq}, prove="main")


def case_w4():
    """the shape of ipc_4_ranks_one_without_rows: three LINEAR rows, one each for ranks 0-2, none for rank 3; violations on rows 0 and 2"""
    kinds, truth, _ = lr.build_trace(L, K, N, 700, 0)
    assert deal(kinds, 4) == [[0], [1], [2], []]
    system = lr.make_system(kinds, truth, L, 1500, 0, seed=5, hot_terms=60)
    rows = truth.copy()
    for r, seed in ((0, 6), (2, 7)):
        for s in victims_of(system, [r], kinds, 3, seed):
            set_wit(rows, s, wit(rows, s) + 7)
    return dict(kinds=kinds, rows=rows, systems={"main": system}, prove="main")


def case_batch():
    """rows of a batch program in front (test_batch_rows.demo_program): a BIT row of each rank holding a 2, an EQX / EQY pair differing in
    one column, a batch product with a wrong z, a changed LINEAR slot behind them"""
    import test_batch_rows
    kinds, truth, _ = lr.build_trace(L, K, N, 2 * L + 5, L, test_batch_rows.demo_program())
    ranks = deal(kinds, 2)
    system = lr.make_system(kinds, truth, L, 800, 0, seed=13, hot_terms=60)
    rows = truth.copy()
    bits = [int(r) for r in np.flatnonzero(kinds == BIT)]
    bit0, bit1 = next(r for r in bits if r in ranks[0]), next(r for r in reversed(bits) if r in ranks[1])
    eqy, bqz = int(np.flatnonzero(kinds == EQY)[0]), int(np.flatnonzero(kinds == BQZ)[0])
    rows[bit0, 3, 0] = 2
    rows[bit1, L - 1, 0] = 2
    rows[eqy, 300, 0] ^= 1
    rows[bqz, 1, 2] ^= 4
    s = victims_of(system, ranks[1], kinds, 1, 8)[0]
    set_wit(rows, s, wit(rows, s) + 9)
    return dict(kinds=kinds, rows=rows, systems={"main": system}, prove="main",
                planted=[(bit0, bit0, bit0, 3), (bit1, bit1, bit1, L - 1), (eqy - 1, dr.NO_ROW, eqy, 300), (bqz - 2, bqz - 1, bqz, 1)])


def case_narrow():
    """18 rows made here, 9 per rank: a full-width row, a 16-bit row, a bit row, a MIXED row (16-bit with three record-carried slots), two
    8-byte rows and a triple whose QZ row is DERIVED (LIG_ELEM_PRODUCT), twice.  An operand of the second triple is wrong: the derived
    z is x' * y, the quadratic test holds, and the constraint that pins z to the honest product is violated; a record-carried slot of
    rank 1's mixed row is wrong as well."""
    kinds = np.array(([LINEAR] * 6 + [QX, QY, QZ]) * 2, dtype=np.uint8)
    assert deal(kinds, 2) == [list(range(9)), list(range(9, 18))]
    rng = np.random.default_rng(71)
    truth = np.zeros((18, K, 8), dtype=np.uint32)
    widths = np.zeros(18, dtype=np.uint8)
    wide = np.zeros(18, dtype=np.uint32)
    ELEM_BIT, ELEM_PRODUCT = 0x81, 0x82
    for base in (0, 9):
        truth[base, :L] = ol.rand_field(rng, L)
        truth[base + 1, :L, 0] = rng.integers(0, 1 << 16, L)
        truth[base + 2, :L, 0] = rng.integers(0, 2, L)
        truth[base + 3, :L, 0] = rng.integers(0, 1 << 16, L)
        for col, v in zip((0, 100, L - 1), (1 << 16, (1 << 64) + base, P - 1 - base)):
            set_wit(truth, (base + 3) * L + col, v)
        for r in (base + 4, base + 5):
            v = rng.integers(0, 1 << 63, L, dtype=np.uint64)
            truth[r, :L, 0], truth[r, :L, 1] = (v & 0xFFFFFFFF).astype(np.uint32), (v >> 32).astype(np.uint32)
        truth[base + 6, :L], truth[base + 7, :L] = ol.rand_field(rng, L), ol.rand_field(rng, L)
        widths[base:base + 9] = [32, 2, ELEM_BIT, 2, 8, 8, 32, 32, ELEM_PRODUCT]
        wide[base + 3] = 3

    def derive(rows):
        for z in (8, 17):
            xs, ys = ol.from_limbs(rows[z - 2, :L]), ol.from_limbs(rows[z - 1, :L])
            rows[z, :L] = ol.to_limbs([x * y % P for x, y in zip(xs, ys)])

    derive(truth)
    b = Builder(truth)
    b.coefs = [5, P - 2, (1 << 253) + 3]
    pin_z = b.add([(17 * L + 17, ONE)])                              # z[17] of the second triple = the honest product
    b.add([(17 * L + 18, ONE)])                                      # the next column: holds
    pin_rec = b.add([(12 * L + 100, ONE), (1 * L + 5, 0)])           # the record-carried slot of rank 1's mixed row, with a 16-bit slot of rank 0
    spans_ok = b.add([(3 * L, ONE), (12 * L + L - 1, NEG_ONE), (8 * L + 4, 2)])      # records of both ranks and a derived slot of rank 0: holds
    pin_x = b.add([(15 * L + 17, 1)])                                # the wrong operand itself
    pool = [r * L + c for r in (0, 1, 2, 4, 9, 10, 11, 13) for c in range(L)]
    for _ in range(300):
        b.add([(int(s), [ONE, NEG_ONE, 0, 1, 2][int(ci)]) for s, ci in zip(rng.choice(pool, 3), rng.integers(0, 5, 3))])
    rows = truth.copy()
    set_wit(rows, 15 * L + 17, wit(truth, 15 * L + 17) + 1)
    set_wit(rows, 12 * L + 100, (1 << 70) + 1)
    derive(rows)
    return dict(kinds=kinds, rows=rows, systems={"main": b.system()}, prove="main", widths=widths, wide=wide,
                expect_lin=[pin_z, pin_rec, pin_x], spans_ok=spans_ok)


CASES = {"satisfied": case_satisfied, "corrupted": case_corrupted, "gloo": case_gloo, "w4": case_w4, "batch": case_batch, "narrow": case_narrow}


def expected(case, sysname, lin_cap, quad_cap):
    """what every rank must return: {counts, lin, quad}, from the Python restatement over the whole matrix (computed once per system)"""
    memo = case.setdefault("_want", {})
    if "q" not in memo:
        memo["q"] = dr.quad_violations(case["kinds"], case["rows"], L)
    if sysname is not None and sysname not in memo:
        memo[sysname] = dr.linear_violations(case["systems"][sysname], case["rows"], L)
    wl, wq = (memo[sysname] if sysname is not None else []), memo["q"]
    return {"counts": [len(wl), min(len(wl), lin_cap), len(wq), min(len(wq), quad_cap)],
            "lin": [[c, dr.residual_bytes(r).hex()] for c, r in wl[:lin_cap]],
            "quad": [[x, y, z, i, dr.residual_bytes(r).hex()] for x, y, z, i, r in wq[:quad_cap]]}


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
    import linear_ref as lr
    import test_gpu_shard_diagnose as tsd
    g = dist.Group("gloo")
    ctx = pkg.Context(l, k, n, device=0)
    comm = g.make_comm(pkg, ctx)
    out = {"rank": g.rank, "shards": []}

    def ship(case):
        """-> (kinds | DRAW_PAD, all rows as shipped, this rank's rows as shipped, keyword arguments of both begin calls)"""
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

    def record(info, lin, quad):
        return {"counts": [int(info.n_linear_bad), int(info.n_linear_reported), int(info.n_quad_bad), int(info.n_quad_reported)],
                "lin": [[int(r["constraint"]), bytes(r["residual"]).hex()] for r in lin],
                "quad": [[int(r["row_x"]), int(r["row_y"]), int(r["row_z"]), int(r["column"]), bytes(r["residual"]).hex()] for r in quad]}

    def info_():
        i = pkg.DiagInfo(); i.struct_bytes = C.sizeof(pkg.DiagInfo); return i

    for step in plan:            # one shard per step: {"case", "calls": [[system name or null, lin_cap, quad_cap]], "diagnose", "misuse", "after_prove"}
        case = tsd.CASES[step["case"]]()
        binds = {nm: s.to_binding(pkg) for nm, s in case["systems"].items()}
        kk, msgs, local, kw, mine = ship(case)
        sh = ctx.shard_rows_begin(kk, local, g.rank, g.world, comm, generated_at=lr.GEN, **kw)
        res = {"case": step["case"], "local_rows": len(mine), "calls": []}
        main = binds[case["prove"]]
        if step.get("misuse"):
            system = case["systems"][case["prove"]]
            res["before_commit"] = ctx.L.lig_shard_rows_diagnose(sh, C.byref(main), None, 0, None, 0, C.byref(info_()))
        ctx.shard_rows_set_linear(sh, main)
        commit = ctx.shard_rows_commit(sh)
        if step.get("misuse"):       # refused on the host before any collective: the calls below would hang or fail otherwise
            beyond = system.to_binding(pkg, slots=system.slots[:-1] + [len(case["kinds"]) * l])
            res["slot_out_of_range"] = ctx.L.lig_shard_rows_diagnose(sh, C.byref(beyond), None, 0, None, 0, C.byref(info_()))
            res["null_lin"] = ctx.L.lig_shard_rows_diagnose(sh, C.byref(main), None, 5, None, 0, C.byref(info_()))
            res["null_quad"] = ctx.L.lig_shard_rows_diagnose(sh, C.byref(main), None, 0, None, 5, C.byref(info_()))
            short = info_(); short.struct_bytes -= 8
            res["short_info"] = ctx.L.lig_shard_rows_diagnose(sh, C.byref(main), None, 0, None, 0, C.byref(short))
        def run_calls():
            got = []
            for nm, lc, qc in step["calls"]:
                info, lin, quad = ctx.shard_rows_diagnose(sh, binds[nm] if nm is not None else None, lin_cap=min(lc, 1 << 16), quad_cap=min(qc, 1 << 16))
                got.append(record(info, lin, quad))
            return got
        if step.get("diagnose", True):
            res["calls"] = run_calls()
        proof, pinfo = ctx.shard_rows_prove(sh, None, None)
        res["proof"] = hashlib.sha256(proof).hexdigest()
        res["valid"] = [pinfo.valid_code, pinfo.valid_linear, pinfo.valid_quad]
        if step.get("after_prove"):
            res["calls_after_prove"] = run_calls()
        ctx.shard_destroy(sh)
        if step.get("deal_facts"):   # from the deal and the Python restatement: which violated / satisfied constraints span ranks, where they fall
            import diagnose_ref as dr
            system = case["systems"]["main"]
            owner_of_row = {}
            for rk, rws in enumerate(tsd.deal(case["kinds"], g.world)):
                owner_of_row.update({r: rk for r in rws})
            bad = [c for c, _ in dr.linear_violations(system, case["rows"], l)]
            spans = lambda c: len({owner_of_row[system.slots[t] // l] for t in range(system.term_begin[c], system.term_begin[c + 1])}) > 1
            B = tsd.SLICE // g.world
            res["deal_facts"] = {"violated_spanning": sum(1 for c in bad if spans(c)),
                                 "satisfied_spanning": sum(1 for c in range(system.n_constraints) if c not in set(bad) and spans(c)),
                                 "slices": sorted({c // (B * g.world) for c in bad}), "owners": sorted({c % (B * g.world) // B for c in bad}),
                                 "n_slices": -(-system.n_constraints // (B * g.world))}
        if g.rank == 0 and step.get("diagnose", True):      # the second check: the one-GPU entry on the same rows
            tr, keep = ctx.rows_begin(kk, msgs, generated_at=lr.GEN, **kw)
            ctx.rows_commit(tr)
            res["one_gpu"] = []
            for nm, lc, qc in step["calls"]:
                info, lin, quad = ctx.rows_diagnose(tr, binds[nm] if nm is not None else None, lin_cap=min(lc, 1 << 16), quad_cap=min(qc, 1 << 16))
                res["one_gpu"].append(record(info, lin, quad))
            ctx.trace_destroy(tr)
        out["shards"].append(res)
    print(json.dumps(out))
    ctx.close()
    g.close()
''')


def run_world(tmp_path, world, comm, plan, **env):
    import json
    script = tmp_path / "shard_diagnose_worker.py"
    script.write_text(WORKER)
    outs = mr.run_ranks(mr.python_argv(script, ROOT, "w", json.dumps(plan)), world, mr.rendezvous_env(world, comm, **env), timeout=300)
    outs = sorted((mr.last_json(o) for o, _ in outs), key=lambda d: d["rank"])
    assert [o["rank"] for o in outs] == list(range(world))
    return outs


def check_calls(outs, plan):
    """every rank's output of every call == the Python restatement; rank 0's one-GPU output == the same"""
    for si, step in enumerate(plan):
        if not step.get("diagnose", True):
            continue
        case = CASES[step["case"]]()
        for ci, (nm, lc, qc) in enumerate(step["calls"]):
            want = expected(case, nm, lc, qc)
            print(step["case"], nm, (lc, qc), "counts", want["counts"])
            for o in outs:
                got = o["shards"][si]["calls"][ci]
                assert got["counts"] == want["counts"], (o["rank"], nm, lc, qc, got["counts"], want["counts"])
                assert got == want, "rank %d, call %d (%s, caps %d / %d): records differ from the reference" % (o["rank"], ci, nm, lc, qc)
                if step.get("after_prove"):
                    assert o["shards"][si]["calls_after_prove"][ci] == want, "rank %d: diagnose after the proof differs" % o["rank"]
            assert outs[0]["shards"][si]["one_gpu"][ci] == want, "lig_rows_diagnose on the same rows differs from the reference"


CORRUPTED_CALLS = [["main", BIG, BIG], ["main", 0, 0], ["main", 7, 1], ["main", 1, 0], [None, BIG, BIG], ["heavy", BIG, BIG]]


def test_two_ranks_many_slices_caps_heavy_constraints_and_misuse(tmp_path):
    """ipc, W = 2, six slices: violations on rows of both ranks, in several slices and in sub-blocks of both owners, constraints that span
    ranks violated and satisfied; all records, counts only, caps that cut inside a slice, sys = None, constraints of 2100 terms over
    both ranks; and the misuse calls, which launch nothing and leave no collective half-issued (the shard diagnoses and proves after)"""
    plan = [dict(case="corrupted", calls=CORRUPTED_CALLS, misuse=True, deal_facts=True, after_prove=True)]
    outs = run_world(tmp_path, 2, "ipc", plan, LIG_DIAG_SLICE=SLICE)
    case = case_corrupted()
    want = expected(case, "main", BIG, BIG)
    assert want["counts"][0] >= 12 and want["counts"][2] == 1 and want["quad"][0][:4] == [3, 4, 5, 11]
    assert case["rhs_changed"] in [c for c, _ in want["lin"]]
    assert [c for c, _ in expected(case, "heavy", BIG, BIG)["lin"]] == case["expect_heavy"] == [2]
    # the caps of the third call cut inside a slice: constraint 7 of the violated ones lies beyond the first sub-block boundary or slice
    for o in outs:
        s = o["shards"][0]
        assert (s["before_commit"], s["slot_out_of_range"], s["null_lin"], s["null_quad"], s["short_info"]) == (-3, -1, -1, -1, -1), s
        assert s["valid"] == [1, 0, 0], s
        f = s["deal_facts"]
        assert f["violated_spanning"] >= 1 and f["satisfied_spanning"] >= 1, f
        assert f["n_slices"] >= 4 and len(f["slices"]) >= 2 and f["owners"] == [0, 1], f
    B = SLICE // 2
    first7 = [c for c, _ in want["lin"][:7]]
    assert len({c // B for c in first7}) >= 2, "the seven reported records must come from more than one owner's sub-block"
    check_calls(outs, plan)
    assert len({o["shards"][0]["proof"] for o in outs}) == 1


def test_single_slice_and_a_satisfied_trace_whose_envelope_is_unchanged(tmp_path):
    """the same world with the slice knob at its default (one slice); then a satisfied trace: zero counts before and after the proof, and
    the envelope of the diagnosed shard is byte-identical to that of a shard that was never diagnosed"""
    plan = [dict(case="corrupted", calls=CORRUPTED_CALLS[:4]),
            dict(case="satisfied", calls=[["main", BIG, BIG], ["main", 0, 0]], after_prove=True),
            dict(case="satisfied", calls=[], diagnose=False)]
    outs = run_world(tmp_path, 2, "ipc", plan)
    check_calls(outs, plan)
    assert expected(case_satisfied(), "main", BIG, BIG)["counts"] == [0, 0, 0, 0]
    for o in outs:
        assert o["shards"][1]["valid"] == [1, 1, 1] and o["shards"][1]["proof"] == o["shards"][2]["proof"] == outs[0]["shards"][1]["proof"], o["rank"]


def test_four_ranks_one_without_rows(tmp_path):
    plan = [dict(case="w4", calls=[["main", BIG, BIG], ["main", 2, 0], [None, 5, 5]])]
    outs = run_world(tmp_path, 4, "ipc", plan, LIG_DIAG_SLICE=256)
    assert [o["shards"][0]["local_rows"] for o in outs] == [1, 1, 1, 0]
    assert expected(case_w4(), "main", BIG, BIG)["counts"][0] >= 6
    check_calls(outs, plan)


def test_host_synchronous_collectives_over_gloo(tmp_path):
    plan = [dict(case="gloo", calls=[["main", BIG, BIG], ["main", 0, 0], [None, BIG, BIG]])]
    outs = run_world(tmp_path, 2, None, plan, LIG_DIAG_SLICE=16)
    want = expected(case_gloo(), "main", BIG, BIG)
    assert want["counts"] == [1, 1, 1, 1] and want["quad"][0][:4] == [7, 8, 9, 3]
    check_calls(outs, plan)


def test_narrow_rows_with_a_derived_triple_and_a_mixed_row(tmp_path):
    plan = [dict(case="narrow", calls=[["main", BIG, BIG], ["main", 2, 2]])]
    outs = run_world(tmp_path, 2, "ipc", plan, LIG_DIAG_SLICE=64)
    case = case_narrow()
    want = expected(case, "main", BIG, BIG)
    got = [c for c, _ in want["lin"]]
    assert set(case["expect_lin"]) <= set(got) and case["spans_ok"] not in got
    assert want["quad"] == [], "a wrong operand of a derived triple is no quadratic violation"
    check_calls(outs, plan)


def test_batch_rows_in_front(tmp_path):
    plan = [dict(case="batch", calls=[["main", BIG, BIG], [None, 3, 3], ["main", 0, 0]])]
    outs = run_world(tmp_path, 2, "ipc", plan, LIG_DIAG_SLICE=128)
    case = case_batch()
    want = expected(case, "main", BIG, BIG)
    assert sorted(tuple(q[:4]) for q in want["quad"]) == sorted(case["planted"]) and want["counts"][0] >= 1
    assert any(q[1] == 0xFFFFFFFF for q in want["quad"])
    assert min(o["shards"][0]["local_rows"] for o in outs) > 100
    check_calls(outs, plan)


@pytest.mark.parametrize("force", [False, True])
def test_one_rank(tmp_path, force):
    """W = 1: lig_rows_diagnose's output (no collective); once more with LIG_SHARD_FORCE_EXCHANGE, through the exchange path"""
    plan = [dict(case="corrupted", calls=CORRUPTED_CALLS, after_prove=True)]
    env = dict(LIG_DIAG_SLICE=SLICE)
    if force:
        env["LIG_SHARD_FORCE_EXCHANGE"] = 1
    outs = run_world(tmp_path, 1, "ipc", plan, **env)
    check_calls(outs, plan)
