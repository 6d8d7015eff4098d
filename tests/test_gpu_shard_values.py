"""GPU: lig_shard_rows_set_linear_values -- per-proof values of the coefficient table on the sharded rows entry (csrc/shard.hip,
csrc/linear.hip): W ranks as W processes on the one GPU over comm_ipc (the worker pattern of tests/test_gpu_shard_linear.py).

One structure, two tables: T1 is the table tests/linear_ref.py's make_system computes for the witness (the statement holds), T0 differs
from it in three right-hand-side entries and in one term coefficient (the statement is false for that witness).  What the call has to
reproduce never comes from itself: a FRESH shard given the system with coefs = T1, and the one-GPU entries lig_rows_set_linear_values /
lig_rows_verify_set_linear_values (pinned to the oracle by tests/test_gpu_linear_program.py).  Everything is compared byte for byte, on
every rank, here in the parent.  No test hands a kernel an invalid index: the misuse calls are refused on the host and launch nothing."""
import json
import os
import textwrap

import pytest

import multirank as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

WORKER = textwrap.dedent('''
    import ctypes as C, hashlib, importlib.util, json, os, sys
    import numpy as np
    root, n_lin, n_quad = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    l, k, n = 320, 512, 2048
    sys.path.insert(0, os.path.join(root, "tests"))
    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, "ligero-prover_amd", rel))
        m = importlib.util.module_from_spec(spec); sys.modules[name] = m; spec.loader.exec_module(m); return m
    pkg = load("ligero_prover_amd", "__init__.py")
    dist = load("lig_dist", "dist.py")
    import linear_ref as lr
    import oracle_lib as ol
    g = dist.Group("gloo")
    ctx = pkg.Context(l, k, n, device=0)
    comm = g.make_comm(pkg, ctx)
    # every rank runs the same deterministic "guest": all rows, their kinds, the structure of the WHOLE trace and both tables
    kinds, rows, _ = lr.build_trace(l, k, n, n_lin, n_quad)
    system = lr.make_system(kinds, rows, l, 3000, 0, seed=11, hot_terms=2100)
    assert lr.holds(system, rows, l)
    T1 = list(system.coefs)
    T0 = list(T1)
    term_entry = 20                                  # a full-width table coefficient that terms use, no right-hand side does
    assert term_entry in system.coef_idx and term_entry not in system.rhs_coef
    T0[term_entry] = (T0[term_entry] + 1) % ol.P
    rhs_entries = sorted(set(system.rhs_coef))[::len(set(system.rhs_coef)) // 3][:3]
    for e in rhs_entries:
        assert e not in system.coef_idx
        T0[e] = (T0[e] + 5) % ol.P
    sys0 = lr.System(system.term_begin, system.slots, system.coef_idx, system.rhs_constraint, system.rhs_coef, T0, 0)
    assert not lr.holds(sys0, rows, l)
    b0, b1 = sys0.to_binding(pkg), system.to_binding(pkg)
    rounds, b = pkg.shard_rows_plan(kinds, g.world)
    mine = pkg.local_rows_of(b, g.rank, g.world)
    kk, msgs = kinds.copy(), rows.copy()
    draws = kinds <= 3
    msgs[draws, l:] = 0xDEADBEEF
    kk[draws] |= pkg.ROW_DRAW_PAD
    local = msgs[mine] if len(mine) else np.zeros((0, k, 8), dtype=np.uint32)

    def prove(sh):
        ctx.shard_rows_commit(sh)
        proof, info = ctx.shard_rows_prove(sh, None, None)
        return {"sha": hashlib.sha256(proof).hexdigest(), "const": bytes(info.const_sum).hex(), "valid": [info.valid_code, info.valid_linear, info.valid_quad]}, proof

    out = {"rank": g.rank, "local_rows": len(mine), "hot_terms": int(np.count_nonzero(np.array(system.slots) == system.hot_slot)),
           "n_constraints": system.n_constraints}
    # the shard under test: structure with T0, then the values of T1
    sh = ctx.shard_rows_begin(kk, local, g.rank, g.world, comm, generated_at=lr.GEN)
    tab1 = pkg.coef_table(T1)
    out["no_system"] = ctx.L.lig_shard_rows_set_linear_values(sh, C.c_void_p(tab1.ctypes.data), len(tab1))
    ctx.shard_rows_set_linear(sh, b0)
    ctx.shard_rows_set_linear_values(sh, T1)
    out["values_T1"], proof_T1 = prove(sh)
    ctx.shard_rows_restart(sh, local)                # the values stay in force over the restart
    out["after_restart"], _ = prove(sh)
    ctx.shard_rows_set_linear_values(sh, None)       # back to the system's own table
    ctx.shard_rows_restart(sh, local)
    out["values_none"], _ = prove(sh)
    ctx.shard_rows_set_linear_values(sh, T1)
    short = pkg.coef_table(T1[:-1])
    out["wrong_n_coefs"] = ctx.L.lig_shard_rows_set_linear_values(sh, C.c_void_p(short.ctypes.data), len(short))
    at_p = pkg.coef_table(T1).copy()
    at_p[7] = pkg.coef_table([ol.P - 1])[0]
    at_p[7, 0] += 1                                  # p - 1 is even: no carry, the entry is p itself
    out["entry_is_p"] = ctx.L.lig_shard_rows_set_linear_values(sh, C.c_void_p(at_p.ctypes.data), len(at_p))
    ctx.shard_rows_restart(sh, local)                # the refused calls changed nothing: T1 is still in force
    out["after_misuse"], _ = prove(sh)
    ctx.shard_destroy(sh)
    # fresh shards given the system with coefs = T1 / T0
    for name, bind in (("fresh_T1", b1), ("fresh_T0", b0)):
        sh = ctx.shard_rows_begin(kk, local, g.rank, g.world, comm, generated_at=lr.GEN)
        ctx.shard_rows_set_linear(sh, bind)
        out[name], _ = prove(sh)
        ctx.shard_destroy(sh)
    if g.rank == 0:                                  # the one-GPU entries: prover with values, verifier with values
        tr, keep = ctx.rows_begin(kk, msgs, generated_at=lr.GEN)
        ctx.rows_set_linear(tr, b0)
        ctx.rows_set_linear_values(tr, T1)
        ctx.rows_commit(tr)
        ref, rinfo = ctx.rows_prove(tr, None, None)
        ctx.trace_destroy(tr)
        out["one_gpu"] = {"sha": hashlib.sha256(ref).hexdigest(), "const": bytes(rinfo.const_sum).hex(), "valid": [rinfo.valid_code, rinfo.valid_linear, rinfo.valid_quad]}
        for name, values in (("verify_T1", T1), ("verify_T0", None)):
            vt, _, vi = ctx.rows_verify_begin(kinds, proof_T1)
            ctx.rows_verify_set_linear(vt, b0)
            if values is not None:
                ctx.rows_verify_set_linear_values(vt, values)
            v = ctx.rows_verify_finish(vt, None, None)
            out[name] = [v.valid_linear, v.linear_equal, v.accept]
    print(json.dumps(out))
    ctx.close()
    g.close()
''')

# world -> (linear slots, quadratic slots): the 10-row trace [L L L X Y Z | L X Y Z]; for W = 4 three LINEAR rows, none for the last rank
WORLDS = {1: (3 * 320 + 17, 320 + 9), 2: (3 * 320 + 17, 320 + 9), 4: (700, 0)}
HEAVY_MIN = 2048
E_ARG, E_STATE = -1, -3


@pytest.mark.parametrize("world", list(WORLDS))
def test_values_equal_a_fresh_shard_and_the_one_gpu_entries(tmp_path, world):
    script = tmp_path / "shard_values_worker.py"
    script.write_text(WORKER)
    n_lin, n_quad = WORLDS[world]
    outs = mr.run_ranks(mr.python_argv(script, ROOT, n_lin, n_quad), world, mr.rendezvous_env(world, "ipc"), timeout=300)
    outs = sorted((mr.last_json(o) for o, _ in outs), key=lambda d: d["rank"])
    assert [o["rank"] for o in outs] == list(range(world))
    r0 = outs[0]
    assert r0["hot_terms"] > HEAVY_MIN and r0["n_constraints"] == 3000
    if world == 4:
        assert [o["local_rows"] for o in outs] == [1, 1, 1, 0]
    assert r0["one_gpu"]["valid"] == [1, 1, 1]
    assert r0["verify_T1"] == [1, 1, 1], "the one-GPU verifier with the values of T1 must accept the sharded envelope"
    assert r0["verify_T0"][2] == 0, "the verifier of the T0 statement must not accept the proof of the T1 statement"
    for o in outs:
        print("world", world, "rank", o["rank"], json.dumps({key: o[key] for key in ("values_T1", "values_none")}))
        assert o["values_T1"]["valid"] == [1, 1, 1], o
        assert o["values_T1"] == o["fresh_T1"], "rank %d: values set on a T0 structure differ from a fresh shard with coefs = T1" % o["rank"]
        assert o["values_T1"] == r0["one_gpu"], "rank %d: the sharded envelope differs from lig_rows_set_linear_values on one GPU" % o["rank"]
        assert o["after_restart"] == o["values_T1"], "rank %d: the values did not survive lig_shard_rows_restart" % o["rank"]
        assert o["values_none"]["valid"][1] == 0, "rank %d: with T0 in force the T1 witness must fail the linear check" % o["rank"]
        assert o["values_none"] == o["fresh_T0"], "rank %d: coefs = NULL did not restore the system's own table" % o["rank"]
        assert o["values_none"]["sha"] != o["values_T1"]["sha"] and o["values_none"]["const"] != o["values_T1"]["const"]
        assert (o["no_system"], o["wrong_n_coefs"], o["entry_is_p"]) == (E_STATE, E_ARG, E_ARG), o
        assert o["after_misuse"] == o["values_T1"], "rank %d: the shard must prove the same statement after the refused calls" % o["rank"]
