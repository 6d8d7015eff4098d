"""GPU: sparse linear constraints on the sharded rows entry (lig_shard_rows_set_linear) -- W ranks as W processes on the one GPU,
collectives over gloo callbacks or comm_ipc (the worker pattern of tests/test_gpu_sharded.py).

Expected values never come from the code under test: root, stage-1 seed and envelope are the oracle's prover over the Python
restatement of matrix and constant (tests/linear_ref.py), computed on rank 0 and compared with every rank's results here, in the
parent.  The per-rank counts are compared with the host-only lig_linear_shard_count, which tests/test_linear_shard_count.py ties to
a count in Python.  As in tests/test_gpu_linear_system.py the oracle cannot prove caller rows of batch kinds: that case is checked
through the flags, the constant, the one-GPU entry with the same system and the uploaded-matrix path.  No test hands a kernel an
invalid index; the misuse cases check return codes of calls that launch nothing."""
import os
import textwrap

import pytest

import multirank as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

WORKER = textwrap.dedent('''
    import hashlib, importlib.util, json, os, sys
    import numpy as np
    root, n_lin, n_quad, n_cons, first_random, when, extra = sys.argv[1], *map(int, sys.argv[2:6]), sys.argv[6], sys.argv[7]
    l, k, n = 320, 512, 2048
    sys.path.insert(0, os.path.join(root, "tests"))
    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, "ligero-prover_amd", rel))
        m = importlib.util.module_from_spec(spec); sys.modules[name] = m; spec.loader.exec_module(m); return m
    pkg = load("ligero_prover_amd", "__init__.py")
    dist = load("lig_dist", "dist.py")
    import linear_ref as lr
    batch, narrow, false = extra == "batch", extra == "narrow", extra == "false"
    prog = None
    if batch:
        import test_batch_rows
        prog = test_batch_rows.demo_program()
    g = dist.Group("gloo")
    ctx = pkg.Context(l, k, n, device=0)
    # every rank runs the same deterministic "guest": all rows, their kinds, the system of the WHOLE trace
    kinds, rows, masks = lr.build_trace(l, k, n, n_lin, n_quad, prog, narrow=narrow)
    system = lr.make_system(kinds, rows, l, n_cons, first_random, seed=11)
    assert lr.holds(system, rows, l)
    rounds, b = pkg.shard_rows_plan(kinds, g.world)
    mine = pkg.local_rows_of(b, g.rank, g.world)
    flipped = None
    if false:                                        # one witness slot on a row owned by rank 1 changes after b_c was fixed
        theirs = set(pkg.local_rows_of(b, 1, g.world))
        flipped = next(s for s in system.slots if s // l in theirs and kinds[s // l] == 0)      # a LINEAR row: the quadratic test stays true
        rows = rows.copy()
        rows[flipped // l, flipped % l, 0] ^= 1
        assert not lr.holds(system, rows, l)
    kk, msgs = kinds.copy(), rows.copy()             # the library draws the pads of every row that draws upstream
    draws = (kinds <= 3) | (kinds == pkg.ROW_KINDS["INIT"])
    msgs[draws, l:] = 0xDEADBEEF
    kk[draws] |= pkg.ROW_DRAW_PAD
    local = msgs[mine] if len(mine) else np.zeros((0, k, 8), dtype=np.uint32)
    widths = None
    if narrow:
        widths = pkg.narrowest_widths(rows, kinds, l)
        assert pkg.ELEM_BIT in set(int(w) for w in widths) and 2 in set(int(w) for w in widths)
        local = np.frombuffer(pkg.pack_rows(local, widths[mine], l), dtype=np.uint8).copy() if len(mine) else np.zeros(0, dtype=np.uint8)
    sysb = system.to_binding(pkg)
    comm = g.make_comm(pkg, ctx)
    sh = ctx.shard_rows_begin(kk, local, g.rank, g.world, comm, generated_at=lr.GEN, elem_bytes=widths)
    if when == "before":
        ctx.shard_rows_set_linear(sh, sysb)
    root_, seed1 = ctx.shard_rows_commit(sh)
    if when == "after":
        ctx.shard_rows_set_linear(sh, sysb)
    stats = ctx.shard_rows_linear_stats(sh)
    proof, info = ctx.shard_rows_prove(sh, None, None)
    # the next trace of the same shape: the structure is resident, no second set_linear
    ctx.shard_rows_restart(sh, local)
    again_commit = ctx.shard_rows_commit(sh) == (root_, seed1)
    proof2, info2 = ctx.shard_rows_prove(sh, None, None)
    ctx.shard_destroy(sh)
    out = {"rank": g.rank, "local_rows": len(mine), "rounds": rounds, "root": root_.hex(), "seed1": seed1.hex(), "const": bytes(info.const_sum).hex(),
           "valid": [info.valid_code, info.valid_linear, info.valid_quad], "again": again_commit and proof2 == proof and bytes(info2.const_sum) == bytes(info.const_sum),
           "stats": list(stats), "count": list(pkg.linear_shard_count(sysb, kinds, l, g.rank, g.world)), "sha": hashlib.sha256(proof).hexdigest(),
           "hot_terms": int(np.count_nonzero(np.array(system.slots) == system.hot_slot))}
    if g.rank == 0:
        # the one-GPU entry with the same system on the same rows
        tr, keep = ctx.rows_begin(kk, msgs, generated_at=lr.GEN)
        ctx.rows_set_linear(tr, sysb)
        ctx.rows_commit(tr)
        ref, rinfo = ctx.rows_prove(tr, None, None)
        ctx.trace_destroy(tr)
        out["ref_sha"] = hashlib.sha256(ref).hexdigest()
        out["ref_valid"] = [rinfo.valid_code, rinfo.valid_linear, rinfo.valid_quad]
        # the yardstick: the oracle's commitment, the Python restatement of matrix and constant, the oracle's envelope
        if batch:
            oroot, oseed = lr.oracle_commitment(l, k, n, n_lin, n_quad, prog)
            rn, cs = lr.expected(system, oseed, len(kinds), l, k)
            tr, keep = ctx.rows_begin(kk, msgs, generated_at=lr.GEN)      # the uploaded-matrix path (pinned to the oracle with batch rows by test_gpu_rows_api.py)
            ctx.rows_commit(tr)
            up, _ = ctx.rows_prove(tr, rn, cs)
            ctx.trace_destroy(tr)
            out.update(oracle_root=oroot.hex(), oracle_seed1=oseed.hex(), expected_const=cs.hex(), uploaded_sha=hashlib.sha256(up).hexdigest())
        else:
            oseed, rn, cs, op = lr.oracle_envelope(l, k, n, kinds, rows, masks, system)
            out.update(oracle_root=op["root"].hex(), oracle_seed1=oseed.hex(), expected_const=cs.hex(), oracle_sha=hashlib.sha256(op["proof"]).hexdigest(),
                       oracle_valid=list(op["valid"]))
            if flipped is not None:
                out["flipped_has_randomness"] = bool(rn[flipped // l, flipped % l].any())
    print(json.dumps(out))
    ctx.close()
    g.close()
''')

# name -> (world, transport, n_linear, n_quad, (n_constraints, first_random), set_linear before / after the commit, extra)
CASES = {
    "gloo_small": (2, None, 3 * 320 + 17, 320 + 9, (30000, 0), "after", "-"),
    "ipc_set_before_commit": (2, "ipc", 3 * 320 + 17, 320 + 9, (30000, 0), "before", "-"),
    "ipc_set_after_commit": (2, "ipc", 3 * 320 + 17, 320 + 9, (30000, 0), "after", "-"),
    "ipc_4_ranks_one_without_rows": (4, "ipc", 700, 0, (30000, 0), "before", "-"),
    "ipc_two_rounds_heavy_slot": (2, "ipc", 320 * 1500 + 7, 330, (70000, 1000), "before", "-"),
    "ipc_8_ranks": (8, "ipc", 320 * 9000 + 11, 330, (30000, 0), "before", "-"),
    "ipc_batch_rows": (2, "ipc", 2 * 320 + 5, 320, (70000, 1000), "after", "batch"),
    "ipc_narrow_rows": (2, "ipc", 4 * 320 + 7, 320 + 3, (30000, 1000), "before", "narrow"),
}
HEAVY_MIN = 2048          # csrc/linear.hip: a slot with more terms is summed by the tree of k_lin_heavy_*


def run_world(tmp_path, name, extra=None, timeout=None):
    world, comm, n_lin, n_quad, (nc, first), when, ex = CASES[name]
    script = tmp_path / "shard_linear_worker.py"
    script.write_text(WORKER)
    if timeout is None:
        timeout = 300 if world < 8 else 600
    outs = mr.run_ranks(mr.python_argv(script, ROOT, n_lin, n_quad, nc, first, when, extra or ex), world, mr.rendezvous_env(world, comm), timeout=timeout)
    return sorted((mr.last_json(o) for o, _ in outs), key=lambda d: d["rank"])


@pytest.mark.parametrize("name", list(CASES))
def test_sharded_rows_with_a_linear_system_equal_rows_prove_and_the_oracle(tmp_path, name):
    outs = run_world(tmp_path, name)
    world, ex = CASES[name][0], CASES[name][6]
    r0 = outs[0]
    assert len(outs) == world
    for o in outs:
        print(name, "rank", o["rank"], "local rows", o["local_rows"], "stats", o["stats"], "count", o["count"])
        assert o["valid"] == [1, 1, 1], o
        assert o["again"], o
        assert o["root"] == r0["oracle_root"] and o["seed1"] == r0["oracle_seed1"], o
        assert o["const"] == r0["expected_const"], o
        assert o["sha"] == r0["ref_sha"], "rank %d: the sharded envelope differs from lig_rows_prove with the same system" % o["rank"]
        assert o["stats"] == o["count"], o
    assert r0["ref_valid"] == [1, 1, 1]
    if ex == "batch":
        assert r0["uploaded_sha"] == r0["ref_sha"]
    else:
        assert r0["oracle_valid"] == [1, 1, 1] and r0["oracle_sha"] == r0["ref_sha"], "the envelope differs from the oracle's"
    assert sum(o["stats"][0] for o in outs) > 0 and r0["hot_terms"] > HEAVY_MIN
    if name == "ipc_4_ranks_one_without_rows":
        assert min(o["local_rows"] for o in outs) == 0 and all(o["stats"][0] == 0 for o in outs if o["local_rows"] == 0)
    if name == "ipc_two_rounds_heavy_slot":
        assert r0["rounds"] == 2
    if name == "ipc_8_ranks":
        assert all(o["local_rows"] > 0 for o in outs)


def test_false_statement_fails_the_linear_check_on_every_rank(tmp_path):
    outs = run_world(tmp_path, "ipc_set_after_commit", extra="false")
    r0 = outs[0]
    assert r0["flipped_has_randomness"] is True
    assert r0["ref_valid"] == [1, 0, 1]
    for o in outs:
        assert o["valid"] == [1, 0, 1], o
        assert o["sha"] == r0["ref_sha"], "rank %d: bytes differ from lig_rows_prove of the same false trace" % o["rank"]
        assert o["const"] == r0["expected_const"] and o["again"]


MISUSE_WORKER = textwrap.dedent('''
    import ctypes as C, importlib.util, json, os, sys
    import numpy as np
    root = sys.argv[1]
    l, k, n = 320, 512, 2048
    sys.path.insert(0, os.path.join(root, "tests"))
    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, "ligero-prover_amd", rel))
        m = importlib.util.module_from_spec(spec); sys.modules[name] = m; spec.loader.exec_module(m); return m
    pkg = load("ligero_prover_amd", "__init__.py")
    dist = load("lig_dist", "dist.py")
    import linear_ref as lr
    import test_batch_rows
    g = dist.Group("gloo")
    ctx = pkg.Context(l, k, n, device=0)
    comm = g.make_comm(pkg, ctx)
    out = {}
    kinds, rows, _ = lr.build_trace(l, k, n, 3 * l + 17, l + 9)
    system = lr.make_equality_system(kinds, l, 0)
    sysb = system.to_binding(pkg)
    # a system on a shard whose job has dense_rands_per_row
    dense = np.where(kinds <= 3, l, 0).astype(np.uint32)
    sh = ctx.shard_rows_begin(kinds, rows, 0, 1, comm, generated_at=lr.GEN, dense_rands_per_row=dense)
    out["dense"] = ctx.L.lig_shard_rows_set_linear(sh, C.byref(sysb))
    ctx.shard_destroy(sh)
    # randomness rows next to a system; stats without / with a system; removing the system brings the old rule back
    sh = ctx.shard_rows_begin(kinds, rows, 0, 1, comm, generated_at=lr.GEN)
    lt, sc = C.c_uint64(), C.c_uint64()
    out["stats_without"] = ctx.L.lig_shard_rows_linear_stats(sh, C.byref(lt), C.byref(sc))
    beyond = system.to_binding(pkg, slots=system.slots[:-1] + [len(kinds) * l])
    out["beyond"] = ctx.L.lig_shard_rows_set_linear(sh, C.byref(beyond))
    ctx.shard_rows_set_linear(sh, sysb)
    ctx.shard_rows_commit(sh)
    proof, ln, info = C.POINTER(C.c_uint8)(), C.c_size_t(), pkg.ProofInfo()
    zeros = np.zeros((len(kinds), k, 8), dtype=np.uint32)
    out["rands_with_system"] = ctx.L.lig_shard_rows_prove(sh, C.c_void_p(zeros.ctypes.data), 0, None, C.byref(proof), C.byref(ln), C.byref(info))
    ctx.shard_rows_set_linear(sh, None)
    out["null_after_removal"] = ctx.L.lig_shard_rows_prove(sh, None, 0, None, C.byref(proof), C.byref(ln), C.byref(info))
    ctx.shard_destroy(sh)
    # a slot on a batch-kind row
    bk, brows, _ = lr.build_trace(l, k, n, 2 * l + 5, l, test_batch_rows.demo_program())
    brow = int(np.flatnonzero(bk > 3)[0])
    onbatch = pkg.LinearSystem.make([0, 1], [brow * l], [pkg.COEF_ONE])
    sh = ctx.shard_rows_begin(bk, brows, 0, 1, comm, generated_at=lr.GEN)
    out["batch_row"] = ctx.L.lig_shard_rows_set_linear(sh, C.byref(onbatch))
    ctx.shard_destroy(sh)
    # a shard from lig_shard_prepare
    sh = ctx.shard_prepare(pkg.Context.make_job(700, 0, generated_at=77), 0, 1, comm)
    out["synthetic_shard"] = ctx.L.lig_shard_rows_set_linear(sh, C.byref(sysb))
    ctx.shard_destroy(sh)
    print(json.dumps(out))
    ctx.close()
    g.close()
''')


def test_misuse_returns_codes(tmp_path):
    script = tmp_path / "shard_linear_misuse.py"
    script.write_text(MISUSE_WORKER)
    outs = mr.run_ranks(mr.python_argv(script, ROOT), 1, mr.rendezvous_env(1), timeout=300)
    out = mr.last_json(outs[0][0])
    E_ARG, E_STATE = -1, -3
    assert out == {"dense": E_ARG, "stats_without": E_STATE, "beyond": E_ARG, "rands_with_system": E_ARG, "null_after_removal": E_ARG,
                   "batch_row": E_ARG, "synthetic_shard": E_STATE}, out
