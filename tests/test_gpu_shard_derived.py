"""GPU: derived slots on the sharded rows entry (lig_shard_rows_set_derived) -- W ranks as W processes on the one GPU, collectives over
gloo callbacks or comm_ipc (the worker pattern of tests/test_gpu_shard_linear.py).

Expected bytes never come from the sharded derived path: the values of the targets are the Python integers of tests/shard_derived_ref.py,
root, stage-1 seed and envelope are the oracle's prover over the rows that carry those integers (computed on rank 0, compared with every
rank's results here, in the parent) and the one-GPU lig_rows_set_derived envelope; the per-rank counts are the Python restatement
(shard_derived_ref.shard_info) and the host-only lig_derived_shard_count.  What the list exercises -- which operand crosses which ranks in
which wave -- holds by construction against the deal and is asserted on the host, in the parent, before any rank starts.  No test hands a
kernel an invalid index; the refusals check return codes of calls that launch nothing."""
import json
import os
import textwrap

import numpy as np
import pytest

import derived_ref as dr
import hip_lib
import multirank as mr
import shard_derived_ref as sdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

PRELUDE = textwrap.dedent('''
    import ctypes as C, hashlib, importlib.util, json, os, sys
    import numpy as np
    root, mode = sys.argv[1], sys.argv[2]
    l, k, n = 320, 512, 2048
    sys.path.insert(0, os.path.join(root, "tests"))
    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, "ligero-prover_amd", rel))
        m = importlib.util.module_from_spec(spec); sys.modules[name] = m; spec.loader.exec_module(m); return m
    pkg = load("ligero_prover_amd", "__init__.py")
    dist = load("lig_dist", "dist.py")
    import derived_ref as dr, linear_ref as lr, oracle_lib as ol, shard_derived_ref as sdr
    sha = lambda b: hashlib.sha256(bytes(b)).hexdigest()
    g = dist.Group("gloo")
    ctx = pkg.Context(l, k, n, device=0)
    comm = g.make_comm(pkg, ctx)
    out = {"rank": g.rank}
''')

WORKER = PRELUDE + textwrap.dedent('''
    if mode in ("world", "diagnose"):
        n_lin, n_tri, idle, where = int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6]
        Wd = sdr.world(pkg, g.world, n_lin, n_tri, idle=None if idle < 0 else idle)
        sysb = Wd.system.to_binding(pkg)
        mine = pkg.local_rows_of(Wd.boundaries, g.rank, g.world)
        rows = Wd.shipped_rows
        if mode == "diagnose":                       # every input as the statement has it (what travels at a target is ignored), then one input of t_in -- on another rank than t_in -- changes
            rows = Wd.shipped_rows.copy()
            s = Wd.input_of_in
            rows[s // l, s % l, 0] ^= 1
            moved = (dr.P - int(rows[s // l, s % l, 0])) % dr.P
            assert moved != Wd.w[Wd.t_in]
        kk, _ = Wd.ship(pkg)
        local = Wd.pack_local(pkg, rows, mine)
        device = where == "device"
        msgs = (ctx.upload(local) if len(local) else ctx.malloc(32)) if device else local
        sh = ctx.shard_rows_begin(kk, msgs, g.rank, g.world, comm, on_device=device, generated_at=lr.GEN, elem_bytes=Wd.widths)
        ctx.shard_rows_set_linear(sh, sysb)
        info = ctx.shard_rows_set_derived(sh, sysb, Wd.pairs)
        root_, seed1 = ctx.shard_rows_commit(sh)
        got = ol.from_limbs(ctx.shard_rows_read_slots(sh, Wd.targets))
        out.update(local_rows=len(mine), rounds=int(Wd.rounds), info=info.as_dict(),
                   count=pkg.derived_shard_count(sysb, Wd.kinds, l, Wd.pairs, Wd.widths, g.rank, g.world).as_dict())
        if mode == "diagnose":
            di, lin, quad = ctx.shard_rows_diagnose(sh, sysb)
            out.update(violated=[int(c) for c in lin["constraint"]], n_linear=int(di.n_linear_bad), t_in_value=hex(got[Wd.targets.index(Wd.t_in)]), moved=hex(moved),
                       others_wrong=[t for t, v in zip(Wd.targets, got) if v != Wd.w[t] and t != Wd.t_in])
            ctx.shard_rows_prove(sh, None, None)
        else:
            proof, pi = ctx.shard_rows_prove(sh, None, None)
            ctx.shard_rows_restart(sh, msgs, on_device=device)
            again = ctx.shard_rows_commit(sh) == (root_, seed1)
            proof2, pi2 = ctx.shard_rows_prove(sh, None, None)
            out.update(root=root_.hex(), seed1=seed1.hex(), sha=sha(proof), valid=[pi.valid_code, pi.valid_linear, pi.valid_quad],
                       again=bool(again and proof2 == proof), wrong=[t for t, v in zip(Wd.targets, got) if v != Wd.w[t]])
        ctx.shard_destroy(sh)
        if g.rank == 0 and mode == "world":
            want = Wd.oracle(Wd.expected_rows)
            out.update(oracle_root=want["root"].hex(), oracle_seed1=want["stage1_seed"].hex(), oracle_sha=sha(want["proof"]), oracle_valid=list(want["valid"]))
            tr, keep = ctx.rows_begin(kk, pkg.pack_rows(rows, Wd.widths, l), generated_at=lr.GEN, elem_bytes=Wd.widths)
            ctx.rows_set_linear(tr, sysb)
            ctx.rows_set_derived(tr, sysb, Wd.pairs)
            r1, s1 = ctx.rows_commit(tr)
            ref, rinfo = ctx.rows_prove(tr, None, None)
            ctx.trace_destroy(tr)
            out.update(ref_root=r1.hex(), ref_seed1=s1.hex(), ref_sha=sha(ref))
    elif mode == "guest":
        from test_linear_system import mul_add_terms
        d = np.load(os.path.join(root, "tests", "golden", "ref_rows_mul_add_320.npz"))
        meta = json.loads(str(d["meta"]))
        assert (meta["l"], meta["k"], meta["n"]) == (l, k, n)
        reps, kinds, vals, key = meta["reps"], d["kinds"], d["vals"], bytes.fromhex(meta["encoding_seed"])
        s = mul_add_terms(reps, l, lr.witness(vals, l))
        pairs = [(4 * (i // l) * l + i % l, 2 * i) for i in range(reps)]
        widths = pkg.narrowest_widths(vals, kinds, l, derive_products=True)
        blind = vals.copy()
        blind[kinds == 0] = 0                        # nothing of w reaches the library: LINEAR rows travel as all-zero bit rows
        widths[kinds == 0] = pkg.ELEM_BIT
        blind[kinds == 3] = 0xDEADBEEF               # LIG_ELEM_PRODUCT rows are not shipped at all
        rounds, b = pkg.shard_rows_plan(kinds, g.world)
        mine = pkg.local_rows_of(b, g.rank, g.world)
        local = np.frombuffer(pkg.pack_rows(blind[mine], widths[mine], l), dtype=np.uint8).copy()
        sysb = s.to_binding(pkg)
        sh = ctx.shard_rows_begin(kinds | pkg.ROW_DRAW_PAD, local, g.rank, g.world, comm, encoding_seed=key, generated_at=lr.GEN, elem_bytes=widths)
        ctx.shard_rows_set_linear(sh, sysb)
        info = ctx.shard_rows_set_derived(sh, sysb, pairs)
        root_, seed1 = ctx.shard_rows_commit(sh)
        proof, pi = ctx.shard_rows_prove(sh, None, None)
        ctx.shard_destroy(sh)
        out.update(info=info.as_dict(), reps=reps, root=root_.hex(), seed1=seed1.hex(), sha=sha(proof), valid=[pi.valid_code, pi.valid_linear, pi.valid_quad],
                   local_rows=len(mine))
        if g.rank == 0:
            masks = ol.form_masks(key, len(kinds) * (k - l), l, k)
            want = lr.oracle_envelope(l, k, n, kinds, vals, masks, s)[3]
            out.update(oracle_root=want["root"].hex(), oracle_seed1=want["stage1_seed"].hex(), oracle_sha=sha(want["proof"]), oracle_valid=list(want["valid"]))
    elif mode == "state":
        # one rank; return codes only for everything that is refused
        Wd = dr.world(pkg)
        sysb = Wd.system.to_binding(pkg)
        kk, packed = Wd.ship(pkg)
        packed = np.frombuffer(bytes(packed), dtype=np.uint8).copy()
        set_ = ctx.L.lig_shard_rows_set_derived
        def call(sh, pairs, system=sysb, info=None):
            d = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
            return set_(sh, C.byref(system), d.ctypes.data if len(d) else None, len(d), info)
        sh = ctx.shard_rows_begin(kk, packed, 0, 1, comm, generated_at=lr.GEN, elem_bytes=Wd.widths)
        ctx.shard_rows_set_linear(sh, sysb)
        good = ctx.shard_rows_set_derived(sh, sysb, Wd.pairs)
        out["good"] = [good.n_slots, good.n_waves, good.n_exchanges, good.local_targets, good.exchange_bytes]
        by_slot = dict(Wd.pairs)
        t0, t1 = Wd.targets[0], Wd.targets[1]
        prod_row = int(np.flatnonzero(Wd.widths == pkg.ELEM_PRODUCT)[0])
        on_prod = pkg.LinearSystem.make([0, 2], [prod_row * l + 1, 7], [pkg.COEF_NEG_ONE, pkg.COEF_ONE])
        small = pkg.DerivedShardInfo()
        small.struct_bytes = C.sizeof(pkg.DerivedShardInfo) - 8
        beyond = Wd.system.to_binding(pkg, slots=Wd.system.slots[:-1] + [len(Wd.kinds) * l])
        out["refused"] = {"twice": call(sh, [(t0, by_slot[t0]), (t0, by_slot[t0])]),
                          "no_such_constraint": call(sh, [(t0, Wd.system.n_constraints)]),
                          "absent": call(sh, [(t0, by_slot[t1])]),
                          "table_coefficient": call(sh, [(t0, Wd.check_of[t0])]),
                          "on_product_row": call(sh, [(prod_row * l + 1, 0)], system=on_prod),
                          "system_rejected": call(sh, [(t0, by_slot[t0])], system=beyond),
                          "small_info": call(sh, Wd.pairs, info=C.byref(small))}
        root_, seed1 = ctx.shard_rows_commit(sh)      # the list set first is still in force
        got = ol.from_limbs(ctx.shard_rows_read_slots(sh, Wd.targets))
        proof, pi = ctx.shard_rows_prove(sh, None, None)
        out.update(root=root_.hex(), seed1=seed1.hex(), sha=sha(proof), wrong=[t for t, v in zip(Wd.targets, got) if v != Wd.w[t]])
        # removed: the shipped rows are committed as they are
        ctx.shard_rows_restart(sh, packed)
        gone = ctx.shard_rows_set_derived(sh, None, None)
        out["gone"] = [gone.n_slots, gone.n_waves]
        r2, s2 = ctx.shard_rows_commit(sh)
        p2, _ = ctx.shard_rows_prove(sh, None, None)
        out.update(plain_root=r2.hex(), plain_seed1=s2.hex(), plain_sha=sha(p2))
        # set again (the list survives restart: set before it), then other table values: they do not reach the list
        ctx.shard_rows_set_derived(sh, sysb, Wd.pairs)
        ctx.shard_rows_restart(sh, packed)
        ctx.shard_rows_set_linear_values(sh, [(v + 1) % dr.P for v in Wd.system.coefs])
        r3, s3 = ctx.shard_rows_commit(sh)
        got3 = ol.from_limbs(ctx.shard_rows_read_slots(sh, Wd.targets))
        out.update(values_root=r3.hex(), values_wrong=[t for t, v in zip(Wd.targets, got3) if v != Wd.w[t]])
        ctx.shard_rows_prove(sh, None, None)
        ctx.shard_destroy(sh)
        syn = ctx.shard_prepare(pkg.Context.make_job(700, 0, generated_at=77), 0, 1, comm)
        out["synthetic_shard"] = call(syn, Wd.pairs)
        ctx.shard_destroy(syn)
        want, plain = Wd.oracle(Wd.expected_rows), Wd.oracle(Wd.shipped_rows)
        out.update(oracle_root=want["root"].hex(), oracle_seed1=want["stage1_seed"].hex(), oracle_sha=sha(want["proof"]),
                   oracle_plain_root=plain["root"].hex(), oracle_plain_seed1=plain["stage1_seed"].hex(), oracle_plain_sha=sha(plain["proof"]))
    print(json.dumps(out))
    ctx.close()
    g.close()
''')

# name -> (world, transport, LINEAR rows, triples, the rank that is dealt no target or -1, host / device rows)
CASES = {
    "gloo_2": (2, None, 150, 60, -1, "host"),
    "ipc_2": (2, "ipc", 150, 60, -1, "host"),
    "ipc_2_device_rows": (2, "ipc", 150, 60, -1, "device"),
    "ipc_4_one_rank_without_targets": (4, "ipc", 150, 60, 3, "host"),
    "ipc_2_two_rounds": (2, "ipc", 500, 200, -1, "host"),
}


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def run(tmp_path, world, comm, *args, timeout=300):
    script = tmp_path / "shard_derived_worker.py"
    script.write_text(WORKER)
    outs = mr.run_ranks(mr.python_argv(script, ROOT, *args), world, mr.rendezvous_env(world, comm), timeout=timeout)
    outs = sorted((mr.last_json(o) for o, _ in outs), key=lambda d: d["rank"])
    assert len(outs) == world
    return outs


@pytest.mark.parametrize("name", list(CASES))
def test_world_built_against_the_deal_equals_python_integers_oracle_and_one_gpu(amd, tmp_path, name):
    world, comm, n_lin, n_tri, idle, where = CASES[name]
    # the world on the host first: its constructor asserts every condition the case relies on (ShardWorld.conditions)
    Wd = sdr.world(amd, world, n_lin, n_tri, idle=None if idle < 0 else idle)
    want = [sdr.shard_info(Wd.system, Wd.pairs, Wd.owner, sdr.L, q, world)[0] for q in range(world)]
    assert want[0]["n_waves"] == 4 and want[0]["n_exchanges"] == 3 and want[0]["exchange_bytes"] > 0
    if name == "ipc_2_two_rounds":
        assert Wd.rounds == 2 and len(Wd.kinds) == 1100
        mine = np.flatnonzero(Wd.owner == 0)
        assert (np.diff(mine) != 1).any()                              # a rank's local rows are not a contiguous global range
    if idle >= 0:
        assert want[idle]["local_targets"] == 0 and want[idle]["exports"] > 0
    outs = run(tmp_path, world, comm, "world", n_lin, n_tri, idle, where)
    r0 = outs[0]
    assert r0["oracle_valid"] == [1, 1, 1]
    assert (r0["ref_root"], r0["ref_seed1"], r0["ref_sha"]) == (r0["oracle_root"], r0["oracle_seed1"], r0["oracle_sha"]), "the one-GPU envelope differs from the oracle's"
    for q, o in enumerate(outs):
        print(name, "rank", q, "local rows", o["local_rows"], "info", o["info"])
        assert o["wrong"] == [], "rank %d: targets that differ from the Python integers: %r" % (q, o["wrong"])
        assert o["info"] == want[q] and o["count"] == want[q], o
        assert (o["root"], o["seed1"]) == (r0["oracle_root"], r0["oracle_seed1"]), o
        assert o["sha"] == r0["oracle_sha"], "rank %d: the sharded envelope differs from the oracle's" % q
        assert o["sha"] == r0["ref_sha"], "rank %d: the sharded envelope differs from lig_rows_prove with lig_rows_set_derived" % q
        assert o["valid"] == [1, 1, 1], o
        assert o["again"], "rank %d: restart + commit + prove gave other bytes" % q
        assert o["rounds"] == Wd.rounds


def test_recorded_guest_is_row_local_and_exchanges_nothing(tmp_path):
    outs = run(tmp_path, 2, "ipc", "guest")
    r0 = outs[0]
    assert r0["oracle_valid"] == [1, 1, 1]
    for o in outs:
        assert o["local_rows"] > 0
        assert o["info"]["n_slots"] == o["reps"] and o["info"]["n_waves"] == 1 and o["info"]["local_targets"] > 0
        assert (o["info"]["n_exchanges"], o["info"]["exchange_bytes"], o["info"]["imports"], o["info"]["exports"], o["info"]["imported_terms"]) == (0, 0, 0, 0, 0), o
        assert (o["root"], o["seed1"], o["sha"]) == (r0["oracle_root"], r0["oracle_seed1"], r0["oracle_sha"]), o
        assert o["valid"] == [1, 1, 1]
    assert sum(o["info"]["local_targets"] for o in outs) == r0["reps"]


def test_diagnose_sees_the_derived_values(amd, tmp_path):
    Wd = sdr.world(amd, 2, 150, 60)
    outs = run(tmp_path, 2, "ipc", "diagnose", 150, 60, -1, "host")
    for o in outs:
        assert o["violated"] == [Wd.check_of[Wd.t_in]] and o["n_linear"] == 1, o      # the check constraint of t_in, and no defining constraint
        assert o["t_in_value"] == o["moved"] and o["others_wrong"] == [], o
    assert outs[0] == dict(outs[1], rank=0, local_rows=outs[0]["local_rows"], info=outs[0]["info"], count=outs[0]["count"])


def test_state_and_refusals_on_one_rank(tmp_path):
    out = run(tmp_path, 1, None, "state")[0]
    E_ARG, E_STATE = -1, -3
    W = dr.world(hip_lib.load())
    assert out["good"] == [len(W.pairs), 3, 0, len(W.pairs), 0]
    assert out["refused"] == dict(twice=E_ARG, no_such_constraint=E_ARG, absent=E_ARG, table_coefficient=E_ARG, on_product_row=E_ARG,
                                  system_rejected=E_ARG, small_info=E_ARG), out["refused"]
    # every refused list left the first one in force: the commit is the oracle's over the expected rows
    assert out["wrong"] == [] and (out["root"], out["seed1"], out["sha"]) == (out["oracle_root"], out["oracle_seed1"], out["oracle_sha"])
    assert out["gone"] == [0, 0]
    assert (out["plain_root"], out["plain_seed1"], out["plain_sha"]) == (out["oracle_plain_root"], out["oracle_plain_seed1"], out["oracle_plain_sha"])
    assert out["values_wrong"] == [] and out["values_root"] == out["oracle_root"]
    assert out["synthetic_shard"] == E_STATE
