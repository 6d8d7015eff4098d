"""GPU: product entries of derived slots on the sharded rows entry (lig_shard_rows_set_derived with (slot, DERIVED_PRODUCT) entries) -- W
ranks as W processes on the one GPU (the worker pattern of tests/test_gpu_shard_derived.py).

Expected bytes never come from the sharded derived path: the values of the listed slots are the Python integers of
tests/derived_product_ref.py placed against the deal, root, stage-1 seed and envelope are the oracle's prover over the rows that carry those
integers (computed on rank 0, compared with every rank's results here, in the parent) and the one-GPU lig_rows_set_derived envelope; the
per-rank counts are the Python restatement (derived_product_ref.shard_info) and the host-only lig_derived_shard_count.  The list has a
derived x whose defining constraint imports a term from another rank and a re-formed z that a target of another rank reads; both hold by
construction and are asserted on the host (derived_product_ref.World)."""
import os
import textwrap

import pytest

import derived_product_ref as dpr
import hip_lib
import multirank as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

WORKER = textwrap.dedent('''
    import hashlib, importlib.util, json, os, sys
    import numpy as np
    root = sys.argv[1]
    l, k, n = 320, 512, 2048
    sys.path.insert(0, os.path.join(root, "tests"))
    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, "ligero-prover_amd", rel))
        m = importlib.util.module_from_spec(spec); sys.modules[name] = m; spec.loader.exec_module(m); return m
    pkg = load("ligero_prover_amd", "__init__.py")
    dist = load("lig_dist", "dist.py")
    import derived_product_ref as dpr, linear_ref as lr, oracle_lib as ol
    sha = lambda b: hashlib.sha256(bytes(b)).hexdigest()
    g = dist.Group("gloo")
    ctx = pkg.Context(l, k, n, device=0)
    comm = g.make_comm(pkg, ctx)
    out = {"rank": g.rank}
    Wd = dpr.world(pkg, world_size=g.world)
    sysb = Wd.system.to_binding(pkg)
    mine = pkg.local_rows_of(Wd.boundaries, g.rank, g.world)
    kk, _ = Wd.ship(pkg)
    local = Wd.pack_local(pkg, Wd.shipped_rows, mine)
    sh = ctx.shard_rows_begin(kk, local, g.rank, g.world, comm, generated_at=lr.GEN, elem_bytes=Wd.widths, wide_per_row=Wd.wide)
    ctx.shard_rows_set_linear(sh, sysb)
    info = ctx.shard_rows_set_derived(sh, sysb, Wd.pairs)
    root_, seed1 = ctx.shard_rows_commit(sh)
    got = ol.from_limbs(ctx.shard_rows_read_slots(sh, Wd.listed))
    di, lin, quad = ctx.shard_rows_diagnose(sh, sysb)
    da, lin_a, quad_a = ctx.shard_rows_diagnose_attached(sh)
    # explain over the check constraints of re-formed products (z_far: held by one rank, read by a target of another; c4: the second
    # product of the five waves), explain_slots over re-formed slots; with the term list and against the attached system
    value = lambda rec: ol.from_limbs(np.frombuffer(rec["value"].tobytes(), dtype=np.uint32).reshape(-1, 8))
    products = [Wd.z_far, Wd.c4, Wd.z_a, Wd.z_d]
    checks = sorted(Wd.check_of[t] for t in products)
    asked = sorted([Wd.z_far, Wd.z_b, Wd.c2, Wd.t_back])
    explain_wrong = []
    for name, (_, cons, terms) in (("explain", ctx.shard_rows_explain(sh, sysb, checks)), ("explain_attached", ctx.shard_rows_explain_attached(sh, checks))):
        by = {(int(t["constraint"]), int(t["slot"])): v for t, v in zip(terms, value(terms))}
        explain_wrong += [(name, t) for t in products if by.get((Wd.check_of[t], t)) != Wd.w[t]]
        if cons["residual"].any() or len(cons) != len(checks):
            explain_wrong.append((name, "residual"))
    for name, (_, srec, sterms) in (("explain_slots", ctx.shard_rows_explain_slots(sh, sysb, asked)), ("explain_slots_attached", ctx.shard_rows_explain_slots_attached(sh, asked))):
        if [int(s) for s in srec["slot"]] != asked or value(srec) != [Wd.w[t] for t in asked] or sterms["residual"].any():
            explain_wrong.append((name, "slots"))
    proof, pi = ctx.shard_rows_prove(sh, None, None)
    ctx.shard_rows_restart(sh, local)
    again = ctx.shard_rows_commit(sh) == (root_, seed1)
    proof2, pi2 = ctx.shard_rows_prove(sh, None, None)
    out.update(local_rows=len(mine), info=info.as_dict(), count=pkg.derived_shard_count(sysb, Wd.kinds, l, Wd.pairs, Wd.widths, g.rank, g.world).as_dict(),
               root=root_.hex(), seed1=seed1.hex(), sha=sha(proof), valid=[pi.valid_code, pi.valid_linear, pi.valid_quad],
               again=bool(again and proof2 == proof), wrong=[t for t, v in zip(Wd.listed, got) if v != Wd.w[t]],
               diagnose=[int(di.n_linear_bad), int(di.n_quad_bad), int(da.n_linear_bad), int(da.n_quad_bad)], explain_wrong=explain_wrong)
    ctx.shard_destroy(sh)
    if g.rank == 0:
        want = Wd.oracle(Wd.expected_rows)
        out.update(oracle_root=want["root"].hex(), oracle_seed1=want["stage1_seed"].hex(), oracle_sha=sha(want["proof"]), oracle_valid=list(want["valid"]))
        tr, keep = ctx.rows_begin(kk, Wd.ship(pkg)[1], generated_at=lr.GEN, elem_bytes=Wd.widths, wide_per_row=Wd.wide)
        ctx.rows_set_linear(tr, sysb)
        ctx.rows_set_derived(tr, sysb, Wd.pairs)
        r1, s1 = ctx.rows_commit(tr)
        ref, rinfo = ctx.rows_prove(tr, None, None)
        ctx.trace_destroy(tr)
        out.update(ref_root=r1.hex(), ref_seed1=s1.hex(), ref_sha=sha(ref))
    print(json.dumps(out))
    ctx.close()
    g.close()
''')


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


@pytest.mark.parametrize("world,comm", [(1, None), (2, "ipc")])
def test_products_on_a_shard_equal_python_integers_oracle_and_one_gpu(amd, tmp_path, world, comm):
    # the world on the host first: its constructor asserts what the case relies on (an imported term of a derived x, a re-formed z read
    # by another rank and sent in the reader's wave)
    Wd = dpr.world(amd, world_size=world)
    want = [dpr.shard_info(Wd.system, Wd.pairs, Wd.owner, dpr.L, q, world)[0] for q in range(world)]
    assert want[0]["n_waves"] == 5 and (world == 1 or (want[0]["n_exchanges"] >= 2 and sum(x["imported_terms"] for x in want) >= 3))
    script = tmp_path / "shard_derived_products_worker.py"
    script.write_text(WORKER)
    outs = mr.run_ranks(mr.python_argv(script, ROOT), world, mr.rendezvous_env(world, comm), timeout=300)
    outs = sorted((mr.last_json(o) for o, _ in outs), key=lambda d: d["rank"])
    assert len(outs) == world
    r0 = outs[0]
    assert r0["oracle_valid"] == [1, 1, 1]
    assert (r0["ref_root"], r0["ref_seed1"], r0["ref_sha"]) == (r0["oracle_root"], r0["oracle_seed1"], r0["oracle_sha"]), "the one-GPU envelope differs from the oracle's"
    for q, o in enumerate(outs):
        print("W =", world, "rank", q, "local rows", o["local_rows"], "info", o["info"])
        assert o["wrong"] == [], "rank %d: listed slots that differ from the Python integers: %r" % (q, o["wrong"])
        assert o["info"] == want[q] and o["count"] == want[q], o
        assert (o["root"], o["seed1"]) == (r0["oracle_root"], r0["oracle_seed1"]), o
        assert o["sha"] == r0["oracle_sha"] == r0["ref_sha"], "rank %d: the sharded envelope differs" % q
        assert o["valid"] == [1, 1, 1] and o["diagnose"] == [0, 0, 0, 0], o
        assert o["explain_wrong"] == [], "rank %d: explain readers that differ from the Python integers: %r" % (q, o["explain_wrong"])
        assert o["again"], "rank %d: restart + commit + prove gave other bytes" % q
