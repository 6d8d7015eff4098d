#!/usr/bin/env python3
"""What the sparse linear system buys on the SHARDED rows entry (lig_shard_rows_set_linear), in ONE command on one box.

Shape: the 2^24-constraint trace of bench.py (k = 8192, l = 8000, linear rows), dealt over W ranks by lig_shard_rows_plan; every rank
ships its own rows from pinned host memory (lig_shard_rows_restart -> _commit -> _prove, one trace at a time).  Per world size the
legs ALTERNATE `--rounds` times on the same shard:

  (a) the existing path: the rank's dense randomness rows from pinned host memory with every proof (runs on the parent commit too:
      --legs a --pkg-dir <a build of that commit>)
  (b) the system resident (set once, outside the timed region): lig_shard_rows_prove(local_rands = NULL)

The system is the statement of the synthetic stream -- one single-term constraint per witness slot, coefficient +1, constraint c = slot
c -- whose randomness rows are exactly the dense rows of (a), so both legs must give the SAME proof bytes (checked on every rank).  Its
table is empty (b would be 2^24 table entries), so leg (b) hands over the constant leg (a) reports, as tools/bench_linear_system.py does.

W = 1 is the measurement.  W > 1 here means W processes on the ONE GPU over comm_ipc: `shared_device: true`, a functional run whose
times say nothing about a node; what it does show is every rank's `local_terms` / `sampled_constraints`.
Every world is a step of its own: each rank runs under `timeout -k 10`, a rank that fails ends the run, at most 16 processes hold the GPU.
Prints one JSON line per world and a last line with all of them."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import signal
import socket
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_, K_, N_ = 8000, 8192, 32768
MAX_PROCS = 16


def load_pkg(pkg_dir):
    mods = {}
    for name, rel in (("ligero_prover_amd", "__init__.py"), ("lig_dist", "dist.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(pkg_dir, rel))
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    return mods["ligero_prover_amd"], mods["lig_dist"]


def synth_key():
    import hashlib
    return hashlib.sha256(b"lig-synth" + (1).to_bytes(8, "little")).digest()     # bench.py: synth_key()


def worker(a):
    import hashlib
    import numpy as np
    import torch
    pkg, dist = load_pkg(a.pkg_dir)
    legs = a.legs.split(",")
    g = dist.Group("gloo")
    ctx = pkg.Context(L_, K_, N_, device=0)
    n = 1 << a.log2_constraints
    R = -(-n // L_)
    per_row = np.full(R, L_, dtype=np.uint32)
    if n % L_:
        per_row[-1] = n % L_
    kinds = np.full(R, pkg.ROW_KINDS["LINEAR"] | pkg.ROW_DRAW_PAD, dtype=np.uint8)
    rounds, b = pkg.shard_rows_plan(kinds, g.world)
    mine = np.array(pkg.local_rows_of(b, g.rank, g.world), dtype=np.int64)

    def local_rows_of_stream(key):
        """the rank's rows of the dense stream keyed by `key` (generated on the device once, outside the timed region), pinned"""
        d = ctx.malloc(R * K_ * 32)
        ctx.rng_fill_rows(key, 0, per_row, d)
        full = torch.empty((R, K_, 8), dtype=torch.int32)
        ctx.check(ctx.L.lig_read(ctx.h, C.c_void_p(full.data_ptr()), d, R * K_ * 32))
        ctx.free(d)
        out = torch.empty((len(mine), K_, 8), dtype=torch.int32, pin_memory=True)
        if len(mine):
            out.copy_(full[torch.from_numpy(mine)])
        return out

    host = local_rows_of_stream(synth_key())
    comm = g.make_comm(pkg, ctx)
    sh = ctx.shard_rows_begin(kinds, host.numpy().view(np.uint32), g.rank, g.world, comm)
    _, seed = ctx.shard_rows_commit(sh)
    rands = local_rows_of_stream(seed)                         # the trace and therefore the seed are the same in every step
    rands_np = rands.numpy().view(np.uint32)
    _, info = ctx.shard_rows_prove(sh, rands_np, None)
    const_sum = bytes(info.const_sum)
    hp = C.c_void_p(host.data_ptr() if len(mine) else None)
    system, stats, set_ms = None, None, None
    if "b" in legs:
        rows_of = np.repeat(np.arange(R, dtype=np.uint64), per_row)
        cols = np.arange(n, dtype=np.uint64) - np.repeat(np.cumsum(per_row, dtype=np.uint64) - per_row, per_row)
        system = pkg.LinearSystem.make(np.arange(n + 1, dtype=np.uint32), (rows_of * L_ + cols).astype(np.uint32), np.full(n, pkg.COEF_ONE, dtype=np.uint32))

    def steps(leg, count):
        proof = None
        for _ in range(count):
            ctx.check(ctx.L.lig_shard_rows_restart(sh, hp, 0))
            ctx.shard_rows_commit(sh)
            proof, info = ctx.shard_rows_prove(sh, rands_np if leg == "a" else None, None if leg == "a" else const_sum)
            if not (info.valid_code and info.valid_linear and info.valid_quad):
                raise SystemExit("prover self-check failed in leg (%s)" % leg)
        return proof

    ms = {leg: [] for leg in legs}
    sha = {}
    for _ in range(a.rounds):
        for leg in legs:
            if "b" in legs:                                        # the legs share the shard: the system comes and goes outside the timed region
                t0 = time.perf_counter()
                ctx.shard_rows_set_linear(sh, system if leg == "b" else None)
                if leg == "b":
                    set_ms = 1e3 * (time.perf_counter() - t0)
                    stats = ctx.shard_rows_linear_stats(sh)
            steps(leg, a.warmup)
            ctx.sync()
            g.barrier()
            t0 = time.perf_counter()
            proof = steps(leg, a.steps)
            ctx.sync()
            ms[leg].append(g.max_over_ranks(1e3 * (time.perf_counter() - t0) / a.steps))
            sha[leg] = hashlib.sha256(proof).hexdigest()
    ctx.shard_destroy(sh)
    out = {"rank": g.rank, "local_rows": int(len(mine)), "rounds": rounds, "ms_per_proof": ms, "proof_sha256": sha,
           "h2d_bytes_per_proof": {"a": int(host.numel() * 4 + rands.numel() * 4), "b": int(host.numel() * 4)}}
    if stats is not None:
        out.update(local_terms=stats[0], sampled_constraints=stats[1], set_linear_ms=set_ms)
    print(json.dumps(out), flush=True)
    ctx.close()
    g.close()


def free_port():
    s = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def run_world(a, world):
    """`world` ranks, each under its own `timeout -k 10`; the first rank that fails ends all of them"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    if world > 1:
        env.update(LIG_COMM="ipc", LIG_COMM_TAG="bsl%d_%d" % (os.getpid(), world))
    argv = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--log2-constraints", str(a.log2_constraints),
            "--steps", str(a.steps), "--warmup", str(a.warmup), "--rounds", str(a.rounds), "--legs", a.legs, "--pkg-dir", a.pkg_dir]
    files = [(tempfile.TemporaryFile(), tempfile.TemporaryFile()) for _ in range(world)]       # (not pipes: nobody reads while the ranks run)
    procs = [subprocess.Popen(argv, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=files[r][0], stderr=files[r][1], start_new_session=True)
             for r in range(world)]
    failed = None
    while failed is None and any(p.poll() is None for p in procs):
        failed = next((r for r, p in enumerate(procs) if p.poll() not in (None, 0)), None)
        time.sleep(0.1)
    if failed is None:
        failed = next((r for r, p in enumerate(procs) if p.returncode != 0), None)
    if failed is not None:
        time.sleep(3)                                              # the others fail by themselves (their text is the interesting one), or are ended here
        for p in procs:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
    outs = []
    for p, (fo, fe) in zip(procs, files):
        p.wait()
        fo.seek(0); fe.seek(0)
        outs.append((fo.read(), fe.read()))
        fo.close(); fe.close()
    if failed is not None:
        raise SystemExit("world %d: rank %d exited with %r\n%s" % (world, failed, procs[failed].returncode, outs[failed][1].decode(errors="replace")[-3000:]))
    ranks = sorted((json.loads([ln for ln in o.decode().splitlines() if ln.startswith("{")][-1]) for o, _ in outs), key=lambda d: d["rank"])
    legs = a.legs.split(",")
    res = {"world": world, "shared_device": world > 1, "constraints": 1 << a.log2_constraints, "steps": a.steps, "warmup": a.warmup, "legs": legs,
           "transport": "comm_ipc" if world > 1 else "none (one rank)", "local_rows": [r["local_rows"] for r in ranks]}
    for leg in legs:
        res["%s_ms_per_proof" % leg] = ranks[0]["ms_per_proof"][leg]           # (the maximum over the ranks, the same on every rank)
        res["%s_h2d_bytes_per_proof_and_rank" % leg] = [r["h2d_bytes_per_proof"][leg] for r in ranks]
    res["all_ranks_same_envelope"] = all(r["proof_sha256"] == ranks[0]["proof_sha256"] for r in ranks)
    if "a" in legs and "b" in legs:
        res["same_proof_bytes"] = res["all_ranks_same_envelope"] and ranks[0]["proof_sha256"]["a"] == ranks[0]["proof_sha256"]["b"]
        res["b_over_a_time"] = min(res["b_ms_per_proof"]) / min(res["a_ms_per_proof"])
    if "b" in legs:
        res["local_terms"] = [r["local_terms"] for r in ranks]
        res["sampled_constraints"] = [r["sampled_constraints"] for r in ranks]
        res["set_linear_ms"] = [round(r["set_linear_ms"], 1) for r in ranks]
    print(json.dumps(res), flush=True)
    if not res["all_ranks_same_envelope"] or res.get("same_proof_bytes") is False:
        raise SystemExit("world %d: the legs / ranks produced different proofs" % world)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-constraints", type=int, default=24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2, help="(a), (b) alternations")
    ap.add_argument("--worlds", default="1,2,8")
    ap.add_argument("--legs", default="a,b", help="`a` alone runs on a build without lig_shard_rows_set_linear")
    ap.add_argument("--pkg-dir", default=os.path.join(ROOT, "ligero-prover_amd"), help="binding + library to measure (an A/B build)")
    ap.add_argument("--timeout", type=int, default=420, help="seconds per rank (timeout -k 10)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.pkg_dir = os.path.abspath(a.pkg_dir)
    if a.worker:
        return worker(a)
    worlds = [int(w) for w in a.worlds.split(",")]
    if max(worlds) > MAX_PROCS:
        raise SystemExit("at most %d processes may hold the GPU" % MAX_PROCS)
    print(json.dumps({"bench_shard_linear": [run_world(a, w) for w in worlds]}))


if __name__ == "__main__":
    main()
