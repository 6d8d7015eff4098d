#!/usr/bin/env python3
"""What a new statement and a diagnose cost on the sharded rows entry with and without the calls that use what a rank already holds, in
ONE command on one box.  Records, asserts nothing about speed.

Shape: the 2^24 single-term-constraint trace of tools/time_shard_diagnose.py (k = 8192, l = 8000, linear rows; constraint c = slot c,
coefficient +1, one right-hand side each, w_s = b_s from a table of 251 values), with 1 % of the witness slots changed after the
right-hand sides were fixed; the first `--cap` violated constraints are reported.  Two legs, each a pair that ALTERNATES `--rounds` times
(one warm-up round in front), at W = 1 and at W = 2:

  leg 1  a new statement:  (a) lig_shard_rows_set_linear again  against  (b) lig_shard_rows_set_linear_values with the same table
         (a clock around the call: (a) is synchronous; (b) returns with the upload and the conversion of the 251 entries queued on the
         side stream, and the clock also covers a wait for that stream)
  leg 2  a diagnose:       (c) lig_shard_rows_diagnose with the term list  against  (d) lig_shard_rows_diagnose_attached
         (the library's own wall time of the blocking call, lig_diag_info.ms_total); both must return the same counts and record bytes

W = 2 runs as two PROCESSES on the ONE GPU over comm_ipc: `shared_device: true`, a functional run -- both ranks' kernels and the
"exchange" share one device, the times say nothing about a node with one GPU per rank; the slower rank is recorded.  Rank 0 runs the
W = 1 legs while rank 1 waits at a barrier.
Writes a markdown file (default profiles/r18_shard_values.md) and prints one JSON line."""
import argparse
import json
import os
import signal
import socket
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the shape and the package loader; importing it runs nothing)

LEGS = ("a", "b", "c", "d")


def worker(a):
    import importlib.util
    import numpy as np
    import torch
    pkg = bench.load_pkg()
    spec = importlib.util.spec_from_file_location("lig_dist", os.path.join(ROOT, "ligero-prover_amd", "dist.py"))
    dist = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dist)
    g = dist.Group("gloo")
    l, k, n_enc = bench.L_, bench.K_, bench.N_
    n = 1 << a.log2_constraints
    R = -(-n // l)
    kinds = np.full(R, pkg.ROW_KINDS["LINEAR"] | pkg.ROW_DRAW_PAD, dtype=np.uint8)
    rows = np.zeros((R, k, 8), dtype=np.uint32)
    rows[:, :l, 0] = (np.arange(R * l, dtype=np.uint64) % 251 + 1).reshape(R, l)        # w[s] = table[s % 251]
    rng = np.random.default_rng(12)
    changed = np.sort(rng.choice(n, size=n // 100, replace=False))
    rows.reshape(R * k, 8)[(changed // l) * k + changed % l, 0] += 1000
    cons = np.arange(n, dtype=np.uint32)
    table = list(range(1, 252))
    system = pkg.LinearSystem.make(np.arange(n + 1, dtype=np.uint32), cons, np.full(n, pkg.COEF_ONE, dtype=np.uint32), cons, cons % 251, table)
    c = pkg.Context(l, k, n_enc, device=0)
    comm2 = g.make_comm(pkg, c)
    _, b = pkg.shard_rows_plan(kinds, g.world)
    mine = pkg.local_rows_of(b, g.rank, g.world)
    sh2 = c.shard_rows_begin(kinds, rows[mine], g.rank, g.world, comm2, generated_at=1)
    c.shard_rows_set_linear(sh2, system)
    c.shard_rows_commit(sh2)
    sh1 = comm1 = None
    if g.rank == 0:
        comm1 = c.ipc_comm("/lig_tsv_%d" % os.getpid(), 0, 1)
        sh1 = c.shard_rows_begin(kinds, rows, 0, 1, comm1, generated_at=1)
        c.shard_rows_set_linear(sh1, system)
        c.shard_rows_commit(sh1)

    def clocked(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def round_of(sh, legs, counts, first, keep):
        for leg, call in (("a", lambda: c.shard_rows_set_linear(sh, system)), ("b", lambda: c.shard_rows_set_linear_values(sh, table))):
            ms = clocked(call)
            if keep:
                legs[leg].append(ms)
        for leg, call in (("c", lambda: c.shard_rows_diagnose(sh, system, lin_cap=a.cap, quad_cap=0)),
                          ("d", lambda: c.shard_rows_diagnose_attached(sh, lin_cap=a.cap, quad_cap=0))):
            info, lin, _ = call()
            counts[leg], first[leg] = (int(info.n_linear_bad), int(info.n_linear_reported)), lin.tobytes()
            if keep:
                legs[leg].append(info.ms_total)

    res = {w: ({x: [] for x in LEGS}, {}, {}) for w in (1, 2)}
    for rnd in range(a.rounds + 1):
        if g.rank == 0:
            round_of(sh1, *res[1], rnd)
        g.barrier()
        round_of(sh2, *res[2], rnd)
        g.barrier()
    want = (len(changed), min(a.cap, len(changed)))
    same = all(v == want for w in ((1, 2) if g.rank == 0 else (2,)) for v in res[w][1].values())
    same = same and all(len(set(res[w][2].values())) == 1 for w in ((1, 2) if g.rank == 0 else (2,)))
    c.shard_destroy(sh2)
    if g.rank == 0:
        c.shard_destroy(sh1)
        c.ipc_comm_destroy(comm1)
    print(json.dumps({"rank": g.rank, "w1": res[1][0], "w2": res[2][0], "counts": res[2][1], "same_output": same, "local_rows": len(mine),
                      "changed": int(len(changed))}), flush=True)
    c.close()
    g.close()
    return 0 if same else 1


def free_port():
    s = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-constraints", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per rank (timeout -k 10)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_shard_values.md"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    world = 2
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0", LIG_COMM="ipc",
               LIG_COMM_TAG="tsv%d" % os.getpid())
    argv = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--log2-constraints", str(a.log2_constraints),
            "--rounds", str(a.rounds), "--cap", str(a.cap)]
    files = [(tempfile.TemporaryFile(), tempfile.TemporaryFile()) for _ in range(world)]
    procs = [subprocess.Popen(argv, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=files[r][0], stderr=files[r][1], start_new_session=True)
             for r in range(world)]
    failed = None
    while failed is None and any(p.poll() is None for p in procs):
        failed = next((r for r, p in enumerate(procs) if p.poll() not in (None, 0)), None)
        time.sleep(0.1)
    if failed is None:
        failed = next((r for r, p in enumerate(procs) if p.returncode != 0), None)
    if failed is not None:
        time.sleep(3)                                              # the other rank fails by itself, or is ended here
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
        outs.append((fo.read().decode(errors="replace"), fe.read().decode(errors="replace")))
        fo.close(); fe.close()
    if failed is not None:
        raise SystemExit("rank %d exited with %r\n%s" % (failed, procs[failed].returncode, outs[failed][1][-3000:]))
    ranks = sorted((json.loads([ln for ln in o.splitlines() if ln.startswith("{")][-1]) for o, _ in outs), key=lambda d: d["rank"])
    w1 = ranks[0]["w1"]
    w2 = {x: [max(v) for v in zip(*(r["w2"][x] for r in ranks))] for x in LEGS}      # the slower rank of every round
    med = {"w1": {x: statistics.median(w1[x]) for x in LEGS}, "w2": {x: statistics.median(w2[x]) for x in LEGS}}
    n = 1 << a.log2_constraints
    res = {"constraints": n, "rounds": a.rounds, "cap": a.cap, "changed_slots": ranks[0]["changed"], "violated_and_reported": ranks[0]["counts"]["d"],
           "w1_ms": w1, "w2_ms": w2, "median_ms": med, "w2_shared_device": True, "w2_local_rows": [r["local_rows"] for r in ranks],
           "same_output_in_all_legs": all(r["same_output"] for r in ranks)}
    print(json.dumps(res))
    fmt = lambda v: ", ".join("%.2f" % x for x in v)      # noqa: E731
    what = {"a": "`lig_shard_rows_set_linear` again (clock around the call)", "b": "`lig_shard_rows_set_linear_values` (clock around the call and a wait for the side stream)",
            "c": "`lig_shard_rows_diagnose` with the term list (`ms_total`)", "d": "`lig_shard_rows_diagnose_attached` (`ms_total`)"}
    with open(a.out, "w") as f:
        f.write("# A new statement and a diagnose on the sharded rows entry (tools/time_shard_values.py)\n\n")
        f.write("Trace: %d single-term constraints w_s = b_s over linear rows at l = %d, k = %d, a table of 251 values, %d slots (1 %%) changed: %d "
                "violated, the first %d reported -- the same counts and record bytes from (c) and (d) in both worlds.  %d rounds after one warm-up "
                "round, the legs alternating inside every round; times in ms.  Nothing is asserted about speed.\n\n"
                % (n, bench.L_, bench.K_, res["changed_slots"], res["violated_and_reported"][0], res["violated_and_reported"][1], a.rounds))
        for key, title, legs in (("w1", "W = 1 (no collective)", w1),
                                 ("w2", "W = 2 as two processes on the ONE GPU (`shared_device: true`, functional only; the slower rank of every round; "
                                        "local rows per rank: %s)" % res["w2_local_rows"], w2)):
            f.write("## %s\n\n| leg | what | median ms | all rounds, ms |\n|---|---|---|---|\n" % title)
            for x in LEGS:
                f.write("| (%s) | %s | %.2f | %s |\n" % (x, what[x], med[key][x], fmt(legs[x])))
            f.write("\n(a) / (b) = %.1f, (c) / (d) = %.1f.\n\n" % (med[key]["a"] / med[key]["b"], med[key]["c"] / med[key]["d"]))
        f.write("(a) and (c) contain the host pass of `lig_linear_check` over the term list and its upload, on every rank.  The table of this trace has "
                "251 entries: (b) does not grow with the number of constraints, only with the table.  The \"exchange\" of W = 2 is a copy inside one "
                "device; no node with one GPU per rank was measured.\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
