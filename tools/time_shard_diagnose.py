#!/usr/bin/env python3
"""What lig_shard_rows_diagnose costs next to lig_rows_diagnose, in ONE command on one box.  Records, asserts nothing about speed.

Shape: the 2^24 single-term-constraint trace of tools/time_diagnose.py (k = 8192, l = 8000, linear rows; constraint c = slot c, coefficient
+1, one right-hand side each, w_s = b_s from a table of 251 values), with 1 % of the witness slots changed after the right-hand sides
were fixed; the first `--cap` violated constraints are reported.  Three legs ALTERNATE `--rounds` times (one warm-up round in front):

  (a) lig_rows_diagnose on one GPU: the yardstick, measured in this run
  (b) lig_shard_rows_diagnose at W = 1: no collective, the one-GPU pass behind the sharded entry
  (c) lig_shard_rows_diagnose at W = 2, as two PROCESSES on the ONE GPU over comm_ipc: `shared_device: true`, a functional run -- both
      ranks' kernels and the "exchange" share one device, the times say nothing about a node with one GPU per rank.  What it shows is the
      split of the call into its phases: the library prints it with LIG_TRACE set (a drain of the stream after every phase, so the phases
      do not overlap and their sum is the call minus the host pass of lig_linear_check)

Rank 0 of the two processes runs (a) and (b) while rank 1 waits at a barrier; then both run (c).  The times are the library's own wall
time of the blocking call (lig_diag_info.ms_total): the host pass of lig_linear_check over the term list and the upload of the term list
included, on every rank.  The three legs must count the same violations (checked).
Writes a markdown file (default profiles/r14_shard_diagnose.md) and prints one JSON line."""
import argparse
import json
import os
import re
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

PHASES = ("partial", "exchange", "reduce", "records", "quadratic")
TRACE = re.compile(r"\[lig_trace\] shard_diagnose rank (\d+): " + " ".join(p + r" ([0-9.]+)" for p in PHASES) + " ms")


def worker(a):
    import importlib.util
    import numpy as np
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
    system = pkg.LinearSystem.make(np.arange(n + 1, dtype=np.uint32), cons, np.full(n, pkg.COEF_ONE, dtype=np.uint32), cons, cons % 251,
                                   list(range(1, 252)))
    c = pkg.Context(l, k, n_enc, device=0)
    comm2 = g.make_comm(pkg, c)
    _, b = pkg.shard_rows_plan(kinds, g.world)
    mine = pkg.local_rows_of(b, g.rank, g.world)
    sh2 = c.shard_rows_begin(kinds, rows[mine], g.rank, g.world, comm2, generated_at=1)
    c.shard_rows_commit(sh2)
    tr = sh1 = comm1 = None
    if g.rank == 0:
        tr, keep = c.rows_begin(kinds, rows, generated_at=1)
        c.rows_commit(tr)
        comm1 = c.ipc_comm("/lig_tsd_%d" % os.getpid(), 0, 1)
        sh1 = c.shard_rows_begin(kinds, rows, 0, 1, comm1, generated_at=1)
        c.shard_rows_commit(sh1)
    legs, counts, first = {"a": [], "b": [], "c": []}, {}, {}
    for rnd in range(a.rounds + 1):
        if g.rank == 0:
            for leg, call in (("a", lambda: c.rows_diagnose(tr, system, lin_cap=a.cap, quad_cap=0)),
                              ("b", lambda: c.shard_rows_diagnose(sh1, system, lin_cap=a.cap, quad_cap=0))):
                info, lin, _ = call()
                counts[leg], first[leg] = (int(info.n_linear_bad), int(info.n_linear_reported)), lin.tobytes()
                if rnd:
                    legs[leg].append(info.ms_total)
        g.barrier()
        info, lin, _ = c.shard_rows_diagnose(sh2, system, lin_cap=a.cap, quad_cap=0)
        counts["c"], first["c"] = (int(info.n_linear_bad), int(info.n_linear_reported)), lin.tobytes()
        if rnd:
            legs["c"].append(info.ms_total)
        g.barrier()
    want = (len(changed), min(a.cap, len(changed)))
    same = all(v == want for v in counts.values()) and len(set(first.values())) == 1
    c.shard_destroy(sh2)
    if g.rank == 0:
        c.shard_destroy(sh1)
        c.ipc_comm_destroy(comm1)
        c.trace_destroy(tr)
    print(json.dumps({"rank": g.rank, "legs": legs, "counts": counts, "same_output": same, "local_rows": len(mine), "changed": int(len(changed))}), flush=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_shard_diagnose.md"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    world = 2
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0", LIG_COMM="ipc",
               LIG_COMM_TAG="tsd%d" % os.getpid(), LIG_TRACE="1")
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
    phases = {}
    for _, err in outs:
        for m in TRACE.finditer(err):
            phases.setdefault(int(m.group(1)), []).append([float(v) for v in m.groups()[1:]])
    split = {r: {p: statistics.median(x[i] for x in v[-a.rounds:]) for i, p in enumerate(PHASES)} for r, v in sorted(phases.items())}
    legs = {"a": ranks[0]["legs"]["a"], "b": ranks[0]["legs"]["b"], "c": [max(x) for x in zip(*(r["legs"]["c"] for r in ranks))]}
    med = {key: statistics.median(v) for key, v in legs.items()}
    n = 1 << a.log2_constraints
    res = {"constraints": n, "rounds": a.rounds, "cap": a.cap, "changed_slots": ranks[0]["changed"], "violated_and_reported": ranks[0]["counts"]["c"],
           "a_rows_diagnose_ms": legs["a"], "b_shard_diagnose_w1_ms": legs["b"], "c_shard_diagnose_w2_ms": legs["c"], "median_ms": med,
           "b_over_a": med["b"] / med["a"], "c_world": world, "c_shared_device": True, "c_local_rows": [r["local_rows"] for r in ranks],
           "c_phase_median_ms_by_rank": split, "c_link_bytes_per_rank_out_and_in": 32 * n * (world - 1) // world,
           "same_output_in_all_legs": all(r["same_output"] for r in ranks)}
    print(json.dumps(res))
    fmt = lambda v: ", ".join("%.2f" % x for x in v)      # noqa: E731
    with open(a.out, "w") as f:
        f.write("# lig_shard_rows_diagnose next to lig_rows_diagnose (tools/time_shard_diagnose.py)\n\n")
        f.write("Trace: %d single-term constraints w_s = b_s over linear rows at l = %d, k = %d, %d slots (1 %%) changed: %d violated, the first %d "
                "reported -- the same counts and record bytes in all three legs.  %d rounds after one warm-up round, the legs alternating inside "
                "every round; times in ms: the library's own wall time of the blocking call (`lig_diag_info.ms_total`).  Nothing is asserted "
                "about speed.\n\n" % (n, bench.L_, bench.K_, res["changed_slots"], res["violated_and_reported"][0], res["violated_and_reported"][1], a.rounds))
        f.write("| leg | what | median ms | all rounds, ms |\n|---|---|---|---|\n")
        f.write("| (a) | `lig_rows_diagnose` on one GPU: the yardstick of this run | %.2f | %s |\n" % (med["a"], fmt(legs["a"])))
        f.write("| (b) | `lig_shard_rows_diagnose`, W = 1 (no collective) | %.2f | %s |\n" % (med["b"], fmt(legs["b"])))
        f.write("| (c) | `lig_shard_rows_diagnose`, W = 2 as two processes on the ONE GPU (`shared_device: true`, functional only; the slower rank; "
                "`LIG_TRACE` set: a drain after every phase) | %.2f | %s |\n\n" % (med["c"], fmt(legs["c"])))
        f.write("(b) / (a) = %.3f.\n\n" % res["b_over_a"])
        f.write("Phases of (c), median ms per rank (`[lig_trace] shard_diagnose`; local rows per rank: %s; 4 slices of 2^22 constraints at the "
                "default `LIG_DIAG_SLICE`):\n\n" % res["c_local_rows"])
        f.write("| rank | partial kernels | exchange (all-to-all) | reduce | records: uploads, scan, scatter, gather, merge | quadratic part |\n|---|---|---|---|---|---|\n")
        for r, s in split.items():
            f.write("| %d | %.2f | %.2f | %.2f | %.2f | %.2f |\n" % (r, s["partial"], s["exchange"], s["reduce"], s["records"], s["quadratic"]))
        f.write("\nNot in the phases: the host pass of `lig_linear_check` over the term list, which every rank makes before anything is launched.  "
                "The \"exchange\" of (c) is a copy inside one device; on a node with one GPU per rank it is 32 B x n_constraints x (W - 1) / W "
                "out and in per rank over the links (%d bytes here) -- a prediction, no such node was measured.\n" % res["c_link_bytes_per_rank_out_and_in"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
