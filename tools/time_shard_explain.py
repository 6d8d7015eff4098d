#!/usr/bin/env python3
"""What lig_shard_rows_explain costs next to lig_rows_explain, in ONE command on one box.  Records, asserts nothing about speed.

Shape: the 2^24 single-term-constraint trace of tools/time_shard_diagnose.py (k = 8192, l = 8000, linear rows; constraint c = slot c,
coefficient +1, one right-hand side each, w_s = b_s from a table of 251 values), with 1 % of the witness slots changed after the
right-hand sides were fixed.  Asked: the first 1 / 1024 / 65 536 violated constraints, every term reported.  Three legs ALTERNATE
`--rounds` times for every size (one warm-up round in front):

  (a) lig_rows_explain on one GPU: the yardstick, measured in this run (it uploads the whole term list)
  (b) lig_shard_rows_explain at W = 1 with LIG_SHARD_FORCE_EXCHANGE set: the exchange path with one rank (items on the host, only the
      asked terms uploaded, one all-gather per piece)
  (c) lig_shard_rows_explain at W = 2, as two PROCESSES on the ONE GPU over comm_ipc: `shared_device: true`, a functional run -- both
      ranks' kernels and the "exchange" share one device, the times say nothing about a node with one GPU per rank.  The library
      prints the split of the call into its phases with LIG_TRACE set (a drain of the stream after every phase)

Rank 0 of the two processes runs (a) and (b) while rank 1 waits at a barrier; then both run (c).  The times are the library's own wall
time of the blocking call (lig_explain_info.ms_total): the host pass of lig_linear_check over the term list included, on every rank.
The output arrays are allocated once and kept between calls, as a C caller keeps them.  The three legs must return the same bytes
(checked), and the records are checked against the trace's construction.
Writes a markdown file (default profiles/r17_shard_explain.md) and prints one JSON line."""
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

PHASES = ("part", "exchange", "sum", "records")
TRACE = re.compile(r"\[lig_trace\] shard_explain rank (\d+): " + " ".join(p + r" ([0-9.]+)" for p in PHASES) + " ms")


def worker(a):
    import ctypes as C
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
    changed = np.sort(rng.choice(n, size=n // 100, replace=False)).astype(np.uint32)
    rows.reshape(R * k, 8)[(changed.astype(np.int64) // l) * k + changed % l, 0] += 1000
    if max(a.asked) > len(changed):
        raise SystemExit("only %d constraints are violated at this size: --asked %s is too many" % (len(changed), a.asked))
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
        comm1 = c.ipc_comm("/lig_tse_%d" % os.getpid(), 0, 1)
        sh1 = c.shard_rows_begin(kinds, rows, 0, 1, comm1, generated_at=1)      # LIG_SHARD_FORCE_EXCHANGE is set: the exchange path
        c.shard_rows_commit(sh1)
    cap = max(a.asked)
    con_buf, terms_buf = np.zeros(cap, dtype=pkg.EXPLAIN_CONSTRAINT), np.zeros(cap, dtype=pkg.EXPLAIN_TERM)
    ptr = lambda arr: arr.ctypes.data_as(C.c_void_p)      # noqa: E731

    def explain(call, handle, asked):
        m = len(asked)
        info = pkg.ExplainInfo()
        info.struct_bytes = C.sizeof(pkg.ExplainInfo)
        c.check(call(handle, C.byref(system), ptr(asked), m, ptr(con_buf), ptr(terms_buf), m, C.byref(info)))
        return info, con_buf[:m].tobytes() + terms_buf[:int(info.n_terms_reported)].tobytes()

    def as_built(asked, raw):
        """the records from the trace's construction: one +1 term per constraint on its own slot, the changed value, b = table[s % 251]"""
        m = len(asked)
        con = np.frombuffer(raw[:m * pkg.EXPLAIN_CONSTRAINT.itemsize], dtype=pkg.EXPLAIN_CONSTRAINT)
        terms = np.frombuffer(raw[m * pkg.EXPLAIN_CONSTRAINT.itemsize:], dtype=pkg.EXPLAIN_TERM)
        w, rhs, res = (np.zeros((m, 8), dtype=np.uint32) for _ in range(3))
        w[:, 0], rhs[:, 0], res[:, 0] = asked % 251 + 1001, asked % 251 + 1, 1000
        return (len(terms) == m and (con["constraint"] == asked).all() and (con["n_terms"] == 1).all() and (con["first_term"] == np.arange(m)).all() and
                con["rhs"].tobytes() == rhs.tobytes() and con["residual"].tobytes() == res.tobytes() and (terms["slot"] == asked).all() and
                (terms["coef_index"] == pkg.COEF_ONE).all() and terms["value"].tobytes() == w.tobytes())

    legs = {"%s%d" % (leg, m): [] for leg in "abc" for m in a.asked}
    same = True
    for m in a.asked:
        asked = np.ascontiguousarray(changed[:m])
        for rnd in range(a.rounds + 1):
            raws = {}
            if g.rank == 0:
                for leg, call, handle in (("a", c.L.lig_rows_explain, tr), ("b", c.L.lig_shard_rows_explain, sh1)):
                    info, raws[leg] = explain(call, handle, asked)
                    if rnd:
                        legs["%s%d" % (leg, m)].append(info.ms_total)
            g.barrier()
            info, raws["c"] = explain(c.L.lig_shard_rows_explain, sh2, asked)
            if rnd:
                legs["c%d" % m].append(info.ms_total)
            g.barrier()
            same = same and len(set(raws.values())) == 1 and bool(as_built(asked, raws["c"]))
    c.shard_destroy(sh2)
    if g.rank == 0:
        c.shard_destroy(sh1)
        c.ipc_comm_destroy(comm1)
        c.trace_destroy(tr)
    print(json.dumps({"rank": g.rank, "legs": legs, "same_output": bool(same), "local_rows": len(mine), "changed": int(len(changed))}), flush=True)
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
    ap.add_argument("--asked", type=int, nargs=3, default=[1, 1024, 65536])
    ap.add_argument("--timeout", type=int, default=420, help="seconds per rank (timeout -k 10)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_shard_explain.md"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    world = 2
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0", LIG_COMM="ipc",
               LIG_COMM_TAG="tse%d" % os.getpid(), LIG_TRACE="1", LIG_SHARD_FORCE_EXCHANGE="1")
    argv = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--log2-constraints", str(a.log2_constraints),
            "--rounds", str(a.rounds), "--asked"] + [str(m) for m in a.asked]
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
    legs = {}
    for m in a.asked:
        legs["a%d" % m], legs["b%d" % m] = ranks[0]["legs"]["a%d" % m], ranks[0]["legs"]["b%d" % m]
        legs["c%d" % m] = [max(x) for x in zip(*(r["legs"]["c%d" % m] for r in ranks))]
    med = {key: statistics.median(v) for key, v in legs.items()}
    spread = {m: (max(legs["a%d" % m]) - min(legs["a%d" % m])) / med["a%d" % m] for m in a.asked}
    # the phases of the LAST size's (c) calls (rank 1 makes only those; rank 0's last lines are its (c) calls of the last rounds too: every
    # round ends with (c)) -- the trace lines of rank 0 alternate b, c, so take every second one from the end
    phases = {}
    for r, (_, err) in enumerate(outs):
        lines = [[float(v) for v in mt.groups()[1:]] for mt in TRACE.finditer(err) if int(mt.group(1)) == r]
        mine = lines[-1:-2 * a.rounds:-2] if r == 0 else lines[-a.rounds:]
        phases[r] = {p: statistics.median(x[i] for x in mine) for i, p in enumerate(PHASES)}
    n = 1 << a.log2_constraints
    res = {"constraints": n, "rounds": a.rounds, "asked": a.asked, "changed_slots": ranks[0]["changed"], "ms": legs, "median_ms": med,
           "b_over_a": {m: med["b%d" % m] / med["a%d" % m] for m in a.asked}, "a_spread_over_median": spread, "c_world": world, "c_shared_device": True,
           "c_local_rows": [r["local_rows"] for r in ranks], "c_phase_median_ms_by_rank_at_largest": phases,
           "c_link_bytes_in_per_rank": {m: 32 * world * m for m in a.asked}, "same_output_in_all_legs": all(r["same_output"] for r in ranks)}
    print(json.dumps(res))
    fmt = lambda v: ", ".join("%.2f" % x for x in v)      # noqa: E731
    with open(a.out, "w") as f:
        f.write("# lig_shard_rows_explain next to lig_rows_explain (tools/time_shard_explain.py)\n\n")
        f.write("Trace: %d single-term constraints w_s = b_s over linear rows at l = %d, k = %d, %d slots (1 %%) changed.  Asked: the first m violated "
                "constraints, every term reported (m terms) -- the same record bytes in all three legs, checked against the trace's construction.  "
                "%d rounds after one warm-up round, the legs alternating inside every round; times in ms: the library's own wall time of the blocking "
                "call (`lig_explain_info.ms_total`), output arrays kept between calls.  Nothing is asserted about speed.\n\n"
                % (n, bench.L_, bench.K_, res["changed_slots"], a.rounds))
        f.write("| m | leg | what | median ms | all rounds, ms |\n|---|---|---|---|---|\n")
        for m in a.asked:
            f.write("| %d | (a) | `lig_rows_explain` on one GPU: the yardstick of this run | %.2f | %s |\n" % (m, med["a%d" % m], fmt(legs["a%d" % m])))
            f.write("| %d | (b) | `lig_shard_rows_explain`, W = 1, `LIG_SHARD_FORCE_EXCHANGE=1` (the exchange path with one rank) | %.2f | %s |\n"
                    % (m, med["b%d" % m], fmt(legs["b%d" % m])))
            f.write("| %d | (c) | `lig_shard_rows_explain`, W = 2 as two processes on the ONE GPU (`shared_device: true`, functional only; the slower "
                    "rank; `LIG_TRACE` set: a drain after every phase) | %.2f | %s |\n" % (m, med["c%d" % m], fmt(legs["c%d" % m])))
        f.write("\n| m | (b) / (a), medians | round-to-round spread of (a): (max - min) / median |\n|---|---|---|\n")
        for m in a.asked:
            f.write("| %d | %.3f | %.3f |\n" % (m, res["b_over_a"][m], spread[m]))
        f.write("\n(a) uploads the whole term list (8 B x %d terms and the index) on every call; (b) and (c) form the asked items on the host and "
                "upload only those.  All three make the host pass of `lig_linear_check` over the whole term list first.  (b) and (c) run with "
                "`LIG_TRACE` set, which adds a drain of the stream after every phase; (a) has no phases to print.\n\n" % n)
        f.write("Phases of (c) at m = %d, median ms per rank (`[lig_trace] shard_explain`; local rows per rank: %s):\n\n" % (a.asked[-1], res["c_local_rows"]))
        f.write("| rank | part kernels | exchange (all-gather) | sum | records: uploads, table, fill, finish, copy back |\n|---|---|---|---|---|\n")
        for r, s in sorted(phases.items()):
            f.write("| %d | %.2f | %.2f | %.2f | %.2f |\n" % (r, s["part"], s["exchange"], s["sum"], s["records"]))
        f.write("\nThe \"exchange\" of (c) is a copy inside one device; on a node with one GPU per rank it is 32 B x W x m in per rank over the "
                "links (%d bytes at m = %d) -- a prediction, no such node was measured.\n" % (32 * world * a.asked[-1], a.asked[-1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
