#!/usr/bin/env python3
"""What lig_shard_rows_explain_attached costs next to lig_shard_rows_explain, in ONE command on one box.  Records, asserts nothing about
speed.

Shape: the 2^24 single-term-constraint trace of tools/time_shard_explain.py (k = 8192, l = 8000, linear rows; constraint c = slot c,
coefficient +1, one right-hand side each, w_s = b_s from a table of 251 values), with 1 % of the witness slots changed after the
right-hand sides were fixed.  The system is set on every shard with lig_shard_rows_set_linear.  Asked: the first 1 / 1024 / 65 536
violated constraints, every term reported.  Two legs ALTERNATE `--rounds` times for every size (one warm-up round in front), in two
worlds:

  (A) lig_shard_rows_explain with the term list of the whole trace: the yardstick, measured in this run
  (B) lig_shard_rows_explain_attached: the rank's share as it lies on its device, no term list

  W = 1 with LIG_SHARD_FORCE_EXCHANGE set: the exchange path with one rank
  W = 2 as two PROCESSES on the ONE GPU over comm_ipc: `shared_device: true`, a functional run -- both ranks' kernels and the "exchange"
        share one device, the times say nothing about a node with one GPU per rank

Rank 0 of the two processes runs the W = 1 legs while rank 1 waits at a barrier; then both run the W = 2 legs.  The times are the
library's own wall time of the blocking call (lig_explain_info.ms_total); for (A) that includes the host pass of lig_linear_check over
the term list, on every rank.  The output arrays are allocated once and kept between calls, as a C caller keeps them.  All legs must
return the same bytes (checked), and the records are checked against the trace's construction.
--parent-root DIR: a tree of the parent commit with its library built; leg (A) is timed once more there, in the same command, to show
that the existing call has not changed.  --phases: one more world with LIG_TRACE set (a drain of the stream after every phase, so
its times are not the ones reported) prints the split of (B) into its phases.
Writes a markdown file (default profiles/r19_shard_explain_attached.md) and prints one JSON line."""
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
import bench  # noqa: E402  (the shape; importing it runs nothing)

PHASES = ("select", "exchange", "merge", "records")
TRACE = re.compile(r"\[lig_trace\] shard_explain_attached rank (\d+): " + " ".join(p + r" ([0-9.]+)" for p in PHASES) + " ms")


def load(name, path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def worker(a):
    import ctypes as C
    import numpy as np
    pkg = load("ligero_prover_amd", os.path.join(a.pkg_root, "ligero-prover_amd", "__init__.py"))
    dist = load("lig_dist", os.path.join(a.pkg_root, "ligero-prover_amd", "dist.py"))
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
    c.shard_rows_set_linear(sh2, system)
    c.shard_rows_commit(sh2)
    sh1 = comm1 = None
    if g.rank == 0:
        comm1 = c.ipc_comm("/lig_tsea_%d" % os.getpid(), 0, 1)
        sh1 = c.shard_rows_begin(kinds, rows, 0, 1, comm1, generated_at=1)      # LIG_SHARD_FORCE_EXCHANGE is set: the exchange path
        c.shard_rows_set_linear(sh1, system)
        c.shard_rows_commit(sh1)
    cap = max(a.asked)
    con_buf, terms_buf = np.zeros(cap, dtype=pkg.EXPLAIN_CONSTRAINT), np.zeros(cap, dtype=pkg.EXPLAIN_TERM)
    ptr = lambda arr: arr.ctypes.data_as(C.c_void_p)      # noqa: E731

    def explain(leg, handle, asked):
        m = len(asked)
        info = pkg.ExplainInfo()
        info.struct_bytes = C.sizeof(pkg.ExplainInfo)
        if leg == "A":
            c.check(c.L.lig_shard_rows_explain(handle, C.byref(system), ptr(asked), m, ptr(con_buf), ptr(terms_buf), m, C.byref(info)))
        else:
            c.check(c.L.lig_shard_rows_explain_attached(handle, ptr(asked), m, ptr(con_buf), ptr(terms_buf), m, C.byref(info)))
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

    which = "A" if a.only_a else "AB"
    legs = {"%s%d_%d" % (leg, w, m): [] for leg in which for w in (1, 2) for m in a.asked}
    same = True
    for m in a.asked:
        asked = np.ascontiguousarray(changed[:m])
        for rnd in range(a.rounds + 1):
            raws = {}
            if g.rank == 0:
                for leg in which:
                    info, raws[leg + "1"] = explain(leg, sh1, asked)
                    if rnd:
                        legs["%s1_%d" % (leg, m)].append(info.ms_total)
            g.barrier()
            for leg in which:
                info, raws[leg + "2"] = explain(leg, sh2, asked)
                if rnd:
                    legs["%s2_%d" % (leg, m)].append(info.ms_total)
                g.barrier()
            same = same and len(set(raws.values())) == 1 and bool(as_built(asked, raws[which[-1] + "2"]))
    c.shard_destroy(sh2)
    if g.rank == 0:
        c.shard_destroy(sh1)
        c.ipc_comm_destroy(comm1)
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


def run_world(a, tag, pkg_root, only_a=False, trace=False, rounds=None):
    """two rank processes of this file as workers -> ([rank 0's JSON, rank 1's JSON], [rank 0's stderr, rank 1's stderr])"""
    world = 2
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "LIG_TRACE")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0", LIG_COMM="ipc",
               LIG_COMM_TAG="tsea%s%d" % (tag, os.getpid()), LIG_SHARD_FORCE_EXCHANGE="1")
    if trace:
        env["LIG_TRACE"] = "1"
    argv = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--pkg-root", pkg_root, "--log2-constraints",
            str(a.log2_constraints), "--rounds", str(rounds or a.rounds), "--asked"] + [str(m) for m in a.asked] + (["--only-a"] if only_a else [])
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
        raise SystemExit("world %s: rank %d exited with %r\n%s" % (tag, failed, procs[failed].returncode, outs[failed][1][-3000:]))
    ranks = sorted((json.loads([ln for ln in o.splitlines() if ln.startswith("{")][-1]) for o, _ in outs), key=lambda d: d["rank"])
    return ranks, [e for _, e in outs]


def merged(ranks, which, asked):
    """W = 1: rank 0's times; W = 2: the slower rank of every round"""
    legs = {}
    for leg in which:
        for m in asked:
            legs["%s1_%d" % (leg, m)] = ranks[0]["legs"]["%s1_%d" % (leg, m)]
            legs["%s2_%d" % (leg, m)] = [max(x) for x in zip(*(r["legs"]["%s2_%d" % (leg, m)] for r in ranks))]
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-constraints", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--asked", type=int, nargs=3, default=[1, 1024, 65536])
    ap.add_argument("--timeout", type=int, default=420, help="seconds per rank (timeout -k 10)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_shard_explain_attached.md"))
    ap.add_argument("--parent-root", default=None, help="a tree of the parent commit with its library built: leg (A) once more there")
    ap.add_argument("--phases", action="store_true", help="one more world with LIG_TRACE set: the phases of (B)")
    ap.add_argument("--pkg-root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--only-a", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    ranks, _ = run_world(a, "n", ROOT)
    legs = merged(ranks, "AB", a.asked)
    ok = all(r["same_output"] for r in ranks)
    parent = None
    if a.parent_root:
        pranks, _ = run_world(a, "p", os.path.abspath(a.parent_root), only_a=True)
        parent = merged(pranks, "A", a.asked)
        ok = ok and all(r["same_output"] for r in pranks)
    phases = None
    if a.phases:
        _, errs = run_world(a, "t", ROOT, trace=True, rounds=1)
        phases = {}
        for r, err in enumerate(errs):          # the last lines of every rank are its W = 2 calls of the largest size (rank 0 alternates W = 1, W = 2)
            lines = [[float(v) for v in mt.groups()[1:]] for mt in TRACE.finditer(err) if int(mt.group(1)) == r]
            phases[r] = dict(zip(PHASES, lines[-1]))
    med = {key: statistics.median(v) for key, v in legs.items()}
    pmed = {key: statistics.median(v) for key, v in parent.items()} if parent else None
    n = 1 << a.log2_constraints
    res = {"constraints": n, "rounds": a.rounds, "asked": a.asked, "changed_slots": ranks[0]["changed"], "ms": legs, "median_ms": med,
           "b_over_a": {"W%d_%d" % (w, m): med["B%d_%d" % (w, m)] / med["A%d_%d" % (w, m)] for w in (1, 2) for m in a.asked},
           "parent_ms": parent, "parent_median_ms": pmed, "w2_shared_device": True, "w2_local_rows": [r["local_rows"] for r in ranks],
           "b_phase_ms_by_rank_w2_at_largest": phases, "same_output_in_all_legs": ok}
    print(json.dumps(res))
    fmt = lambda v: ", ".join("%.2f" % x for x in v)      # noqa: E731
    what = {"A": "`lig_shard_rows_explain` with the term list", "B": "`lig_shard_rows_explain_attached`"}
    where = {1: "W = 1, `LIG_SHARD_FORCE_EXCHANGE=1` (the exchange path with one rank)",
             2: "W = 2 as two processes on the ONE GPU (`shared_device: true`, functional only; the slower rank)"}
    with open(a.out, "w") as f:
        f.write("# lig_shard_rows_explain_attached next to lig_shard_rows_explain (tools/time_shard_explain_attached.py)\n\n")
        f.write("Trace: %d single-term constraints w_s = b_s over linear rows at l = %d, k = %d, %d slots (1 %%) changed; the system set on every shard "
                "with `lig_shard_rows_set_linear`.  Asked: the first m violated constraints, every term reported (m terms) -- the same record bytes in "
                "all legs (%s), checked against the trace's construction.  %d rounds after one warm-up round, the legs alternating inside every round; "
                "times in ms: the library's own wall time of the blocking call (`lig_explain_info.ms_total`), output arrays kept between calls.  "
                "Nothing is asserted about speed.\n\n" % (n, bench.L_, bench.K_, res["changed_slots"], "checked: yes" if ok else "CHECK FAILED", a.rounds))
        f.write("| m | world | leg | median ms | all rounds, ms |\n|---|---|---|---|---|\n")
        for m in a.asked:
            for w in (1, 2):
                for leg in "AB":
                    key = "%s%d_%d" % (leg, w, m)
                    f.write("| %d | %s | (%s) %s | %.2f | %s |\n" % (m, where[w], leg, what[leg], med[key], fmt(legs[key])))
        f.write("\n| m | (B) / (A) at W = 1, medians | (B) / (A) at W = 2, medians |\n|---|---|---|\n")
        for m in a.asked:
            f.write("| %d | %.3f | %.3f |\n" % (m, res["b_over_a"]["W1_%d" % m], res["b_over_a"]["W2_%d" % m]))
        f.write("\n(A) makes the host pass of `lig_linear_check` over the whole term list and forms the asked items on the host of every rank; (B) reads "
                "no term list: one mark pass over the rank's local index (%d entries at W = 1), a scan, a collect, one header all-gather and the record "
                "all-gathers.\n" % n)
        if parent:
            f.write("\nLeg (A) once more on a build of the parent commit, same command, same shards (the system set as well), in a world of its own started after the first -- the two columns are not alternating legs, and the difference between them is what two worlds of the same code differ by:\n\n")
            f.write("| m | world | (A) here, median ms | (A) on the parent, median ms | parent, all rounds |\n|---|---|---|---|---|\n")
            for m in a.asked:
                for w in (1, 2):
                    key = "A%d_%d" % (w, m)
                    f.write("| %d | W = %d | %.2f | %.2f | %s |\n" % (m, w, med[key], pmed[key], fmt(parent[key])))
        else:
            f.write("\nLeg (A) was not timed on a build of the parent commit in this run (`--parent-root`).\n")
        if phases:
            f.write("\nPhases of (B) at W = 2, m = %d, ms per rank, from one more world with `LIG_TRACE` set (a drain of the stream after every phase: not "
                    "the run timed above; `[lig_trace] shard_explain_attached`; local rows per rank: %s):\n\n" % (a.asked[-1], res["w2_local_rows"]))
            f.write("| rank | select: mark, scan, collect, piece copies | exchange: header and record all-gathers, header merge | merge: keep, walk, order, "
                    "permute | records: fill, finish, copy back |\n|---|---|---|---|---|\n")
            for r, s in sorted(phases.items()):
                f.write("| %d | %.2f | %.2f | %.2f | %.2f |\n" % (r, s["select"], s["exchange"], s["merge"], s["records"]))
        f.write("\nThe \"exchange\" at W = 2 is a copy inside one device; on a node with one GPU per rank a rank receives 48 B x W x max m_r per call over "
                "the links plus the header blocks of 16 + 8 m bytes per rank (%d bytes at m = %d when one rank holds every asked term) -- a prediction, "
                "no such node was measured.\n" % (48 * 2 * a.asked[-1] + 2 * (16 + 8 * a.asked[-1]), a.asked[-1]))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
