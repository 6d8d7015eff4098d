#!/usr/bin/env python3
"""What lig_shard_rows_explain_slots_attached and lig_shard_rows_untouched_slots_attached cost, in ONE command on one box.  Records,
asserts nothing about speed.

Shape: the 2^24 single-term-constraint trace of tools/time_shard_explain_attached.py (k = 8192, l = 8000, linear rows; constraint c = slot
c, coefficient +1, one right-hand side each, w_s = b_s from a table of 251 values; the slots behind the last constraint are touched by
nothing), with 1 % of the witness slots changed after the right-hand sides were fixed.  The system is set on every shard with
lig_shard_rows_set_linear and attached to a one-GPU trace of the same rows.  Legs, ALTERNATING `--rounds` times (one warm-up round in
front):

  S<m>   lig_shard_rows_explain_slots_attached for the slots of the first m = 1 / 1024 / 65 536 violated constraints, every term reported
  E<m>   lig_shard_rows_explain_attached of those constraints (the call S<m> itself makes for the residuals)
  U0, U  lig_shard_rows_untouched_slots_attached: the counts only (cap 0), and with every record

  W = 1 with LIG_SHARD_FORCE_EXCHANGE set: the exchange path with one rank
  W = 2 as two PROCESSES on the ONE GPU over comm_ipc: `shared_device: true`, a functional run -- both ranks' kernels and the "exchange"
        share one device, the times say nothing about a node with one GPU per rank
  one   lig_rows_explain_slots_attached / lig_rows_untouched_slots_attached on the one-GPU trace, by rank 0 in the same run

Rank 0 of the two processes runs the W = 1 and one-GPU legs while rank 1 waits at a barrier; then both run the W = 2 legs.  The times are
the library's own wall time of the blocking call (ms_total of the info struct).  All worlds must return the same bytes (checked), and the
records are checked against the trace's construction.
--parent-root DIR: a tree of the parent commit with its library built; the E legs are timed once more there, in the same command, to
show that the existing call has not changed.
Writes a markdown file (default profiles/r21_shard_explain_slots.md) and prints one JSON line."""
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
import bench  # noqa: E402  (the shape; importing it runs nothing)


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
    free = R * l - n                                       # the slots behind the last constraint
    c = pkg.Context(l, k, n_enc, device=0)
    comm2 = g.make_comm(pkg, c)
    _, b = pkg.shard_rows_plan(kinds, g.world)
    mine = pkg.local_rows_of(b, g.rank, g.world)
    sh2 = c.shard_rows_begin(kinds, rows[mine], g.rank, g.world, comm2, generated_at=1)
    c.shard_rows_set_linear(sh2, system)
    c.shard_rows_commit(sh2)
    sh1 = comm1 = tr = keep = None
    if g.rank == 0:
        comm1 = c.ipc_comm("/lig_tses_%d" % os.getpid(), 0, 1)
        sh1 = c.shard_rows_begin(kinds, rows, 0, 1, comm1, generated_at=1)      # LIG_SHARD_FORCE_EXCHANGE is set: the exchange path
        c.shard_rows_set_linear(sh1, system)
        c.shard_rows_commit(sh1)
        if not a.only_e:
            tr, keep = c.rows_begin(kinds, rows, generated_at=1)
            c.rows_set_linear(tr, system)
            c.rows_commit(tr)
    cap = max(a.asked)
    rec_buf, terms_buf, vals_buf = np.zeros(cap, dtype=pkg.SLOT_RECORD), np.zeros(cap, dtype=pkg.SLOT_TERM), np.zeros(max(free, 1), dtype=pkg.SLOT_VALUE)
    con_buf = np.zeros(cap, dtype=pkg.EXPLAIN_CONSTRAINT)
    ptr = lambda arr: arr.ctypes.data_as(C.c_void_p)      # noqa: E731

    def slots_leg(where, asked):
        m = len(asked)
        info = pkg.SlotInfo()
        info.struct_bytes = C.sizeof(pkg.SlotInfo)
        if where == "one":
            c.check(c.L.lig_rows_explain_slots_attached(tr, ptr(asked), m, ptr(rec_buf), ptr(terms_buf), m, C.byref(info)))
        else:
            c.check(c.L.lig_shard_rows_explain_slots_attached(sh1 if where == 1 else sh2, ptr(asked), m, ptr(rec_buf), ptr(terms_buf), m, C.byref(info)))
        return info.ms_total, rec_buf[:m].tobytes() + terms_buf[:int(info.n_terms_reported)].tobytes() + str(int(info.n_constraints_distinct)).encode()

    def explain_leg(where, asked):
        m = len(asked)
        info = pkg.ExplainInfo()
        info.struct_bytes = C.sizeof(pkg.ExplainInfo)
        c.check(c.L.lig_shard_rows_explain_attached(sh1 if where == 1 else sh2, ptr(asked), m, ptr(con_buf), None, 0, C.byref(info)))
        return info.ms_total, con_buf[:m].tobytes()

    def untouched_leg(where, ucap):
        info = pkg.UntouchedInfo()
        info.struct_bytes = C.sizeof(pkg.UntouchedInfo)
        if where == "one":
            c.check(c.L.lig_rows_untouched_slots_attached(tr, 0, ptr(vals_buf) if ucap else None, ucap, C.byref(info)))
        else:
            c.check(c.L.lig_shard_rows_untouched_slots_attached(sh1 if where == 1 else sh2, 0, ptr(vals_buf) if ucap else None, ucap, C.byref(info)))
        return info.ms_total, vals_buf[:int(info.n_reported)].tobytes() + str((int(info.n_untouched), int(info.n_untouched_nonzero), int(info.n_reported))).encode()

    def slots_as_built(asked, raw):
        """one +1 term per slot, in the constraint of the same number, the changed value, residual 1000"""
        m = len(asked)
        rec = np.frombuffer(raw[:m * pkg.SLOT_RECORD.itemsize], dtype=pkg.SLOT_RECORD)
        terms = np.frombuffer(raw[m * pkg.SLOT_RECORD.itemsize:m * pkg.SLOT_RECORD.itemsize + m * pkg.SLOT_TERM.itemsize], dtype=pkg.SLOT_TERM)
        w, one, res = (np.zeros((m, 8), dtype=np.uint32) for _ in range(3))
        w[:, 0], one[:, 0], res[:, 0] = asked % 251 + 1001, 1, 1000
        return ((rec["slot"] == asked).all() and (rec["n_terms"] == 1).all() and (rec["first_term"] == np.arange(m)).all() and rec["value"].tobytes() == w.tobytes() and
                (terms["slot"] == asked).all() and (terms["constraint"] == asked).all() and (terms["constraint_terms"] == 1).all() and
                terms["coef"].tobytes() == one.tobytes() and terms["residual"].tobytes() == res.tobytes())

    def untouched_as_built(raw, ucap):
        rep = min(free, ucap)
        vals = np.frombuffer(raw[:rep * pkg.SLOT_VALUE.itemsize], dtype=pkg.SLOT_VALUE)
        return raw[rep * pkg.SLOT_VALUE.itemsize:] == str((free, free, rep)).encode() and (vals["slot"] == np.arange(n, n + rep)).all()

    names = ["E%d" % m for m in a.asked] if a.only_e else ["S%d" % m for m in a.asked] + ["E%d" % m for m in a.asked] + ["U0", "U"]
    worlds = [1, 2] if a.only_e else [1, 2, "one"]
    legs = {"%s_%s" % (nm, w): [] for nm in names for w in worlds if not (w == "one" and nm[0] == "E")}
    same = True

    def run(nm, where):
        if nm[0] == "S":
            asked = np.ascontiguousarray(changed[:int(nm[1:])])
            ms, raw = slots_leg(where, asked)
            return ms, raw, bool(slots_as_built(asked, raw))
        if nm[0] == "E":
            ms, raw = explain_leg(where, np.ascontiguousarray(changed[:int(nm[1:])]))
            return ms, raw, True
        ucap = 0 if nm == "U0" else free
        ms, raw = untouched_leg(where, ucap)
        return ms, raw, bool(untouched_as_built(raw, ucap))

    for rnd in range(a.rounds + 1):
        raws = {nm: [] for nm in names}
        if g.rank == 0:
            for nm in names:
                for where in (1, "one"):
                    if "%s_%s" % (nm, where) not in legs:
                        continue
                    ms, raw, ok = run(nm, where)
                    same = same and ok
                    raws[nm].append(raw)
                    if rnd:
                        legs["%s_%s" % (nm, where)].append(ms)
        g.barrier()
        for nm in names:
            ms, raw, ok = run(nm, 2)
            same = same and ok
            raws[nm].append(raw)
            if rnd:
                legs["%s_2" % nm].append(ms)
            g.barrier()
        same = same and all(len(set(v)) == 1 for v in raws.values())
    c.shard_destroy(sh2)
    if g.rank == 0:
        if tr is not None:
            c.trace_destroy(tr)
        c.shard_destroy(sh1)
        c.ipc_comm_destroy(comm1)
    print(json.dumps({"rank": g.rank, "legs": legs, "same_output": bool(same), "local_rows": len(mine), "changed": int(len(changed)), "untouched": int(free)}), flush=True)
    c.close()
    g.close()
    return 0 if same else 1


def free_port():
    s = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def run_world(a, tag, pkg_root, only_e=False):
    """two rank processes of this file as workers -> [rank 0's JSON, rank 1's JSON]"""
    world = 2
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "LIG_TRACE")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0", LIG_COMM="ipc",
               LIG_COMM_TAG="tses%s%d" % (tag, os.getpid()), LIG_SHARD_FORCE_EXCHANGE="1")
    argv = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--pkg-root", pkg_root, "--log2-constraints",
            str(a.log2_constraints), "--rounds", str(a.rounds), "--asked"] + [str(m) for m in a.asked] + (["--only-e"] if only_e else [])
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
    return sorted((json.loads([ln for ln in o.splitlines() if ln.startswith("{")][-1]) for o, _ in outs), key=lambda d: d["rank"])


def merged(ranks):
    """W = 1 and one GPU: rank 0's times; W = 2: the slower rank of every round"""
    legs = {}
    for key, v in ranks[0]["legs"].items():
        legs[key] = [max(x) for x in zip(*(r["legs"][key] for r in ranks))] if key.endswith("_2") else v
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-constraints", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--asked", type=int, nargs=3, default=[1, 1024, 65536])
    ap.add_argument("--timeout", type=int, default=420, help="seconds per rank (timeout -k 10)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_shard_explain_slots.md"))
    ap.add_argument("--parent-root", default=None, help="a tree of the parent commit with its library built: the E legs once more there")
    ap.add_argument("--pkg-root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--only-e", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    ranks = run_world(a, "n", ROOT)
    legs = merged(ranks)
    ok = all(r["same_output"] for r in ranks)
    parent = None
    if a.parent_root:
        pranks = run_world(a, "p", os.path.abspath(a.parent_root), only_e=True)
        parent = merged(pranks)
        ok = ok and all(r["same_output"] for r in pranks)
    med = {key: statistics.median(v) for key, v in legs.items()}
    spread = {key: max(v) - min(v) for key, v in legs.items()}
    pmed = {key: statistics.median(v) for key, v in parent.items()} if parent else None
    n = 1 << a.log2_constraints
    res = {"constraints": n, "rounds": a.rounds, "asked": a.asked, "changed_slots": ranks[0]["changed"], "untouched_slots": ranks[0]["untouched"], "ms": legs,
           "median_ms": med, "spread_ms": spread, "parent_ms": parent, "parent_median_ms": pmed, "shared_device": True,
           "w2_local_rows": [r["local_rows"] for r in ranks], "same_output_in_all_legs": ok}
    print(json.dumps(res))
    fmt = lambda v: ", ".join("%.2f" % x for x in v)      # noqa: E731
    where = {"1": "W = 1, `LIG_SHARD_FORCE_EXCHANGE=1` (the exchange path with one rank)",
             "2": "W = 2 as two processes on the ONE GPU (`shared_device: true`, functional only; the slower rank)",
             "one": "one GPU: `lig_rows_explain_slots_attached` / `lig_rows_untouched_slots_attached` on a trace of the same rows"}
    what = {"S": "`lig_shard_rows_explain_slots_attached`, the slots of the first %s violated constraints", "E": "`lig_shard_rows_explain_attached` of those %s constraints",
            "U0": "`lig_shard_rows_untouched_slots_attached`, counts only", "U": "`lig_shard_rows_untouched_slots_attached`, every record"}
    with open(a.out, "w") as f:
        f.write("# lig_shard_rows_explain_slots_attached and lig_shard_rows_untouched_slots_attached (tools/time_shard_explain_slots.py)\n\n")
        f.write("Trace: %d single-term constraints w_s = b_s over linear rows at l = %d, k = %d, %d slots (1 %%) changed, %d slots behind the last "
                "constraint touched by nothing; the system set on every shard with `lig_shard_rows_set_linear` and attached to a one-GPU trace of the "
                "same rows.  The same bytes in every world (%s), checked against the trace's construction.  %d rounds after one warm-up round, the "
                "legs alternating inside every round; times in ms: the library's own wall time of the blocking call (`ms_total`), output arrays kept "
                "between calls.  Nothing is asserted about speed.\n\n" % (n, bench.L_, bench.K_, res["changed_slots"], res["untouched_slots"],
                                                                          "checked: yes" if ok else "CHECK FAILED", a.rounds))
        f.write("| leg | world | median ms | spread (max - min) | all rounds, ms |\n|---|---|---|---|---|\n")
        for key in legs:
            nm, w = key.rsplit("_", 1)
            text = what[nm] if nm in what else what[nm[0]] % nm[1:]
            f.write("| %s | %s | %.2f | %.2f | %s |\n" % (text, where[w], med[key], spread[key], fmt(legs[key])))
        if parent:
            f.write("\n`lig_shard_rows_explain_attached` (constraint records only) once more on a build of the parent commit, same command, same shards, in a "
                    "world of its own started after the first -- the two columns are not alternating legs, and the difference between them is what two worlds "
                    "of the same code differ by:\n\n")
            f.write("| m | world | here, median ms | on the parent, median ms | parent, all rounds |\n|---|---|---|---|---|\n")
            for m in a.asked:
                for w in ("1", "2"):
                    key = "E%d_%s" % (m, w)
                    f.write("| %d | W = %s | %.2f | %.2f | %s |\n" % (m, w, med[key], pmed[key], fmt(parent[key])))
        else:
            f.write("\n`lig_shard_rows_explain_attached` was not timed on a build of the parent commit in this run (`--parent-root`).\n")
        f.write("\nThe \"exchange\" at W = 2 is a copy inside one device; on a node with one GPU per rank a rank receives 16 B x W x max m_r per call over the "
                "links plus the header blocks of 16 + 48 m bytes per rank and the exchange of the inner `lig_shard_rows_explain_attached` -- a prediction, no "
                "such node was measured.\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
