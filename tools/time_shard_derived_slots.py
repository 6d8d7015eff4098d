#!/usr/bin/env python3
"""Derived slots on the sharded rows entry (lig_shard_rows_set_derived): what the list costs and saves there, and what the exchange costs.

The trace of tools/time_derived_slots.py: linear rows at the default bench geometry (l = 8000, k = 8192, n = 32768; 2098 rows = 2^24
constraints), every row with the profile of the recorded i32_add linear row -- 40 machine words recomposed from 32 or 33 bits of the SAME
row, so the list is row-local and issues no collective.  The library draws every pad and samples the dense randomness rows on the device.
World sizes in ONE command: W = 1 (one process, LIG_SHARD_FORCE_EXCHANGE: the exchange path of stage 1) and W = 2 (two processes on the
one GPU over comm_ipc: `shared_device`, functional only -- the ranks share the device's CUs and its host link).  Legs, alternating
(1a, 1b, 1x, 1p, 2a, 2b, 2x, 1a, ...), every rank a worker process that stays alive over the rounds:
    a   MIXED rows (a bit row + 40 records of 36 bytes) from pinned host memory, no list; the caller computed the words
    b   pure BIT rows (0 at the 40 word slots) + the derive list, from pinned host memory
    x   the exchange: bit rows + a SYNTHETIC list in which each of a row's 40 word slots copies one bit slot of a row of the NEXT rank
        (one wave, one all-gather).  Recorded: the derive bracket of one commit (export + all-gather + wave kernel, from
        lig_profile_read_launches(rows_in_launch = 0), a separate untimed commit) and exchange_bytes; ms per proof for completeness
    p   leg a at W = 1 on a build of the PARENT commit (--parent-root: a tree with ligero-prover_amd/ and its library), in a worker of its
        own: is the sharded stage 1 without a list what it was?
Timed per round: `steps` proofs of restart (the synchronous copy of the rank's rows) -> commit -> prove, after `warmup` proofs; ms per
proof = the slowest rank's.  Per leg: every round, median and spread (max - min), link bytes per trace summed over the ranks, the proof's
sha256 (a = b = p at both world sizes: the same rows).  Legs b / x also: lig_shard_rows_set_derived once per program (ms, host plan
included), its info, the derive bracket.

    python tools/time_shard_derived_slots.py [--rows 2098] [--reps 5] [--steps 4] [--parent-root DIR] [--write profiles/r23_shard_derived_slots.md]"""
import argparse
import ctypes as C
import hashlib
import importlib.util
import json
import os
import socket
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_derived_slots as tds                                       # the trace, its packing and its term list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_, K_, N_, WORDS = tds.L_, tds.K_, tds.N_, tds.WORDS


def load(root, name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "ligero-prover_amd", rel))
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def exchange_system(pkg, R, distinct, wcols, bcols, owner, world, l=L_):
    """every word slot of row r = the first bit slot of that word's list on a row of the NEXT rank (row r itself with one rank)"""
    held = [np.flatnonzero(owner == q) for q in range(world)]
    seen = [0] * world
    tb, slots, cidx, pairs = [0], [], [], []
    for r in range(R):
        q = (int(owner[r]) + 1) % world
        src = int(held[q][seen[q] % len(held[q])])
        seen[q] += 1
        d = r % distinct
        for i in range(WORDS):
            slots += [src * l + int(bcols[src % distinct, i, 0]), r * l + int(wcols[d, i])]
            cidx += [pkg.COEF_ONE, pkg.COEF_NEG_ONE]
            tb.append(len(slots))
            pairs.append((r * l + int(wcols[d, i]), len(tb) - 2))
    return pkg.LinearSystem.make(tb, slots, cidx), np.array(pairs, dtype=np.uint32)


class Worker:
    """one rank, one library: builds the trace once, then runs legs on request (a line of JSON in, a line of JSON out)"""

    def __init__(self, a):
        import torch
        self.torch, self.a = torch, a
        self.pkg = load(a.root, "ligero_prover_amd", "__init__.py")
        self.dist = load(a.root, "lig_dist", "dist.py")
        self.g = self.dist.Group("gloo")
        self.R = a.rows
        self.kinds = np.full(self.R, self.pkg.ROW_KINDS["LINEAR"] | self.pkg.ROW_DRAW_PAD, dtype=np.uint8)
        self.per_row = np.full(self.R, L_, dtype=np.uint32)
        self.data, self.wcols, self.bcols = tds.profile_rows(a.distinct, np.random.default_rng(13))
        self.ctx = self.pkg.Context(L_, K_, N_, device=a.device)
        self.comm = self.g.make_comm(self.pkg, self.ctx)
        rounds, b = self.pkg.shard_rows_plan(self.kinds, self.g.world)
        self.mine = np.array(self.pkg.local_rows_of(b, self.g.rank, self.g.world), dtype=np.int64)
        self.owner = np.zeros(self.R, dtype=np.int64)
        for g in range(len(b) - 1):
            self.owner[int(b[g]):int(b[g + 1])] = g % self.g.world
        self.systems, self.packed = {}, {}

    def fmt(self, name):
        """this rank's rows packed back to back -> (pinned tensor, widths of ALL rows, wide_per_row of ALL rows or None)"""
        if name not in self.packed:
            pkg, distinct = self.pkg, len(self.data)
            kinds = np.zeros(distinct, dtype=np.uint8)
            if name == "mixed":
                w, c = pkg.mixed_widths(self.data, kinds, L_)
                per = [pkg.pack_rows_mixed(self.data[d:d + 1], w[d:d + 1], c[d:d + 1], L_) for d in range(distinct)]
            else:
                blind = self.data.copy()
                for d in range(distinct):
                    blind[d, self.wcols[d]] = 0
                w, c = np.full(distinct, pkg.ELEM_BIT, dtype=np.uint8), None
                per = [pkg.pack_rows(blind[d:d + 1], w[d:d + 1], L_) for d in range(distinct)]
            idx = np.arange(self.R) % distinct
            local = np.concatenate([np.frombuffer(bytes(per[i]), dtype=np.uint8) for i in idx[self.mine]]) if len(self.mine) else np.zeros(0, dtype=np.uint8)
            assert len(local) == tds.expected_link_bytes(name, len(self.mine))
            keep = self.torch.empty(max(len(local), 1), dtype=self.torch.uint8, pin_memory=True)
            keep[:len(local)].copy_(self.torch.from_numpy(local))
            self.packed[name] = (keep, len(local), np.ascontiguousarray(w[idx]), None if c is None else np.ascontiguousarray(c[idx]))
        return self.packed[name]

    def system(self, which):
        if which not in self.systems:
            if which == "recompose":
                self.systems[which] = tds.derive_system(self.pkg, self.R, self.a.distinct, self.wcols, self.bcols)
            else:
                self.systems[which] = exchange_system(self.pkg, self.R, self.a.distinct, self.wcols, self.bcols, self.owner, self.g.world)
        return self.systems[which]

    def leg(self, fmt, derive):
        pkg, a, c = self.pkg, self.a, self.ctx
        keep, nbytes, widths, wide = self.fmt(fmt)
        ptr = C.c_void_p(keep.data_ptr())
        msgs = np.frombuffer((C.c_uint8 * max(nbytes, 1)).from_address(keep.data_ptr()), dtype=np.uint8)[:nbytes]      # a view of the pinned bytes
        sh = c.shard_rows_begin(self.kinds, msgs, self.g.rank, self.g.world, self.comm, dense_rands_per_row=self.per_row, elem_bytes=widths, wide_per_row=wide)
        set_ms, info = None, None
        if derive:
            sysb, pairs = self.system(derive)
            t0 = time.perf_counter()
            info = c.shard_rows_set_derived(sh, sysb, pairs).as_dict()
            set_ms = 1e3 * (time.perf_counter() - t0)
            assert info["n_waves"] == 1 and info["n_slots"] == self.R * WORDS

        def proofs(steps, first):
            out, flags = None, None
            for s in range(steps):
                if not (first and s == 0):
                    c.check(c.L.lig_shard_rows_restart(sh, ptr, 0))
                c.shard_rows_commit(sh)
                out, pi = c.shard_rows_prove(sh, None, None)
                flags = [pi.valid_code, pi.valid_linear, pi.valid_quad]
            return out, flags

        proofs(a.warmup, True)
        self.g.barrier()
        t0 = time.perf_counter()
        proof, flags = proofs(a.steps, False)
        dt = time.perf_counter() - t0
        bracket_ms = None
        if derive:                                                                   # untimed: one more commit + prove with the brackets on
            c.profile_enable(True)
            c.check(c.L.lig_shard_rows_restart(sh, ptr, 0))
            c.shard_rows_commit(sh)
            c.shard_rows_prove(sh, None, None)
            n, ms = C.c_uint64(), C.c_double()
            c.check(c.L.lig_profile_read_launches(c.h, 0, C.byref(n), C.byref(ms)))
            c.profile_enable(False)
            assert n.value == 1
            bracket_ms = ms.value
        c.shard_destroy(sh)
        return {"rank": self.g.rank, "ms_per_proof": 1e3 * dt / a.steps, "sha256": hashlib.sha256(bytes(proof)).hexdigest(), "link_bytes": nbytes, "valid": flags,
                "set_derived_ms": set_ms, "derive_bracket_ms": bracket_ms, "info": info}

    def serve(self):
        for line in sys.stdin:
            req = json.loads(line)
            if req.get("quit"):
                break
            print("RESULT " + json.dumps(self.leg(req["fmt"], req["derive"])), flush=True)
        self.ctx.close()
        self.g.close()


LEGS = {"a": ("mixed", None), "b": ("bits", "recompose"), "x": ("bits", "exchange"), "p": ("mixed", None)}
WHAT = {"a": "mixed rows, no list (as today)", "b": "bit rows + the row-local list", "x": "bit rows + the synthetic cross-rank list", "p": "leg a on a build of the parent commit"}


def free_port():
    s = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def write_profile(out, path):
    by = {e["leg"]: e for e in out["results"]}
    with open(path, "w") as f:
        f.write("# Derived slots on the sharded rows entry (`tools/time_shard_derived_slots.py`)\n\n")
        f.write("One MI355X, one command, alternating legs, %d rounds of %d proofs (restart + commit + prove); %d rows x %d slots, %d derived slots (%d per row) in one "
                "wave.  W = 1 runs the exchange path of stage 1 (`LIG_SHARD_FORCE_EXCHANGE`); W = 2 is two processes on the ONE device (`shared_device: true`): "
                "functional only, its times say nothing about a node with one GPU per rank.  Legs a, b, p prove the same rows: `same_proof` = %s.\n\n" % (
                    out["reps"], out["steps"], out["rows"], L_, out["derived_slots"], WORDS, out["same_proof"]))
        f.write("| leg | W | shared_device | what | median ms/proof | spread (max - min) | all rounds | link bytes per trace (all ranks) |\n|---|---|---|---|---|---|---|---|\n")
        for e in out["results"]:
            f.write("| %s | %d | %s | %s | %.2f | %.2f | %s | %d |\n" % (e["leg"], e["world"], "true" if e["shared_device"] else "false", e["what"], e["median_ms"], e["spread_ms"],
                                                                    ", ".join("%.2f" % x for x in e["ms_per_proof"]), e["link_bytes_per_trace"]))
        f.write("\n")
        for e in out["results"]:
            if e.get("set_derived_ms"):
                f.write("* leg %s: `lig_shard_rows_set_derived` once per program, per rank (host plan of the whole list, copies, table conversion) median %.1f ms; the derive "
                        "bracket of one commit (export + all-gather + wave kernel; `lig_profile_read_launches(rows_in_launch = 0)`, a separate untimed commit) median %.3f ms "
                        "(%s); n_exchanges %d, exchange_bytes %d per rank per commit.\n" % (
                            e["leg"], statistics.median(e["set_derived_ms"]), statistics.median(e["derive_bracket_ms"]), ", ".join("%.3f" % x for x in e["derive_bracket_ms"]),
                            e["info"]["n_exchanges"], e["info"]["exchange_bytes"]))
        f.write("\nMedian differences against the round spread of the two legs compared (the larger of the two):\n\n")
        for x, y, what in (("1p", "1a", "stage 1 without a list, parent build against this build"), ("1a", "1b", "the list, W = 1"), ("2a", "2b", "the list, W = 2 on the shared device")):
            if x in by and y in by:
                diff, spread = by[y]["median_ms"] - by[x]["median_ms"], max(by[x]["spread_ms"], by[y]["spread_ms"])
                f.write("* %s -> %s (%s): %+.2f ms, spread %.2f ms: %s\n" % (x, y, what, diff, spread, "within the spread" if abs(diff) <= spread else "BEYOND the spread"))
        f.write("\nOne GPU only.  What fewer link bytes and no host pass over the eval outputs are worth on a node with one GPU per rank, where every rank's rows cross "
                "its own link in the synchronous copy in front of stage 1, is a prediction, not measured here; so is the cost of the all-gather over xGMI "
                "(32 B x W x sum_w B(w) received per rank per commit).\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2098, help="linear rows of the trace (2098 x 8000 slots = 2^24 constraints)")
    ap.add_argument("--legs", default="1a,1b,1x,2a,2b,2x")
    ap.add_argument("--distinct", type=int, default=8, help="distinct rows of data, tiled over the trace")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent-root", default=None, help="a tree of the parent commit with its library built: leg 1p = leg 1a there")
    ap.add_argument("--write", default=None, help="write the profile (markdown) here")
    ap.add_argument("--json", default=None)
    ap.add_argument("--from-json", default=None, help="no run: write the profile of an earlier run's --json")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        Worker(a).serve()
        return 0
    if a.from_json:
        with open(a.from_json) as f:
            write_profile(json.load(f), a.write)
        return 0
    legs = a.legs.split(",") + (["1p"] if a.parent_root else [])
    legs.sort(key=lambda x: (x[0], "abxp".index(x[1])))

    def spawn(root, world, tag):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
        if world == 1:
            env["LIG_SHARD_FORCE_EXCHANGE"] = "1"
        else:
            env.update(LIG_COMM="ipc", LIG_COMM_TAG="tsds_%d_%s" % (os.getpid(), tag))
        return [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--root", os.path.abspath(root), "--rows", str(a.rows), "--distinct", str(a.distinct),
                                  "--steps", str(a.steps), "--warmup", str(a.warmup), "--device", str(a.device)],
                                 env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True) for r in range(world)]

    groups = {}
    for leg in legs:
        key = "p" if leg[1] == "p" else leg[0]
        if key not in groups:
            groups[key] = spawn(a.parent_root if key == "p" else ROOT, int(leg[0]), key)

    def ask(ws, leg):
        fmt, der = LEGS[leg[1]]
        for w in ws:
            w.stdin.write(json.dumps({"fmt": fmt, "derive": der}) + "\n")
            w.stdin.flush()
        got = []
        for w in ws:
            while True:
                line = w.stdout.readline()
                if not line:
                    raise SystemExit("a worker of leg %s ended (exit %s)" % (leg, w.poll()))
                if line.startswith("RESULT "):
                    got.append(json.loads(line[7:]))
                    break
        if len({r["sha256"] for r in got}) != 1:
            raise SystemExit("leg %s: the ranks' proofs differ" % leg)
        return got

    res = {leg: [] for leg in legs}
    try:
        for rep in range(a.reps):
            for leg in legs:                                                          # alternating
                got = ask(groups["p" if leg[1] == "p" else leg[0]], leg)
                res[leg].append(got)
                print("leg %s round %d  %7.2f ms/proof  %11d link bytes/trace  valid %s  sha256 %s%s" % (
                    leg, rep, max(r["ms_per_proof"] for r in got), sum(r["link_bytes"] for r in got), got[0]["valid"], got[0]["sha256"][:16],
                    "" if got[0]["derive_bracket_ms"] is None else "  set_derived %.1f ms, derive bracket %.3f ms, exchange_bytes %d" % (
                        max(r["set_derived_ms"] for r in got), max(r["derive_bracket_ms"] for r in got), got[0]["info"]["exchange_bytes"])), flush=True)
    finally:
        for ws in groups.values():
            for w in ws:
                try:
                    w.stdin.write(json.dumps({"quit": True}) + "\n")
                    w.stdin.flush()
                except Exception:
                    pass
            for w in ws:
                try:
                    w.wait(timeout=60)
                except Exception:
                    w.kill()
    same = {r["sha256"] for leg in legs if leg[1] in "abp" for got in res[leg] for r in got}
    out = {"tool": "time_shard_derived_slots", "rows": a.rows, "slots": a.rows * L_, "derived_slots": a.rows * WORDS, "steps": a.steps, "reps": a.reps,
           "same_proof": len(same) == 1, "results": []}
    for leg in legs:
        ms = [max(r["ms_per_proof"] for r in got) for got in res[leg]]
        world = int(leg[0])
        e = {"leg": leg, "world": world, "shared_device": world > 1, "what": WHAT[leg[1]], "ms_per_proof": ms, "median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms),
             "link_bytes_per_trace": sum(r["link_bytes"] for r in res[leg][0]), "valid": res[leg][0][0]["valid"]}
        if LEGS[leg[1]][1]:
            e["set_derived_ms"] = [max(r["set_derived_ms"] for r in got) for got in res[leg]]
            e["derive_bracket_ms"] = [max(r["derive_bracket_ms"] for r in got) for got in res[leg]]
            e["info"] = res[leg][0][0]["info"]
        out["results"].append(e)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if a.write:
        write_profile(out, a.write)
    return 0 if out["same_proof"] else 1


if __name__ == "__main__":
    sys.exit(main())
