#!/usr/bin/env python3
"""Derived slots (lig_rows_set_derived): what forming the eval outputs of a bit row on the device costs, and what it saves.

A trace of linear rows at the default bench geometry (l = 8000, k = 8192, n = 32768; 2098 rows = 2^24 constraints), every row with the
profile of the recorded i32_add linear row: 40 of its 8000 data slots are machine words among bits.  Here every word IS what i32_add's
eval makes it: the recomposition sum_j 2^j * bit_j of 32 (36 words) or 33 (4 words) bit slots of the same row, so one term list serves
both formats and every leg proves the same rows.  The library draws every pad and samples the dense randomness rows on the device.
Legs, alternating in ONE command (a, b, c, d, p, a, b, ...), each in a worker process that stays alive over the rounds:
    a   MIXED rows (a bit row + 40 records of 36 bytes) from pinned host memory, as today; the caller computed the words
    b   pure BIT rows (0 at the 40 word slots) + the derive list, from pinned host memory: stage 1 queues every chunk's arrival, expansion
        and pads, then the wave, then the encodes -- the upload / encode overlap is given up
    c   as a, rows resident on the device          d   as b, rows resident on the device: c -> d isolates the kernels' cost
    p   leg a on a build of the PARENT commit (--parent-root: a tree with ligero-prover_amd/__init__.py and its library), in a worker of
        its own: is stage 1 without a list what it was?
The upload of every trace is inside the timed region (commit -> restart of the next trace -> prove, --inflight proofs in flight on as
many contexts, as tools/time_mixed_rows.py).  Per leg: ms per proof of every round, median and spread, bytes over the link per trace,
the proof's sha256 (equal across all legs).  Legs b / d also: lig_rows_set_derived once per program (ms, with the host plan), and the
time of the derive launches per commit from lig_profile_read_launches(rows_in_launch = 0), taken in a separate untimed pass.

    python tools/time_derived_slots.py [--rows 2098] [--reps 5] [--steps 4] [--parent-root DIR] [--write profiles/r22_derived_slots.md]"""
import argparse
import ctypes as C
import hashlib
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_, K_, N_ = 8000, 8192, 32768
WORDS32, WORDS33 = 36, 4                   # per row: words recomposed from 32 bits, from 33 bits (the 4-byte and 8-byte words of i32_add)
WORDS = WORDS32 + WORDS33


def load_pkg(root):
    spec = importlib.util.spec_from_file_location("ligero_prover_amd", os.path.join(root, "ligero-prover_amd", "__init__.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["ligero_prover_amd"] = m
    spec.loader.exec_module(m)
    return m


def profile_rows(distinct, rng, l=L_, k=K_):
    """-> (rows (distinct, k, 8) uint32 with the words filled in, word columns (distinct, WORDS), bit columns (distinct, WORDS, 33))"""
    rows = np.zeros((distinct, k, 8), dtype=np.uint32)
    rows[:, :l, 0] = rng.integers(0, 2, (distinct, l))
    wcols = np.zeros((distinct, WORDS), dtype=np.int64)
    bcols = np.zeros((distinct, WORDS, 33), dtype=np.int64)
    for d in range(distinct):
        perm = rng.permutation(l)
        wcols[d] = np.sort(perm[:WORDS])
        pool = perm[WORDS:]
        for i in range(WORDS):
            bcols[d, i] = rng.choice(pool, 33, replace=False)
            rows[d, bcols[d, i, 32 if i >= WORDS32 else 16], 0] = 1      # never narrower than its class: 17..32 bits | 33 bits
        for i in range(WORDS):                                          # (bit slots may serve several words: values after every forced bit)
            nb = 32 if i < WORDS32 else 33
            v = sum(int(rows[d, bcols[d, i, j], 0]) << j for j in range(nb))
            rows[d, wcols[d, i], 0], rows[d, wcols[d, i], 1] = v & 0xFFFFFFFF, v >> 32
    return rows, wcols, bcols


def derive_system(pkg, R, distinct, wcols, bcols, l=L_):
    """the defining constraints of the whole trace: sum_j 2^j * bit_j - word = 0, one per word slot -> (LinearSystem, pairs (n, 2))"""
    tb, slots, cidx, pairs = [0], [], [], []
    for r in range(R):
        d = r % distinct
        for i in range(WORDS):
            nb = 32 if i < WORDS32 else 33
            slots.extend((r * l + bcols[d, i, :nb]).tolist())
            cidx.extend(range(nb))
            slots.append(r * l + int(wcols[d, i]))
            cidx.append(pkg.COEF_NEG_ONE)
            tb.append(len(slots))
            pairs.append((r * l + int(wcols[d, i]), len(tb) - 2))
    return pkg.LinearSystem.make(tb, slots, cidx, coefs=[1 << j for j in range(33)]), np.array(pairs, dtype=np.uint32)


def pack_trace(pkg, fmt, R, data, wcols, l=L_):
    """-> (packed bytes, widths, wide_per_row or None); fmt "mixed": bits + records, "bits": the word slots zeroed, pure bit rows"""
    distinct = len(data)
    kinds = np.zeros(distinct, dtype=np.uint8)
    if fmt == "mixed":
        w, c = pkg.mixed_widths(data, kinds, l)
        per = [pkg.pack_rows_mixed(data[d:d + 1], w[d:d + 1], c[d:d + 1], l) for d in range(distinct)]
    else:
        blind = data.copy()
        for d in range(distinct):
            blind[d, wcols[d]] = 0
        w, c = np.full(distinct, pkg.ELEM_BIT, dtype=np.uint8), None
        per = [pkg.pack_rows(blind[d:d + 1], w[d:d + 1], l) for d in range(distinct)]
    idx = np.arange(R) % distinct
    return np.concatenate([per[i] for i in idx]), np.ascontiguousarray(w[idx]), None if c is None else np.ascontiguousarray(c[idx])


def expected_link_bytes(fmt, rows, l=L_):
    return rows * ((l + 31) // 32 * 4 + (36 * WORDS if fmt == "mixed" else 0))


class Worker:
    """one process, one library: builds the trace once, then runs legs on request (a line of JSON in, a line of JSON out)"""

    def __init__(self, a):
        import torch
        self.torch, self.a = torch, a
        self.pkg = load_pkg(a.root)
        self.R = a.rows
        self.kinds = np.full(self.R, self.pkg.ROW_KINDS["LINEAR"] | self.pkg.ROW_DRAW_PAD, dtype=np.uint8)
        self.per_row = np.full(self.R, L_, dtype=np.uint32)
        self.data, self.wcols, self.bcols = profile_rows(a.distinct, np.random.default_rng(13))
        self.ctxs = [self.pkg.Context(L_, K_, N_, device=a.device) for _ in range(a.inflight)]
        self.packed, self.system = {}, None

    def fmt(self, name):
        if name not in self.packed:
            p = pack_trace(self.pkg, name, self.R, self.data, self.wcols)
            assert len(p[0]) == expected_link_bytes(name, self.R)
            self.packed[name] = p
        return self.packed[name]

    def leg(self, fmt, on_device, derive):
        pkg, torch, a, ctxs = self.pkg, self.torch, self.a, self.ctxs
        packed, widths, wide = self.fmt(fmt)
        if derive and self.system is None:
            self.system = derive_system(pkg, self.R, a.distinct, self.wcols, self.bcols)
        if on_device:
            keep = torch.from_numpy(packed).to("cuda:%d" % a.device)
        else:
            keep = torch.empty(len(packed), dtype=torch.uint8, pin_memory=True)
            keep.copy_(torch.from_numpy(packed))
        ptr, dev = keep.data_ptr(), int(bool(on_device))
        traces, set_ms = [], []
        for c in ctxs:
            job = pkg.RowsJob()
            job.rows, job.kinds, job.msgs, job.msgs_on_device = self.R, self.kinds.ctypes.data, ptr, dev
            for i in range(32):
                job.encoding_seed[i] = i
                job.program_hash[i] = 0
            job.version = b"1.5.0"
            job.set_public_args(None)
            job.dense_rands_per_row = self.per_row.ctypes.data
            job.elem_bytes = widths.ctypes.data
            if wide is not None:
                job.wide_per_row = wide.ctypes.data
                job.reserved = pkg.ROWS_JOB_WIDE
            t = C.c_void_p()
            c.check(c.L.lig_rows_begin(c.h, C.byref(job), C.byref(t)))
            if derive:
                t0 = time.perf_counter()
                info = c.rows_set_derived(t, self.system[0], self.system[1])
                set_ms.append(1e3 * (time.perf_counter() - t0))
                assert info.n_waves == 1 and info.n_slots == self.R * WORDS
            traces.append([t, True])

        def loop(i, steps, last):
            c, t = ctxs[i], traces[i][0]
            out = None
            for s in range(steps):
                if not traces[i][1]:
                    c.check(c.L.lig_rows_restart(t, C.c_void_p(ptr), dev))
                c.rows_commit(t)
                traces[i][1] = s + 1 < steps or not last
                if traces[i][1]:                                                     # the next trace goes up under this proof
                    c.check(c.L.lig_rows_restart(t, C.c_void_p(ptr), dev))
                out, info = c.rows_prove(t, None, None, copy=False)
                if not (info.valid_code and info.valid_linear and info.valid_quad):
                    raise SystemExit("prover self-check failed")
            return C.string_at(*out)

        with ThreadPoolExecutor(max_workers=a.inflight) as pool:
            list(pool.map(lambda i: loop(i, a.warmup, False), range(a.inflight)))
            t0 = time.perf_counter()
            proofs = list(pool.map(lambda i: loop(i, a.steps, True), range(a.inflight)))
            dt = time.perf_counter() - t0
        derive_ms = None
        if derive:                                                                   # untimed: one more commit + prove with the brackets on
            c, t = ctxs[0], traces[0][0]
            c.profile_enable(True)
            c.check(c.L.lig_rows_restart(t, C.c_void_p(ptr), dev))
            c.rows_commit(t)
            c.rows_prove(t, None, None, copy=False)
            n, ms = C.c_uint64(), C.c_double()
            c.check(c.L.lig_profile_read_launches(c.h, 0, C.byref(n), C.byref(ms)))
            c.profile_enable(False)
            assert n.value == 1
            derive_ms = ms.value
        for c, (t, _) in zip(ctxs, traces):
            c.trace_destroy(t)
        del keep
        if len(set(proofs)) != 1:
            raise SystemExit("the proofs in flight differ")
        return {"ms_per_proof": 1e3 * dt / (a.inflight * a.steps), "sha256": hashlib.sha256(proofs[0]).hexdigest(), "link_bytes": 0 if on_device else len(packed),
                "set_derived_ms": statistics.median(set_ms) if set_ms else None, "derive_launch_ms": derive_ms}

    def serve(self):
        for line in sys.stdin:
            req = json.loads(line)
            if req.get("quit"):
                break
            print("RESULT " + json.dumps(self.leg(req["fmt"], req["on_device"], req["derive"])), flush=True)
        for c in self.ctxs:
            c.close()


def write_profile(out, path):
    by = {e["leg"]: e for e in out["results"]}
    with open(path, "w") as f:
        f.write("# Derived slots: the 40 eval outputs of a bit row formed on the device (`tools/time_derived_slots.py`)\n\n")
        f.write("One MI355X, one command, alternating legs, %d rounds of %d proofs x %d in flight; %d rows x %d slots, %d derived slots (%d per row, each "
                "with 32 or 33 other terms) in one wave.  Every leg proves the same rows: `same_proof_across_legs` = %s.\n\n" % (
                    out["reps"], out["steps"], out["inflight"], out["rows"], L_, out["derived_slots"], WORDS, out["same_proof_across_legs"]))
        f.write("| leg | what | median ms/proof | spread (max - min) | all rounds | link bytes per trace |\n|---|---|---|---|---|---|\n")
        for e in out["results"]:
            f.write("| %s | %s | %.2f | %.2f | %s | %d |\n" % (e["leg"], e["what"], e["median_ms"], e["spread_ms"], ", ".join("%.2f" % x for x in e["ms_per_proof"]), e["link_bytes_per_trace"]))
        for e in out["results"]:
            if "set_derived_ms" in e:
                f.write("\nLeg %s: `lig_rows_set_derived` once per program (host plan, copies, table conversion) median %.1f ms (%s); the derive launches of one commit "
                        "(`lig_profile_read_launches(rows_in_launch = 0)`, a separate untimed commit) median %.3f ms (%s).\n" % (
                            e["leg"], statistics.median(e["set_derived_ms"]), ", ".join("%.1f" % x for x in e["set_derived_ms"]),
                            statistics.median(e["derive_launch_ms"]), ", ".join("%.3f" % x for x in e["derive_launch_ms"])))
        f.write("\nMedian differences against the round spread of the two legs compared (the larger of the two):\n\n")
        for x, y, what in (("a", "b", "the list and the lost upload / encode overlap, host rows"), ("c", "d", "the derive kernels alone, device rows"),
                           ("p", "a", "stage 1 without a list, parent build against this build")):
            if x in by and y in by:
                diff, spread = by[y]["median_ms"] - by[x]["median_ms"], max(by[x]["spread_ms"], by[y]["spread_ms"])
                f.write("* %s -> %s (%s): %+.2f ms, spread %.2f ms: %s\n" % (x, y, what, diff, spread, "within the spread" if abs(diff) <= spread else "BEYOND the spread"))
        f.write("\nOne GPU only.  What fewer link bytes are worth on a node whose GPUs share the host link is a prediction, not measured here.\n")


LEGS = {"a": ("mixed", False, False), "b": ("bits", False, True), "c": ("mixed", True, False), "d": ("bits", True, True), "p": ("mixed", False, False)}
WHAT = {"a": "mixed rows, pinned host memory (as today)", "b": "bit rows + derive list, pinned host memory", "c": "mixed rows, device rows",
        "d": "bit rows + derive list, device rows", "p": "leg a on a build of the parent commit"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2098, help="linear rows of the trace (2098 x 8000 slots = 2^24 constraints)")
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--distinct", type=int, default=8, help="distinct rows of data, tiled over the trace")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent-root", default=None, help="a tree of the parent commit with its library built: leg p = leg a there")
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
    legs = a.legs.split(",") + (["p"] if a.parent_root else [])

    def spawn(root):
        return subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--root", os.path.abspath(root), "--rows", str(a.rows), "--distinct", str(a.distinct),
                                 "--steps", str(a.steps), "--warmup", str(a.warmup), "--inflight", str(a.inflight), "--device", str(a.device)],
                                stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    here, parent = spawn(ROOT), spawn(a.parent_root) if a.parent_root else None

    def ask(w, leg):
        fmt, dev, der = LEGS[leg]
        w.stdin.write(json.dumps({"fmt": fmt, "on_device": dev, "derive": der}) + "\n")
        w.stdin.flush()
        while True:
            line = w.stdout.readline()
            if not line:
                raise SystemExit("worker of leg %s ended (exit %s)" % (leg, w.poll()))
            if line.startswith("RESULT "):
                return json.loads(line[7:])

    res = {leg: [] for leg in legs}
    try:
        for rep in range(a.reps):
            for leg in legs:                                                          # alternating
                r = ask(parent if leg == "p" else here, leg)
                res[leg].append(r)
                print("leg %s round %d  %7.2f ms/proof  %11d link bytes/trace  sha256 %s%s" % (
                    leg, rep, r["ms_per_proof"], r["link_bytes"], r["sha256"][:16],
                    "" if r["derive_launch_ms"] is None else "  set_derived %.1f ms, derive launches %.3f ms" % (r["set_derived_ms"], r["derive_launch_ms"])), flush=True)
    finally:
        for w in (here, parent):
            if w:
                try:
                    w.stdin.write(json.dumps({"quit": True}) + "\n")
                    w.stdin.flush()
                    w.wait(timeout=60)
                except Exception:
                    w.kill()
    out = {"tool": "time_derived_slots", "rows": a.rows, "slots": a.rows * L_, "derived_slots": a.rows * WORDS, "inflight": a.inflight, "steps": a.steps, "reps": a.reps,
           "same_proof_across_legs": len({r["sha256"] for v in res.values() for r in v}) == 1, "results": []}
    for leg in legs:
        ms = [r["ms_per_proof"] for r in res[leg]]
        e = {"leg": leg, "what": WHAT[leg], "ms_per_proof": ms, "median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "link_bytes_per_trace": res[leg][0]["link_bytes"]}
        if LEGS[leg][2]:
            e["set_derived_ms"] = [r["set_derived_ms"] for r in res[leg]]
            e["derive_launch_ms"] = [r["derive_launch_ms"] for r in res[leg]]
        out["results"].append(e)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if a.write:
        write_profile(out, a.write)
    return 0 if out["same_proof_across_legs"] else 1


if __name__ == "__main__":
    sys.exit(main())
