#!/usr/bin/env python3
"""Product entries of derived slots (LIG_DERIVED_PRODUCT): what re-forming the products of eval outputs on the device costs and saves.

A trace at the default bench geometry (l = 8000, k = 8192, n = 32768) of 1049 blocks of four rows LINEAR, QX, QY, QZ = 2^24 constraints,
half of them quadratic.  The guest, in every column i of every block:  x_i = eval(3 y_i + 5);  z_i = x_i * y_i;  v_i = eval(z_i + y_i)
with y_i < 2^61 on the QY row, x on the QX row, z on the QZ row and v on the LINEAR row -- linear, product, linear: three waves.  x fits
8 bytes; z and v have up to 125 bits and fit no narrow width.  Every leg proves the same rows; the library draws every pad and samples
the dense randomness rows on the device.  Legs, alternating in ONE command, each in a worker process that stays alive over the rounds:
    a   nothing derived: v and z rows at full width, x and y rows 8 bytes wide, no list
    b   only y shipped (8 bytes): x and v rows all-zero bit rows, z rows LIG_ELEM_PRODUCT; the list {x, its constraint}, {z, PRODUCT},
        {v, its constraint} for every column
    d   a list WITHOUT product entries: as leg a, but the v rows all-zero bit rows and {v, its constraint} listed (z is shipped)
    c   leg a, and e: leg d, on a build of the PARENT commit (--parent-root: a tree with ligero-prover_amd/__init__.py and its library)
The upload of every trace is inside the timed region (commit -> restart of the next trace -> prove, --inflight proofs in flight on as
many contexts, as tools/time_derived_slots.py).  Per leg: ms per proof of every round, median and spread, bytes over the link per trace,
the proof's sha256 (equal across all legs).  Legs with a list also: lig_rows_set_derived once per program (ms, with the host plan), and
the derive bracket per commit from lig_profile_read_launches(rows_in_launch = 0), taken in a separate untimed pass.

    python tools/time_derived_products.py [--blocks 1049] [--reps 5] [--steps 4] [--parent-root DIR] [--write profiles/r24_derived_products.md]"""
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
PRODUCT = 0xFFFFFFFF                       # LIG_DERIVED_PRODUCT (named here: the parent's package has no such constant)
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617      # the BN254 scalar field


def load_pkg(root):
    spec = importlib.util.spec_from_file_location("ligero_prover_amd", os.path.join(root, "ligero-prover_amd", "__init__.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["ligero_prover_amd"] = m
    spec.loader.exec_module(m)
    return m


def limbs_of(values, k=K_):
    """Python integers (l of them) -> one row (k, 8) uint32, data slots filled, pads zero"""
    row = np.zeros((k, 8), dtype=np.uint32)
    row[:len(values)] = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint32).reshape(-1, 8)
    return row


def block_rows(distinct, rng, l=L_):
    """-> (distinct, 4, k, 8) uint32: the rows v, x, y, z of `distinct` blocks in integers"""
    out = np.zeros((distinct, 4, K_, 8), dtype=np.uint32)
    for d in range(distinct):
        y = [int(v) for v in rng.integers(0, 1 << 61, l, dtype=np.uint64)]
        x = [3 * v + 5 for v in y]
        z = [a * b for a, b in zip(x, y)]
        v = [a + b for a, b in zip(z, y)]
        for i, vals in enumerate((v, x, y, z)):
            out[d, i] = limbs_of(vals)
    return out


def derive_system(pkg, blocks, with_x, l=L_):
    """constraints 2j (x = 3 y + 5, only with_x) and 2j + 1 (v = z + y) of every column j of the trace -> (LinearSystem, n_constraints)"""
    col = np.arange(l, dtype=np.int64)
    parts_s, parts_c = [], []
    for b in range(blocks):
        v, x, y, z = ((4 * b + i) * l + col for i in range(4))
        if with_x:
            s = np.stack([y, x, z, y, v], axis=1)
            c = np.tile(np.array([0, pkg.COEF_NEG_ONE, pkg.COEF_ONE, pkg.COEF_ONE, pkg.COEF_NEG_ONE], dtype=np.int64), (l, 1))
        else:
            s = np.stack([z, y, v], axis=1)
            c = np.tile(np.array([pkg.COEF_ONE, pkg.COEF_ONE, pkg.COEF_NEG_ONE], dtype=np.int64), (l, 1))
        parts_s.append(s.reshape(-1))
        parts_c.append(c.reshape(-1))
    slots, cidx = np.concatenate(parts_s), np.concatenate(parts_c)
    n = blocks * l
    if with_x:                                             # per column: 2 terms (constraint 2j), 3 terms (2j + 1); 3 y - x = -5
        tb = np.zeros(2 * n + 1, dtype=np.int64)
        tb[1::2], tb[2::2] = 2, 3
        tb = np.cumsum(tb)
        rhs_c, rhs_b = np.arange(0, 2 * n, 2), np.full(n, 1)
        return pkg.LinearSystem.make(tb, slots, cidx, rhs_c, rhs_b, coefs=[3, P - 5]), 2 * n
    return pkg.LinearSystem.make(np.arange(0, 3 * n + 1, 3), slots, cidx), n


def derive_list(blocks, with_products, l=L_):
    """-> (n, 2) uint32 pairs.  with_products: {x, 2j}, {z, PRODUCT}, {v, 2j + 1} per column j; else {v, j}"""
    col = np.arange(l, dtype=np.int64)
    out = []
    for b in range(blocks):
        v, x, z = (4 * b + 0) * l + col, (4 * b + 1) * l + col, (4 * b + 3) * l + col
        j = b * l + col
        if with_products:
            out += [np.stack([x, 2 * j], axis=1), np.stack([z, np.full(l, PRODUCT)], axis=1), np.stack([v, 2 * j + 1], axis=1)]
        else:
            out.append(np.stack([v, j], axis=1))
    return np.ascontiguousarray(np.concatenate(out), dtype=np.uint32)


FORMATS = {"full": (32, 8, 8, 32), "v_derived": ("bit", 8, 8, 32), "all_derived": ("bit", "bit", 8, "product")}


def pack_trace(pkg, fmt, blocks, data, l=L_):
    """-> (packed bytes, widths): rows listed as bit rows are shipped as zeros"""
    names = {"bit": pkg.ELEM_BIT, "product": pkg.ELEM_PRODUCT}
    w4 = np.array([names.get(w, w) for w in FORMATS[fmt]], dtype=np.uint8)
    per = []
    for d in range(len(data)):
        rows = data[d].copy()
        for i, w in enumerate(FORMATS[fmt]):
            if w == "bit":
                rows[i] = 0
        per.append(pkg.pack_rows(rows, w4, l))
    idx = np.arange(blocks) % len(data)
    return np.concatenate([per[i] for i in idx]), np.ascontiguousarray(np.tile(w4, blocks))


def expected_link_bytes(fmt, blocks, l=L_):
    one = {32: K_ * 32, 8: 8 * l, "bit": (l + 31) // 32 * 4, "product": 0}
    return blocks * sum(one[w] for w in FORMATS[fmt])


# leg -> (row format, list: None / "linear" / "products")
LEGS = {"a": ("full", None), "b": ("all_derived", "products"), "d": ("v_derived", "linear"), "c": ("full", None), "e": ("v_derived", "linear")}
WHAT = {"a": "nothing derived: z and v rows full width, no list", "b": "only y shipped; x, z = x*y, v formed on the device (3 waves)",
        "d": "a list without product entries: v derived, z shipped", "c": "leg a on a build of the parent commit", "e": "leg d on a build of the parent commit"}
ON_PARENT = ("c", "e")


class Worker:
    """one process, one library: builds the trace once, then runs legs on request (a line of JSON in, a line of JSON out)"""

    def __init__(self, a):
        import torch
        self.torch, self.a = torch, a
        self.pkg = pkg = load_pkg(a.root)
        self.R = 4 * a.blocks
        F = pkg.ROW_DRAW_PAD
        self.kinds = np.tile(np.array([0 | F, 1 | F, 2 | F, 3 | F], dtype=np.uint8), a.blocks)
        self.per_row = np.full(self.R, L_, dtype=np.uint32)
        self.data = block_rows(a.distinct, np.random.default_rng(17))
        self.ctxs = [pkg.Context(L_, K_, N_, device=a.device) for _ in range(a.inflight)]
        self.packed, self.lists = {}, {}

    def fmt(self, name):
        if name not in self.packed:
            p = pack_trace(self.pkg, name, self.a.blocks, self.data)
            assert len(p[0]) == expected_link_bytes(name, self.a.blocks)
            self.packed[name] = p
        return self.packed[name]

    def list_of(self, name):
        if name not in self.lists:
            system, _ = derive_system(self.pkg, self.a.blocks, name == "products")
            self.lists[name] = (system, derive_list(self.a.blocks, name == "products"))
        return self.lists[name]

    def leg(self, fmt, derive):
        pkg, torch, a, ctxs = self.pkg, self.torch, self.a, self.ctxs
        packed, widths = self.fmt(fmt)
        keep = torch.empty(len(packed), dtype=torch.uint8, pin_memory=True)
        keep.copy_(torch.from_numpy(packed))
        ptr = keep.data_ptr()
        traces, set_ms = [], []
        for c in ctxs:
            job = pkg.RowsJob()
            job.rows, job.kinds, job.msgs, job.msgs_on_device = self.R, self.kinds.ctypes.data, ptr, 0
            for i in range(32):
                job.encoding_seed[i] = i
                job.program_hash[i] = 0
            job.version = b"1.5.0"
            job.set_public_args(None)
            job.dense_rands_per_row = self.per_row.ctypes.data
            job.elem_bytes = widths.ctypes.data
            t = C.c_void_p()
            c.check(c.L.lig_rows_begin(c.h, C.byref(job), C.byref(t)))
            if derive:
                system, pairs = self.list_of(derive)
                t0 = time.perf_counter()
                info = c.rows_set_derived(t, system, pairs)
                set_ms.append(1e3 * (time.perf_counter() - t0))
                assert info.n_waves == (3 if derive == "products" else 1) and info.n_slots == len(pairs)
            traces.append([t, True])

        def loop(i, steps, last):
            c, t = ctxs[i], traces[i][0]
            out = None
            for s in range(steps):
                if not traces[i][1]:
                    c.check(c.L.lig_rows_restart(t, C.c_void_p(ptr), 0))
                c.rows_commit(t)
                traces[i][1] = s + 1 < steps or not last
                if traces[i][1]:                                                     # the next trace goes up under this proof
                    c.check(c.L.lig_rows_restart(t, C.c_void_p(ptr), 0))
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
            c.check(c.L.lig_rows_restart(t, C.c_void_p(ptr), 0))
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
        return {"ms_per_proof": 1e3 * dt / (a.inflight * a.steps), "sha256": hashlib.sha256(proofs[0]).hexdigest(), "link_bytes": len(packed),
                "set_derived_ms": statistics.median(set_ms) if set_ms else None, "derive_launch_ms": derive_ms}

    def serve(self):
        for line in sys.stdin:
            req = json.loads(line)
            if req.get("quit"):
                break
            print("RESULT " + json.dumps(self.leg(req["fmt"], req["derive"])), flush=True)
        for c in self.ctxs:
            c.close()


def write_profile(out, path):
    by = {e["leg"]: e for e in out["results"]}
    with open(path, "w") as f:
        f.write("# Product entries of derived slots: x = eval(3y + 5), z = x * y, v = eval(z + y) formed on the device (`tools/time_derived_products.py`)\n\n")
        f.write("One MI355X, one command, alternating legs, %d rounds of %d proofs x %d in flight; %d blocks of LINEAR, QX, QY, QZ rows x %d slots = %d "
                "constraints, half of them quadratic.  Every leg proves the same rows: `same_proof_across_legs` = %s.\n\n" % (
                    out["reps"], out["steps"], out["inflight"], out["blocks"], L_, out["constraints"], out["same_proof_across_legs"]))
        f.write("| leg | what | median ms/proof | spread (max - min) | all rounds | link bytes per trace |\n|---|---|---|---|---|---|\n")
        for e in out["results"]:
            f.write("| %s | %s | %.2f | %.2f | %s | %d |\n" % (e["leg"], e["what"], e["median_ms"], e["spread_ms"], ", ".join("%.2f" % x for x in e["ms_per_proof"]), e["link_bytes_per_trace"]))
        for e in out["results"]:
            if "set_derived_ms" in e:
                f.write("\nLeg %s: `lig_rows_set_derived` once per program (host plan, copies, table conversion) median %.1f ms (%s); the derive bracket of one commit "
                        "(`lig_profile_read_launches(rows_in_launch = 0)`, a separate untimed commit) median %.3f ms (%s).\n" % (
                            e["leg"], statistics.median(e["set_derived_ms"]), ", ".join("%.1f" % x for x in e["set_derived_ms"]),
                            statistics.median(e["derive_launch_ms"]), ", ".join("%.3f" % x for x in e["derive_launch_ms"])))
        f.write("\nMedian differences against the round spread of the two legs compared (the larger of the two):\n\n")
        for x, y, what in (("a", "b", "everything derived against everything shipped"), ("c", "a", "no list, parent build against this build"),
                           ("e", "d", "a list without product entries, parent build against this build")):
            if x in by and y in by:
                diff, spread = by[y]["median_ms"] - by[x]["median_ms"], max(by[x]["spread_ms"], by[y]["spread_ms"])
                f.write("* %s -> %s (%s): %+.2f ms, spread %.2f ms: %s\n" % (x, y, what, diff, spread, "within the spread" if abs(diff) <= spread else "BEYOND the spread"))
        f.write("\nOne GPU only.  What fewer link bytes and no host pass over the eval outputs are worth on a node whose GPUs share the host link is a "
                "prediction, not measured here.\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1049, help="blocks of LINEAR, QX, QY, QZ rows (1049 x 2 x 8000 = 2^24 constraints)")
    ap.add_argument("--legs", default="a,b,d")
    ap.add_argument("--distinct", type=int, default=4, help="distinct blocks of data, tiled over the trace")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent-root", default=None, help="a tree of the parent commit with its library built: legs c = a and e = d there")
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
    legs = a.legs.split(",") + (list(ON_PARENT) if a.parent_root else [])

    def spawn(root):
        return subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--root", os.path.abspath(root), "--blocks", str(a.blocks), "--distinct", str(a.distinct),
                                 "--steps", str(a.steps), "--warmup", str(a.warmup), "--inflight", str(a.inflight), "--device", str(a.device)],
                                stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    here, parent = spawn(ROOT), spawn(a.parent_root) if a.parent_root else None

    def ask(w, leg):
        fmt, der = LEGS[leg]
        w.stdin.write(json.dumps({"fmt": fmt, "derive": der}) + "\n")
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
                r = ask(parent if leg in ON_PARENT else here, leg)
                res[leg].append(r)
                print("leg %s round %d  %7.2f ms/proof  %11d link bytes/trace  sha256 %s%s" % (
                    leg, rep, r["ms_per_proof"], r["link_bytes"], r["sha256"][:16],
                    "" if r["derive_launch_ms"] is None else "  set_derived %.1f ms, derive bracket %.3f ms" % (r["set_derived_ms"], r["derive_launch_ms"])), flush=True)
    finally:
        for w in (here, parent):
            if w:
                try:
                    w.stdin.write(json.dumps({"quit": True}) + "\n")
                    w.stdin.flush()
                    w.wait(timeout=60)
                except Exception:
                    w.kill()
    out = {"tool": "time_derived_products", "blocks": a.blocks, "constraints": 2 * a.blocks * L_, "inflight": a.inflight, "steps": a.steps, "reps": a.reps,
           "same_proof_across_legs": len({r["sha256"] for v in res.values() for r in v}) == 1, "results": []}
    for leg in legs:
        ms = [r["ms_per_proof"] for r in res[leg]]
        e = {"leg": leg, "what": WHAT[leg], "ms_per_proof": ms, "median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "link_bytes_per_trace": res[leg][0]["link_bytes"]}
        if LEGS[leg][1]:
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
