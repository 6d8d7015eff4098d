#!/usr/bin/env python3
"""What a prepared linear program (lig_linear_prepare) buys over a system every trace owns, in ONE command on one box.

Shape: 2^24 single-term constraints (constraint c = slot c, coefficient +1) over full-width linear rows at bench.py's (l, k, n); the
first 2^20 constraints have a right-hand side with a table entry of its own (w_c = b_c, the "public outputs"), the other witnesses
are zero, so the statement holds and the constant is the system's own.  Legs ALTERNATE `--rounds` times, `--steps` calls each after
`--warmup`; every call is timed to its return (the verifier's and the prover's calls are blocking).

  (a) verifier, the path of the parent commit: lig_rows_verify_begin + lig_rows_verify_set_linear + lig_rows_verify_finish per proof
  (b) verifier with ONE program: lig_rows_verify_begin + lig_rows_verify_attach_linear + lig_rows_verify_finish per proof
  (c) prover, a new statement per proof (2^20 right-hand sides): restart + lig_rows_set_linear_values + commit + prove, against
      restart + lig_rows_set_linear + commit + prove
  (d) device memory of two traces in flight: two private systems against one shared program, from lig_linear_program_bytes (the
      sizes of the library's own allocations)

`--legs a` uses nothing this entry added, and `--pkg DIR` loads the binding and library of another build (the parent commit's
ligero-prover_amd directory): the same leg at the parent, in the same session.
Prints one JSON line."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_, K_, N_ = 8000, 8192, 32768              # bench.py's shape
P = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def load_pkg(path):
    spec = importlib.util.spec_from_file_location("ligero_prover_amd_timed", os.path.join(path, "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ms(samples):
    return {"min": round(min(samples), 3), "median": round(float(np.median(samples)), 3), "all": [round(v, 3) for v in samples]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-constraints", type=int, default=24)
    ap.add_argument("--log2-outputs", type=int, default=20, help="constraints with a right-hand side = table entries")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "ligero-prover_amd"))
    a = ap.parse_args()
    pkg = load_pkg(a.pkg)
    n, n_out = 1 << a.log2_constraints, 1 << a.log2_outputs
    assert n_out <= n
    R = -(-n // L_)
    rng = np.random.default_rng(1)

    def outputs():
        """n_out canonical elements (top limb below p's: every value < p)"""
        t = rng.integers(0, 1 << 32, (n_out, 8), dtype=np.uint32)
        t[:, 7] &= 0x0FFFFFFF
        return t

    def rows_for(tab):
        rows = np.zeros((R, K_, 8), dtype=np.uint32)
        flat = rows[:, :L_].reshape(-1, 8)          # a copy: the data slots in slot order
        flat[:n_out] = tab
        rows[:, :L_] = flat.reshape(R, L_, 8)
        return rows

    tabs = [outputs(), outputs()]
    rows = [rows_for(t) for t in tabs]
    kinds = np.full(R, pkg.ROW_DRAW_PAD, dtype=np.uint8)           # LINEAR rows, pads drawn by the library
    plain_kinds = np.zeros(R, dtype=np.uint8)
    idx = np.arange(n_out, dtype=np.uint32)

    def system(tab):
        return pkg.LinearSystem.make(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.full(n, pkg.COEF_ONE, dtype=np.uint32),
                                     idx, idx, tab)

    systems = [system(t) for t in tabs]
    ctx = pkg.Context(L_, K_, N_, device=0)
    res = {"constraints": n, "outputs": n_out, "rows": R, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "pkg": os.path.relpath(a.pkg, ROOT)}

    # one proof per statement, by the one-owner path
    tr, keep = ctx.rows_begin(kinds, rows[0])
    ctx.rows_set_linear(tr, systems[0])
    ctx.rows_commit(tr)
    proof, info = ctx.rows_prove(tr, None, None)
    assert (info.valid_code, info.valid_linear, info.valid_quad) == (1, 1, 1), "the statement does not hold"
    proofs = [proof]

    def timed(fn, count):
        out = []
        for i in range(a.warmup + count):
            t0 = time.perf_counter()
            fn(i)
            if i >= a.warmup:
                out.append(1e3 * (time.perf_counter() - t0))
        return out

    def verify(how):
        def once(_):
            vt, _, _ = ctx.rows_verify_begin(plain_kinds, proofs[0])
            how(vt)
            v = ctx.rows_verify_finish(vt, None, None)
            assert v.accept == 1, "the verifier rejects"
        return once

    prog = None
    if set("bcd") & set(a.legs):
        t0 = time.perf_counter()
        prog = ctx.linear_prepare(systems[0], plain_kinds)
        res["prepare_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    va, vb = [], []
    for _ in range(a.rounds):
        if "a" in a.legs:
            va += timed(verify(lambda vt: ctx.rows_verify_set_linear(vt, systems[0])), a.steps)
        if "b" in a.legs:
            vb += timed(verify(lambda vt: ctx.rows_verify_attach_linear(vt, prog)), a.steps)
    if va:
        res["a_verify_set_linear_ms"] = ms(va)
    if vb:
        res["b_verify_attached_ms"] = ms(vb)
    if va and vb:
        res["a_minus_b_ms"] = round(min(va) - min(vb), 3)

    if "c" in a.legs:
        ctx.rows_restart(tr, rows[0])
        ctx.rows_attach_linear(tr, prog)
        full = [np.ascontiguousarray(t) for t in tabs]

        def with_values(i):
            ctx.rows_restart(tr, rows[i & 1])
            ctx.rows_set_linear_values(tr, full[i & 1])
            ctx.rows_commit(tr)
            _, inf = ctx.rows_prove(tr, None, None, copy=False)
            assert inf.valid_linear == 1

        def with_set_linear(i):
            ctx.rows_restart(tr, rows[i & 1])
            ctx.rows_set_linear(tr, systems[i & 1])
            ctx.rows_commit(tr)
            _, inf = ctx.rows_prove(tr, None, None, copy=False)
            assert inf.valid_linear == 1

        def values_only(i):
            ctx.rows_set_linear_values(tr, full[i & 1])
            ctx.sync()

        cv, cs = [], []
        for _ in range(a.rounds):
            ctx.rows_restart(tr, rows[0])
            ctx.rows_attach_linear(tr, prog)
            ctx.rows_commit(tr)
            ctx.rows_prove(tr, None, None, copy=False)
            cv += timed(with_values, a.steps)
            cs += timed(with_set_linear, a.steps)
        res["c_proof_with_set_linear_values_ms"] = ms(cv)
        res["c_proof_with_set_linear_ms"] = ms(cs)
        ctx.rows_restart(tr, rows[0])
        ctx.rows_attach_linear(tr, prog)
        res["c_set_linear_values_alone_ms"] = ms(timed(values_only, a.steps))
    ctx.trace_destroy(tr)

    if "d" in a.legs:
        pb, ab = prog.bytes()
        res["d_program_bytes"], res["d_attachment_bytes"], res["d_values_bytes"] = pb, ab, 32 * n_out
        res["d_two_private_systems_bytes"] = 2 * (pb + ab)
        res["d_one_shared_program_bytes"] = pb + 2 * ab
    if prog is not None:
        prog.release()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
