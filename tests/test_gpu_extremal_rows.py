"""GPU: extremal and limb-edge inputs (tests/extremal.py) through the public entry points, bit for bit against the CPU oracle.

The hot path is a lazy, redundant arithmetic core (csrc/fr29.hpp) whose correctness rests on operand bounds; uniform inputs sit
in the middle of every one of them.  Here every slot is at an end: constant rows of p - 1 (the codeword is p - 1 at all n
positions), flat and single-coefficient spectra, limb-boundary values, and witness x randomness pairs whose Montgomery product
has all-ones limbs -- a renormalisation interval that is one too long then overflows with certainty, not with small probability.
No tolerances: integer arithmetic mod p and SHA-256."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import extremal as ex
import hip_lib
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
P = ol.P


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


def case_id(c):
    return "-".join(str(x) for x in c)


# ------------------------------------------------------------------------------------------------ (a), (b): the rows entry
def rows_case(amd, case):
    """rows_begin (device rows, own pads) -> rows_commit -> rows_prove(rands, None), rows_restart + commit + prove, then the verifier's
    two halves; -> dict of named comparisons with the oracle's prover over the same rows (all must be True), and under
    "tiled_launches" the library's own count of multi-row launches of the tiled row encoder during the two proofs (lig_profile_read):
    zero exactly when the context takes the generic radix-2 row path"""
    l, k, n, n_lin, n_tri, fam = case
    kinds, rows, masks, rands = ex.build_extremal_trace(*case)
    want = ex.oracle_proof(*case)
    out = {}
    c = amd.Context(l, k, n)
    try:
        d_rows = c.upload(rows)
        c.profile_enable()
        tr, keep = c.rows_begin(kinds, d_rows, on_device=True, generated_at=ex.GEN)
        root, seed1 = c.rows_commit(tr)
        out["root"], out["stage1_seed"] = root == want["root"], seed1 == want["stage1_seed"]
        proof, info = c.rows_prove(tr, rands, None)
        out["rows"] = info.rows == want["rows"]
        out["const_sum"] = bytes(info.const_sum) == want["const_sum"]
        out["stage2_seed"] = bytes(info.stage2_seed) == want["stage2_seed"]
        out["valid"] = [info.valid_code, info.valid_linear, info.valid_quad] == list(want["valid"])
        out["proof"] = proof == want["proof"]
        c.rows_restart(tr, d_rows, on_device=True)
        out["restart_commit"] = c.rows_commit(tr) == (root, seed1)
        proof2, info2 = c.rows_prove(tr, rands, None)
        out["restart_proof"] = proof2 == proof and bytes(info2.const_sum) == bytes(info.const_sum)
        c.trace_destroy(tr)
        out["tiled_launches"] = c.profile_read()[0]
        c.profile_enable(False)
        vt, vseed, vinfo = c.rows_verify_begin(kinds, proof)
        out["verify_begin"] = vt is not None and vseed == seed1 and vinfo.parsed == 1 and vinfo.indices_match == 1
        if vt is not None:
            v = c.rows_verify_finish(vt, rands, want["const_sum"])
            out["verify_valid"] = [v.valid_code, v.valid_linear, v.valid_quad] == list(want["valid"])
            out["verify_equal"] = [v.code_equal, v.linear_equal, v.quad_equal, v.valid_merkle] == [1, 1, 1, 1]
            out["verify_accept"] = v.accept == int(all(want["valid"]))
    finally:
        c.close()
    return out


def assert_case(case, report, generic=False):
    report = dict(report)
    launches = report.pop("tiled_launches")
    failed = [name for name, ok in report.items() if ok is not True]
    assert not failed and len(report) == 13, (case, failed)
    assert (launches == 0) if generic else (launches > 0), (case, launches)


@pytest.mark.parametrize("case", ex.ROWS_CASES, ids=case_id)
def test_rows_entry_on_extremal_rows_equals_oracle(amd, case):
    """130 linear rows + 2 triples: full and ragged groups of 64, 16, 8 and 6 rows; 520 + 3: the group partials persist across the
    512-row launches; l = 832, k = 1024: tile length 128 with the extra radix-2 stage"""
    assert_case(case, rows_case(amd, case))


TRANSFORM_FAMILIES = ("pm1", "delta", "alt", "geom", "limb_edges")


def encode_rows_case(amd, k, fams):
    """lig_encode_rows of one row per family against the oracle -> dict of named comparisons, and under "tiled_launches" the
    library's own count of launches of the tiled row encoder (lig_profile_read): zero exactly on the generic radix-2 row path"""
    n, l = 4 * k, k - 192
    msgs = np.stack([ex.family(f, k, k) for f in fams])
    want = ol.Ctx(l, k, n).encode_rows(msgs, threads=4)
    c = amd.Context(l, k, n)
    try:
        dm, dc = c.upload(msgs), c.malloc(len(fams) * 32 * n)
        c.profile_enable()
        c.encode_rows(dm, dc, len(fams))
        got = c.download(dc, (len(fams), n, 8))
        launches = c.profile_read()[0]
    finally:
        c.close()
    out = {f: bool(np.array_equal(got[i], want[i])) for i, f in enumerate(fams)}
    out["constant_row"] = bool(np.array_equal(got[0], ex.family("pm1", n))) and fams[0] == "pm1"
    out["tiled_launches"] = launches
    return out


def assert_encode_rows(report, fams, generic):
    report = dict(report)
    launches = report.pop("tiled_launches")
    assert all(v is True for v in report.values()) and sorted(report) == sorted(list(fams) + ["constant_row"]), report
    assert (launches == 0) if generic else (launches > 0), launches


# the knobs (LIG_ZRES, LIG_ENCODE_GENERIC) are read once per process, by its first context: every case under one runs in a child
CHILD = textwrap.dedent('''
    import json, os, sys
    root = sys.argv[1]; cases = json.loads(sys.argv[2])
    sys.path.insert(0, os.path.join(root, "tests"))
    import hip_lib
    import test_gpu_extremal_rows as te
    amd = hip_lib.load()
    out = []
    for c in cases:
        out.append(te.encode_rows_case(amd, c[1], c[2]) if c[0] == "encode_rows" else te.rows_case(amd, tuple(c)))
    print(json.dumps(out))
''')


def run_child(tmp_path, cases, env):
    script = tmp_path / "extremal_child.py"
    script.write_text(CHILD)
    p = subprocess.run([sys.executable, str(script), ROOT, json.dumps(cases)], env=dict(os.environ, **env), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    reports = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("[")][-1])
    assert len(reports) == len(cases)
    return reports


def test_generic_row_path_on_extremal_rows_equals_oracle(tmp_path):
    """the radix-2 row path of contexts without the tiled encoder (planar codewords through strided copies, coset-2 values by the
    separate pass), forced at small k by LIG_ENCODE_GENERIC=1 in a child process: the whole rows entry on pm1 and mixed, and
    the batched encode of one row per family.  Every report shows that the knob took: no launch of the tiled encoder."""
    cases = [list(c) for c in ex.GENERIC_CASES] + [["encode_rows", 512, list(TRANSFORM_FAMILIES)]]
    assert [c[5] for c in ex.GENERIC_CASES] == ["pm1", "mixed"]
    reports = run_child(tmp_path, cases, dict(LIG_ENCODE_GENERIC="1"))
    for case, rep in zip(ex.GENERIC_CASES, reports):
        assert_case(case, rep, generic=True)
    assert_encode_rows(reports[-1], TRANSFORM_FAMILIES, generic=True)


def test_generic_row_encoder_beyond_the_tiled_sizes():
    """k = 65536 is past the tiled row encoder (k <= 32768): lig_encode_rows takes the radix-2 kernels there without any knob.
    3 rows: the oracle's transforms of 2^18 elements are what the test waits for."""
    fams = ("pm1", "geom", "limb_edges")
    assert_encode_rows(encode_rows_case(hip_lib.load(), 65536, fams), fams, generic=True)


@pytest.mark.parametrize("n_rows", [130, 520])
def test_resident_tiles_on_extremal_rows_equal_oracle(tmp_path, n_rows):
    """LIG_ZRES=1 (read once per process: a child process, as tests/test_gpu_zres.py): the last radix-8 pass inside the column hash,
    stage 2 / 3 from the tiles (k_encode_out_dot_z, k_gather_rows_z).  Traces without triples -- triples keep the planar matrix."""
    cases = [c for c in ex.ZRES_CASES if c[3] == n_rows]
    assert [c[5] for c in cases] == ["pm1", "allones_products", "mixed"] and all(c[4] == 0 for c in cases)
    reports = run_child(tmp_path, [list(c) for c in cases], dict(LIG_ZRES="1"))
    for case, rep in zip(cases, reports):
        assert_case(case, rep)


# ------------------------------------------------------------------------------------------------ (c): lig_rlc_rows
def rlc_reference(U, Rn, acc, rc, triples, rq):
    """the reference's per-row sequence (as test_rlc_and_gather_vs_oracle)"""
    n = U.shape[1]
    code, lin, quad = (a.copy() for a in acc)
    for r in range(U.shape[0]):
        ol.eltwise(10, U[r], None, code, scalar=rc[r])
        ol.eltwise(9, U[r], Rn[r], lin)
    for (x, y, z), q in zip(triples, rq):
        t1, t2 = np.zeros((n, 8), np.uint32), np.zeros((n, 8), np.uint32)
        ol.eltwise(6, U[x], U[y], t1); ol.eltwise(1, t1, U[z], t2); ol.eltwise(10, t2, None, quad, scalar=q)
    return code, lin, quad


@pytest.mark.parametrize("which", ["all_max", "allones_products"])
def test_rlc_rows_on_extremal_rows(amd, which):
    """lig_rlc_rows runs k_rlc_rows on the 8 x 32-bit core (fr.hpp), not on the 29-bit-limb one: nothing is lazy in it, so this is
    edge-value coverage of that entry and no renormalisation coverage (the rows entry above is).  The all-ones pairs are therefore
    taken in their plain form, U * Rn = the all-ones value."""
    n, rows = 2048, 135                                           # 2 * 64 + 7
    triples = [(0, 1, 2), (4, 5, 6), (130, 131, 134)]
    if which == "all_max":
        U = np.broadcast_to(ex.family("pm1", n), (rows, n, 8)).copy()
        Rn = U.copy()
        acc = [ex.family("pm1", n) for _ in range(3)]
        rc, rq = [P - 1] * rows, [P - 1] * 3
    else:
        rng = np.random.default_rng(17)
        pairs = [ex.allones_products(n, rng, plain=True) for _ in range(rows)]          # U[r][j] * Rn[r][j] = the all-ones value (this entry multiplies plain values)
        U, Rn = np.stack([u for u, _ in pairs]), np.stack([r for _, r in pairs])
        # rc[r]: U[r][0] * rc[r] is the all-ones value (the entry takes the constant to Montgomery form itself)
        rc = ex.allones_partner([ol.from_limbs(U[r, :1])[0] for r in range(rows)], plain=True)
        assert all(ol.from_limbs(U[r, :1])[0] * rc[r] % P == ex.T_ALLONES for r in range(rows))
        acc = [ex.family("limb_edges", n, shift=s) for s in (0, 5, 11)]
        rq = ex.limb_edge_values()[-4:-1]
    code, lin, quad = rlc_reference(U, Rn, acc, rc, triples, rq)
    c = amd.Context(320, 512, n)
    try:
        dU, dR = c.upload(U), c.upload(Rn)
        dc, dl, dq = (c.upload(a) for a in acc)
        c.rlc_rows(dU, dR, rows, rc, dc, dl, triples, rq, dq)
        assert np.array_equal(c.download(dc, (n, 8)), code)
        assert np.array_equal(c.download(dl, (n, 8)), lin)
        assert np.array_equal(c.download(dq, (n, 8)), quad)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ (d): transforms
@pytest.mark.parametrize("k", [512, 1024, 2048, 8192, 16384, 32768])
def test_transforms_on_extremal_rows(amd, k):
    """the tiled encoder and the tiled single-row transforms at tile lengths 64, 128, 256, 1024, 2048 and 4096 (k = 32768 is the
    largest k with the tiled encoder: the batched encode takes 3 rows there).  The radix-2 row encoder is covered by
    test_generic_row_path_* and test_generic_row_encoder_* above; the radix-2 single-row transforms start at n > 2^20, which
    no test of a few seconds reaches."""
    n, l = 4 * k, k - 192
    c = amd.Context(l, k, n)
    o = ol.Ctx(l, k, n)
    pm1_n = ex.family("pm1", n)
    try:
        c.profile_enable()
        fams = TRANSFORM_FAMILIES if k < 32768 else ("pm1", "geom", "limb_edges")
        msgs = np.stack([ex.family(f, k, k) for f in fams])
        dm, dc = c.upload(msgs), c.malloc(len(fams) * 32 * n)
        c.encode_rows(dm, dc, len(fams))
        got = c.download(dc, (len(fams), n, 8))
        want_rows = o.encode_rows(msgs, threads=4)
        assert np.array_equal(got, want_rows)
        assert np.array_equal(got[0], pm1_n)                      # a constant row is the constant at all n positions
        assert c.profile_read()[0] > 0                            # the tiled encoder ran
        buf = c.malloc(32 * n)
        for f in TRANSFORM_FAMILIES:
            m = ex.family(f, k, k)
            x = np.zeros((n, 8), dtype=np.uint32); x[:k] = m
            c.write(buf, x); c.encode(buf)
            cw = c.download(buf, (n, 8))
            want = o.encode(m)
            assert np.array_equal(cw, want), f
            if f == "pm1":
                assert np.array_equal(cw, pm1_n)
            c.decode(buf)                                         # decode(encode(m)) = m || 0
            dec = c.download(buf, (n, 8))
            assert np.array_equal(dec, o.decode(want)), f
            assert np.array_equal(dec[:k], m) and not dec[k:].any(), f
            m2 = np.zeros((n, 8), dtype=np.uint32); m2[:2 * k] = ex.family(f, 2 * k, k)
            c.write(buf, m2); c.encode_2k(buf)
            assert np.array_equal(c.download(buf, (n, 8)), o.encode_2k(m2[:2 * k])), f
            for which, size in ((0, k), (1, 2 * k), (2, n)):
                x = np.zeros((n, 8), dtype=np.uint32); x[:size] = ex.family(f, size, k)
                for inverse in (False, True):
                    c.write(buf, x); c.ntt(buf, which, inverse)
                    res = c.download(buf, (n, 8))
                    assert np.array_equal(res[:size], o.ntt(which, inverse, x[:size])), (f, which, inverse)
                    assert np.array_equal(res[size:], x[size:]), (f, which, inverse)
        # decode of the all-(p - 1) vector of length n: not a codeword, raw coefficients stay in [k, n)
        c.write(buf, pm1_n); c.decode(buf)
        assert np.array_equal(c.download(buf, (n, 8)), o.decode(pm1_n))
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ (e): elementwise
@pytest.mark.parametrize("fam", ["limb_edges", "pm1"])
def test_eltwise_all_ops_on_extremal_operands(amd, fam):
    """test_eltwise_all_ops's loop over the 13 ops with both operands (and the accumulated output) from one family"""
    N = 4099
    x, y, o = ex.family(fam, N, shift=0), ex.family(fam, N, shift=7), ex.family(fam, N, shift=19)
    scalar = P - 1
    c = amd.Context(320, 512, 2048)
    try:
        dx, dy = c.upload(x), c.upload(y)
        for op in range(13):
            do = c.upload(o)
            want = o.copy()
            ol.eltwise(op, x, y, want, scalar=scalar, bit=231)     # bit 231: the top bit of 29-bit limb 7
            c.eltwise(op, dx, dy, do, N, scalar=scalar, bit=231)
            assert np.array_equal(c.download(do, (N, 8)), want), "op %d" % op
            c.free(do)
    finally:
        c.close()


def test_division_by_limb_edge_values(amd):
    """DIV with y = limb_edges (every value nonzero) and with x = y: the quotient is 1"""
    N = 4099
    rng = np.random.default_rng(23)
    y = ex.family("limb_edges", N, shift=2)
    c = amd.Context(320, 512, 2048)
    try:
        for x in (ol.rand_field(rng, N), ex.family("limb_edges", N, shift=9), ex.family("pm1", N), y):
            dx, dy, do = c.upload(x), c.upload(y), c.malloc(32 * N)
            want = np.zeros_like(x)
            ol.eltwise(11, x, y, want)
            c.eltwise("DIV", dx, dy, do, N)
            assert np.array_equal(c.download(do, (N, 8)), want)
            if x is y:
                assert np.array_equal(want, ex.family("one", N))
            for p in (dx, dy, do):
                c.free(p)
    finally:
        c.close()
