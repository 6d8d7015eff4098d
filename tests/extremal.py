"""Extremal and limb-edge inputs for the field core (a helper, not a test file; numpy and Python integers only, no GPU).

Every end-to-end proof of the suite is otherwise taken over uniform field elements, which sit in the middle of every operand
range the lazy 29-bit-limb core (csrc/fr29.hpp) relies on.  The families here put every slot at an end of those ranges:
constant rows (the codeword of a constant row is that constant at all n positions: the largest magnitude the codeword-domain
accumulators see), flat and single-coefficient spectra, values on the 29- and 32-bit limb boundaries, and pairs (u, r) whose
Montgomery product has all-ones limbs, so that a sum of such products grows as fast as a sum of normalised values can.

All vectors are (count, 8) uint32 little-endian limbs of canonical values (< P, asserted)."""
import functools

import numpy as np

import oracle_lib as ol

P = ol.P
RP = 1 << 261                                              # the Montgomery radix R' of csrc/fr29.hpp
# the largest value below P whose low eight 29-bit limbs are all 2^29 - 1 and whose top limb is one below P's
T_ALLONES = (((P >> 232) - 1) << 232) | ((1 << 232) - 1)
GEN = 53                                                   # generated_at of every extremal trace

FAMILIES = ("zero", "one", "pm1", "delta", "alt", "geom", "limb_edges")
MIXED_CYCLE = ("pm1", "zero", "delta", "alt", "geom", "limb_edges", "allones_products", "one")
ROWS_FAMILIES = ("pm1", "zero", "delta", "alt", "geom", "limb_edges", "allones_products", "mixed")


def limbs(vals):
    """python ints, all canonical -> (len, 8) uint32"""
    vals = [int(v) for v in vals]
    assert all(0 <= v < P for v in vals)
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint32).reshape(len(vals), 8).copy()


@functools.lru_cache(maxsize=None)
def _core_model():
    """tools/check_fr29.py, the integer model of the device core: one list of limb-boundary values for both"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "check_fr29.py")
    spec = importlib.util.spec_from_file_location("check_fr29", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def limb_edge_values():
    """the values on the limb boundaries of both representations (9 x 29 bits on the device, 8 x 32 bits in memory)"""
    v = _core_model().limb_edge_values()
    assert all(0 <= x < P for x in v)
    return v


@functools.lru_cache(maxsize=None)
def omega(k):
    """the oracle's k-th root of unity (lo_omegas)"""
    w = [np.zeros((1, 8), dtype=np.uint32) for _ in range(3)]
    ol.lib().lo_omegas(int(k), *[ol.ptr(x) for x in w])
    g = ol.from_limbs(w[0])[0]
    assert pow(g, k, P) == 1 and pow(g, k // 2, P) == P - 1
    return g


def _cycle(pattern, count, shift=0):
    pat = limbs(pattern)
    idx = (np.arange(count) + shift) % len(pattern)
    return pat[idx]


def family(name, count, k=None, shift=0):
    """(count, 8) uint32 of the named family; k: the transform length whose root `geom` uses (default: count); shift rotates
    the cyclic families, so that rows of one trace differ"""
    if name == "zero":
        return _cycle([0], count)
    if name == "one":
        return _cycle([1], count)
    if name == "pm1":
        return _cycle([P - 1], count)
    if name == "delta":
        out = _cycle([0], count)
        if count:
            out[0] = limbs([P - 1])[0]
        return out
    if name == "alt":
        return _cycle([P - 1, 0], count)
    if name == "geom":                                      # c * g^i, c = P - 1: one non-DC coefficient
        g, v, vals = omega(k or count), P - 1, []
        for _ in range(count):
            vals.append(v)
            v = v * g % P
        return limbs(vals)
    if name == "limb_edges":
        return _cycle(limb_edge_values(), count, shift)
    raise KeyError(name)


def allones_partner(u_vals, plain=False):
    """r with f29_montmul(u, r) == T_ALLONES exactly (plain: u * r == T_ALLONES mod P, for entries that take the constant in
    Montgomery form).  Where u is zero the partner is T_ALLONES itself."""
    # one inversion for the whole vector (prefix products), zeros skipped
    nz = [u for u in u_vals if u]
    pre, run = [], 1
    for u in nz:
        pre.append(run)
        run = run * u % P
    inv, invs = pow(run, -1, P), [0] * len(nz)
    for i in range(len(nz) - 1, -1, -1):
        invs[i] = inv * pre[i] % P
        inv = inv * nz[i] % P
    out, it, rinv = [], iter(invs), pow(RP, -1, P)
    for u in u_vals:
        if u == 0:
            out.append(T_ALLONES)
            continue
        r = T_ALLONES * (1 if plain else RP) * next(it) % P
        if plain:
            assert u * r % P == T_ALLONES
        else:
            # the Montgomery product is the representative of u*r/R' in [u*r/R', u*r/R' + p): T itself when T >= u*r // R'
            assert u * r * rinv % P == T_ALLONES and T_ALLONES >= u * r // RP
        out.append(r)
    return out


def random_nonzero(count, rng):
    """(count, 8) uint32: uniform nonzero values below 2^252 (< P)"""
    raw = rng.integers(0, 1 << 32, size=(count, 8), dtype=np.uint64).astype(np.uint32)
    raw[:, 7] &= 0x0FFFFFFF
    raw[~raw.any(axis=1), 0] = 1
    return raw


def allones_products(count, rng, plain=False):
    """-> (u, r): u random nonzero, u[i] * r[i] / R' (plain: u[i] * r[i]) is T_ALLONES"""
    assert T_ALLONES < P and all((T_ALLONES >> (29 * i)) & 0x1FFFFFFF == 0x1FFFFFFF for i in range(8))
    u = random_nonzero(count, rng)
    return u, limbs(allones_partner(ol.from_limbs(u), plain))


def _mul(x, y):
    return limbs([a * b % P for a, b in zip(ol.from_limbs(x), ol.from_limbs(y))])


@functools.lru_cache(maxsize=None)
def build_extremal_trace(l, k, n, n_rows_linear, n_triples, fam, seed=7):
    """-> (kinds, rows, (mask_code, mask_lin, mask_quad), rands): the oracle's kinds and masks for n_rows_linear linear rows and
    n_triples quadratic triples; all k slots of every witness row (pads too: the rows are shipped without ROW_DRAW_PAD) from the
    family, z = x * y over all k slots; randomness rows from the same family on the l data slots, zero beyond.
    fam "allones_products": row r holds u, its randomness row the partner; "mixed": MIXED_CYCLE row by row.
    Cached and shared: callers must not write to the arrays."""
    job = ol.make_job(l, k, n, 192, l * n_rows_linear, l * n_triples, generated_at=GEN, threads=4)
    rows, mc, ml, mq = ol.form_rows(job)
    kinds = ol.row_kinds(job).copy()
    R = len(kinds)
    assert R == n_rows_linear + 3 * n_triples and int((kinds == 0).sum()) == n_rows_linear and int((kinds == 1).sum()) == n_triples
    rng = np.random.default_rng(seed)
    rows = np.zeros((R, k, 8), dtype=np.uint32)
    rands = np.zeros((R, k, 8), dtype=np.uint32)
    fam_of = [MIXED_CYCLE[r % len(MIXED_CYCLE)] if fam == "mixed" else fam for r in range(R)]
    for r in range(R):
        f = fam_of[r]
        if kinds[r] == 3:
            rows[r] = _mul(rows[r - 2], rows[r - 1])
        elif f == "allones_products":
            rows[r] = random_nonzero(k, rng)
        else:
            rows[r] = family(f, k, k, shift=r)
        if f == "allones_products":
            rands[r, :l] = limbs(allones_partner(ol.from_limbs(rows[r, :l])))
        else:
            rands[r, :l] = family(f, l, k, shift=3 * r + 1)
    for a in (kinds, rows, mc, ml, mq, rands):
        a.setflags(write=False)
    return kinds, rows, (mc, ml, mq), rands


@functools.lru_cache(maxsize=None)
def oracle_proof(l, k, n, n_rows_linear, n_triples, fam):
    """ol.prove_rows over the trace, the linear constant derived from the rows (const_sum = None)"""
    kinds, rows, masks, rands = build_extremal_trace(l, k, n, n_rows_linear, n_triples, fam)
    return ol.prove_rows(l, k, n, 192, kinds, rows, *masks, rands, None, generated_at=GEN, threads=4)


# (l, k, n, linear rows, triples, family) of every trace the GPU tests prove
SMALL = (320, 512, 2048)
ROWS_CASES = [SMALL + (130, 2, f) for f in ROWS_FAMILIES]           # full and ragged groups of 64, 16, 8 and 6 rows
ROWS_CASES += [SMALL + (520, 3, "mixed")]                           # crosses the 512-row chunk
ROWS_CASES += [(832, 1024, 4096, 130, 2, f) for f in ("pm1", "allones_products")]     # tile length 128: the extra radix-2 stage
ZRES_CASES = [SMALL + (r, 0, f) for r in (130, 520) for f in ("pm1", "allones_products", "mixed")]
GENERIC_CASES = [SMALL + (130, 2, f) for f in ("pm1", "mixed")]
ALL_TRACES = sorted(set(ROWS_CASES + ZRES_CASES + GENERIC_CASES))
