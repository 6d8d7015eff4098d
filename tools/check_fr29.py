#!/usr/bin/env python3
"""Exact integer model of the 29-bit-limb field core (ligero-prover_amd/csrc/fr29.hpp) on Python integers:
f29_montmul, f29_qnorm, f29_reduce_2p, f29_canon, f29_sub_k2/4/8/16, unpack29 / pack29 and the lazy accumulation loops built
from them, at the corners of the operand ranges the header states.  (f29_mulw has its own: tools/gen_fr29_mulw.py --check.)

Every constant is parsed from the committed csrc/fr29_consts.hpp; the Montgomery columns are tools/gen_fr29_montmul.py's own
tables, so the model multiplies what the generated header multiplies.  Every intermediate the C++ keeps in 32 or 64 bits goes
through u32() / u64(), which assert that it fits.
    python tools/check_fr29.py          prints one "ok: ..." line per primitive, raises on the first violated bound"""
import os
import random
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_fr29_montmul  # noqa: E402

P = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
W, L = 29, 9
RP = 1 << (W * L)


def parse_consts(path=os.path.join(HERE, "..", "ligero-prover_amd", "csrc", "fr29_consts.hpp")):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"#define (F29_\w+)\(i\) \(([^\n]*)\)\n", text):
        vals = [int(x, 16) for x in re.findall(r"0x([0-9A-Fa-f]+)u", m.group(2))]
        assert len(vals) == L, m.group(1)
        out[m.group(1)] = vals
    for m in re.finditer(r"#define (F29_\w+) 0x([0-9A-Fa-f]+)u", text):
        out[m.group(1)] = int(m.group(2), 16)
    return out


K = parse_consts()
MASK, N0, RECIP229 = K["F29_MASK"], K["F29_N0"], K["F29_RECIP229"]
PL, PBAR = K["F29_P"], K["F29_PBAR"]


def u32(x):
    assert 0 <= x < 1 << 32, "does not fit 32 bits: %x" % x
    return x


def u64(x):
    assert 0 <= x < 1 << 64, "does not fit 64 bits: %x" % x
    return x


def value(x):
    return sum(v << (W * i) for i, v in enumerate(x))


def norm(v):
    """normalised limbs of a value below 2^(232 + 32)"""
    return [(v >> (W * i)) & MASK for i in range(L - 1)] + [u32(v >> (W * (L - 1)))]


def lazify(x, amount):
    """the same value with carries pushed back down: limb i takes amount(i) * 2^29 from limb i + 1 where both stay in 32 bits"""
    x = list(x)
    for i in range(L - 2, -1, -1):
        t = min(amount(i), x[i + 1], ((1 << 32) - 1 - x[i]) >> W)
        x[i + 1] -= t
        x[i] += t << W
    return x


# ---------------------------------------------------------------------------------------------- the primitives, restated
def montmul(a, b, check=True):
    """f29_montmul: the generated columns, one 64-bit accumulator"""
    m, t, acc = [0] * L, [0] * L, 0
    for ab, mp, quot, res in gen_fr29_montmul.columns():
        for i, j in ab:
            acc = u64(acc + u32(a[i]) * u32(b[j]))
        for i, j in mp:
            acc = u64(acc + m[i] * PL[j])
        if quot is not None:
            m[quot] = (((acc & 0xFFFFFFFF) * N0) & 0xFFFFFFFF) & MASK
            acc = u64(acc + m[quot] * PL[0])
            assert acc & MASK == 0
        else:
            t[res] = acc & MASK
        acc >>= W
    t[8] = u32(acc)
    if check:
        va, vb, vt = value(a), value(b), value(t)
        assert vt * RP == va * vb + value(m) * P                      # exact: (a*b + m*p) / R'
        assert vt % P == va * vb * pow(RP, -1, P) % P
        assert all(v <= MASK for v in t[:8]) and vt * RP < va * vb + P * RP
    return t


def qnorm(a):
    r = [u32(a[0]) & MASK]
    for i in range(1, 8):
        r.append(u32((u32(a[i]) & MASK) + (a[i - 1] >> W)))
    r.append(u32(u32(a[8]) + (a[7] >> W)))
    assert value(r) == value(a) and all(v < (1 << W) + 8 for v in r[:8])
    return r


def reduce_2p(a):
    va = value(a)
    assert va < RP
    hh = u32(u32((a[8] << 3)) + (u32(a[7]) >> 26))
    assert hh << 229 <= va
    q = u64(hh * RECIP229) >> 56
    assert q in (va // P, va // P - 1), (hex(va), q, va // P)
    r, acc = [], 0
    for i in range(L):
        acc = u64(acc + u32(a[i]))
        acc = u64(acc + q * PBAR[i])
        r.append(acc & MASK)
        acc >>= W
    vr = value(r)
    assert vr == va - q * P and 0 <= vr < 2 * P and r[8] < 1 << 25
    return r


def canon(a):
    r = reduce_2p(a)
    d, br = [], 0
    for i in range(L):
        s = r[i] - PL[i] + br
        assert -(1 << 31) <= s < 1 << 31
        d.append(s & MASK)
        br = s >> W                                                     # Python's >> is arithmetic, as the C++'s on int32_t
        assert br in (0, -1)
    o = r if br < 0 else d
    assert value(o) == value(a) % P and all(v <= MASK for v in o)
    return o


def sub_k(a, b, name):
    Kc = K[name]
    r = []
    for i in range(L):
        assert Kc[i] >= b[i], "%s limb %d lends less than the subtrahend takes" % (name, i)
        r.append(u32(u32(a[i]) + u32(Kc[i] - b[i])))
    assert value(r) == value(a) + value(Kc) - value(b)
    return r


def alignbit(hi, lo, s):
    return (((hi << 32) | lo) >> s) & 0xFFFFFFFF


def unpack29(w):
    r = [w[0] & MASK] + [alignbit(w[i], w[i - 1], 32 - 3 * i) & MASK for i in range(1, 8)] + [w[7] >> 8]
    assert value(r) == sum(v << (32 * i) for i, v in enumerate(w)) and all(v <= MASK for v in r)
    return r


def pack29(x):
    w = [(x[0] | (x[1] << 29)) & 0xFFFFFFFF]
    for i in range(1, 8):
        w.append(((x[i] >> (3 * i)) | (x[i + 1] << (29 - 3 * i))) & 0xFFFFFFFF)
    return w


def words(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


# ---------------------------------------------------------------------------------------------- inputs
def limb_edge_values():
    """the values on the limb boundaries of both representations, 9 x 29 bits on the device and 8 x 32 bits in memory
    (tests/extremal.py takes its limb_edges family from here)"""
    v = []
    for i in range(1, 9):
        v += [1 << (29 * i), (1 << (29 * i)) - 1]
    for i in range(1, 8):
        v += [1 << (32 * i), (1 << (32 * i)) - 1]
    v += [P - (1 << (29 * i)) for i in range(9)]
    v.append(((P >> 232) << 232) - 1)                                 # low eight 29-bit limbs all ones, top limb one below p's
    v += [(P - 1) // 2, (P + 1) // 2]
    return v


T_ALLONES = (((P >> 232) - 1) << 232) | ((1 << 232) - 1)             # the largest normalised value a product below p can have in its low limbs
EDGES = [0, 1, P - 1, T_ALLONES] + limb_edge_values()


# ---------------------------------------------------------------------------------------------- the checks
def check_constants():
    assert PL == norm(P) and PBAR == norm(RP - P) and MASK == (1 << W) - 1
    assert N0 == (-pow(P, -1, 1 << W)) % (1 << W)
    assert RECIP229 == (1 << 56) // ((P >> 229) + 1)
    assert K["F29_R2"] == norm(RP * RP % P) and K["F29_ONE_M"] == norm(RP % P)
    assert value(K["F29_K64P"]) == 64 * P and K["F29_K64P"] == norm(64 * P)
    print("ok: constants of fr29_consts.hpp are p, 2^261 - p, -1/p mod 2^29, the reciprocal, R' and R'^2 mod p")


# f29_sub_k*: (constant, multiple of p, lend c, largest limb of an admissible subtrahend below the top one).  K = mult * p with
# c * 2^29 lent to every limb below the top one: limbs 1..7 are >= c * (2^29 - 1), the top limb is (mult * p >> 232) - c.  So the
# admissible subtrahends are: limbs 0..7 <= c * (2^29 - 1)... and value < mult * p - c * 2^232 (NOT "< mult * p": a subtrahend in
# the last c * 2^232 below mult * p has a top limb the constant's does not cover).
SUBK = (("F29_K2P_C1", 2, 1, (1 << 29) - 1), ("F29_K4P_C2", 4, 2, (1 << 30) - 2), ("F29_K8P_C4", 8, 4, (1 << 31) - 4), ("F29_K16P_C2", 16, 2, (1 << 30) - 2))
# What the kernels subtract: the largest value and limb of each call site's subtrahend.  These figures are READ OFF the call
# sites named here, nothing derives them from the code: whoever changes one of those butterflies updates its line.
#   f29_sub_k2:  radix8_dit spans 4 and 8 (tile_dft.hpp: t = tab_mul(...)), tile_step S > 0 and its radix-2 tail (t1, t3, ta, tb):
#                products, f29_montmul < 1.2p or f29_mulw < p(1 + 2^-20); k_quad_rows (prover_kernels.hip: zq, a product);
#                k_sum_elems (neg_out: a canonical sum)
#   f29_sub_k4:  radix8_dit span 2 and tile_step S == 0 spans 2: the transform's inputs, normalised, < 3p
#   f29_sub_k8:  radix8_dit span 4 pairs (0,2),(4,6) and tile_step S == 0 span 4: a sum of two such inputs
#   f29_sub_k16: radix8_dit span 8 pair (0,4): a sum of four inputs after f29_qnorm
SUBK_CALLERS = {"F29_K2P_C1": (P + P // 5, MASK),
                "F29_K4P_C2": (3 * P, MASK),
                "F29_K8P_C4": (6 * P, (1 << 30) - 2),
                "F29_K16P_C2": (12 * P, (1 << W) + 7)}


def check_sub_k(rng):
    for name, mult, c, limb_max in SUBK:
        Kc = K[name]
        assert value(Kc) == mult * P and all(0 <= v < 1 << 32 for v in Kc)
        assert Kc[0] >= limb_max and all(v >= limb_max for v in Kc[1:8]) and Kc[8] == (mult * P >> 232) - c
        vmax = mult * P - (c << 232)                                  # exclusive
        # corners: every low limb at its bound with the largest admissible top limb; the largest admissible value
        top = (vmax - 1) >> 232
        assert top == Kc[8]
        corner = [limb_max] * 8 + [0]
        corner[8] = (vmax - 1 - value(corner)) >> 232
        cases = [corner, norm(vmax - 1), [0] * L, norm(P - 1)]
        for _ in range(500):
            b = [rng.randrange(limb_max + 1) for _ in range(8)] + [0]
            room = (vmax - 1 - value(b)) >> 232
            b[8] = rng.randrange(room + 1)
            cases.append(b)
        amax = (1 << 32) - 1 - max(Kc)                                # the minuend limb that still leaves the sum in 32 bits
        for b in cases:
            assert value(b) < vmax
            for a in ([0] * L, [amax] * L, [rng.randrange(amax + 1) for _ in range(L)]):
                sub_k(a, b, name)
        # the first value past the admissible range is NOT covered: the stated "< mult * p" was too wide
        try:
            sub_k([0] * L, norm(mult * P - 1), name)
            raise SystemExit("%s covers a subtrahend just below %d p after all: tighten this check" % (name, mult))
        except AssertionError:
            pass
        cv, cl = SUBK_CALLERS[name]
        assert cv <= vmax and cl <= limb_max, name                   # every call site stays inside
    print("ok: K2P/K4P/K8P/K16P are multiples of p and cover every subtrahend with limbs <= c(2^29 - 1), value < mult*p - c*2^232; "
          "all call sites stay inside")


def check_pack(rng):
    vals = EDGES + [(1 << 256) - 1, 1 << 255, 2 * P - 1, 2 * P, (1 << 256) - (1 << 29)] + [rng.randrange(1 << 256) for _ in range(3000)]
    for v in vals:
        x = unpack29(words(v))
        assert x == norm(v) and x[8] < 1 << 24
        assert pack29(x) == words(v)
    print("ok: unpack29 / pack29 are exact inverses on %d values below 2^256 (limb edges included)" % len(vals))


def check_qnorm(rng):
    full = (1 << 32) - 1
    cases = [[full] * 8 + [full - 7], [0] * L, [MASK] * L, [1 << W] * L, [full] * 8 + [0]]
    cases += [[rng.randrange(1 << 32) for _ in range(8)] + [rng.randrange((1 << 32) - 7)] for _ in range(3000)]
    cases += [lazify(norm(v), lambda i: 7) for v in EDGES]
    for a in cases:
        qnorm(a)
    # the top limb absorbs the carry of limb 7 without a mask: it has to leave room for it
    try:
        qnorm([full] * L)
        raise SystemExit("f29_qnorm holds with a full top limb after all: tighten this check")
    except AssertionError:
        pass
    print("ok: f29_qnorm keeps the value and leaves limbs < 2^29 + 8 for limbs < 2^32, top limb <= 2^32 - 8 (%d cases)" % len(cases))


def check_reduce(rng):
    cases, qmax = [], (RP - 1) // P
    offs = [0, 1, 2, 3, 1 << 28, 1 << 29, 1 << 203, 1 << 229, (1 << 229) + 1, (1 << 230), (1 << 232) - 1]
    for m in range(qmax + 2):
        for d in offs:
            for v in (m * P + d, m * P - d):
                if 0 <= v < RP:
                    cases.append(v)
    cases += [RP - 1 - d for d in range(64)] + [RP - (1 << s) for s in range(1, 261, 7)]
    cases += [v for v in EDGES] + [rng.randrange(RP) for _ in range(3000)]
    n = 0
    for v in cases:
        for a in (norm(v), lazify(norm(v), lambda i: 7), lazify(norm(v), lambda i: rng.randrange(8))):
            assert value(a) == v
            r = reduce_2p(a)
            c = canon(a)
            assert value(c) == v % P and value(r) % P == v % P
            n += 1
    print("ok: f29_reduce_2p in [0, 2p) with q = floor(V/p) or one less, f29_canon in [0, p), on %d lazy values across [0, 2^261)" % n)


def check_montmul(rng):
    amax, atop = (5 << 29) - 1, (1 << 31) - 1                         # limbs < 1.25 * 2^31, top limb < 2^31
    # the column bound, every limb of both operands at its maximum (b is not below p here: only the 64-bit fit is meant)
    montmul([amax] * 8 + [atop], [MASK] * L, check=False)
    bs = [norm(v) for v in EDGES] + [norm(rng.randrange(P)) for _ in range(40)]
    lazy_as = [[amax] * 8 + [atop], [amax] * 8 + [0], [0] * 8 + [atop], norm(32 * P - 1), lazify(norm(32 * P - 1), lambda i: 4),
               lazify(norm(RP - 1), lambda i: 4)]
    n = 0
    for a in lazy_as + [norm(v) for v in EDGES]:
        for b in bs:
            t = montmul(a, b)
            if value(a) < 32 * P:
                assert value(t) * 5 < 6 * P                           # the header's "< 1.2 p for value(a) < 32 p"
            n += 1
    assert 160 * P < RP                                               # ... which is 32 p * p / 2^261 < 0.2 p
    for _ in range(4000):
        a = [rng.randrange(amax + 1) for _ in range(8)] + [rng.randrange(atop + 1)]
        montmul(a, norm(rng.randrange(P)))
        n += 1
    # b need not be below p (the division kernel multiplies two products, each < 1.2 p): normalised limbs are what the columns need
    for _ in range(500):
        a, b = norm(rng.randrange(P + P // 5)), norm(rng.randrange(P + P // 5))
        assert value(montmul(a, b)) * 100 < 101 * P
        n += 1
    # conversions: x * R'^2 / R' = x R' (Montgomery form), 1 in Montgomery form
    assert value(canon(montmul(norm(1), K["F29_R2"]))) == RP % P == value(K["F29_ONE_M"])
    print("ok: f29_montmul exact, normalised, < a*b/2^261 + p on %d products; every column fits 64 bits with all limbs at their maximum" % n)


def check_accumulation():
    """the lazy sums of k_rlc_partial / k_encode_out_dot[_z] / k_sum_elems (renormalised every 6 terms) and k_rlc_combine (every 4),
    with every term at the largest normalised value a product can have"""
    t_all = norm(T_ALLONES)                                           # all-ones low limbs, < p
    t_12 = [MASK] * 8 + [(P + P // 5) >> 232]                         # the bound of a product: limbs all ones, value ~ 1.2p
    for term, group in ((t_all, 128), (t_12, 128)):
        a, since = [0] * L, 0
        for _ in range(group):
            a = [u32(x + y) for x, y in zip(a, term)]
            since += 1
            if since == 6:
                a, since = qnorm(a), 0
        assert value(a) == group * value(term) < RP
        v = montmul(qnorm(a), K["F29_R2"])                            # back to a plain value
        # NOT "< 1.2p" (that holds for a < 32p only): < p + group * 1.2p * p / 2^261, which is < 2p up to group = 128 --
        # what k_rlc_combine and the accumulate path (v + a partial < 2p, then f29_reduce_2p) need
        assert value(v) < 2 * P and value(v) % P == group * value(term) * RP % P
        reduce_2p([u32(x + y) for x, y in zip(v, norm(2 * P - 1))])
    assert 7 * MASK + (1 << W) + 7 >= 1 << 32                         # ... and 6 is the longest interval: a 7th all-ones term overflows
    # k_rlc_combine: partials < 2p, normalised, f29_qnorm every 4, up to 64 groups (+ 1 for the accumulator)
    part = [MASK] * 8 + [(2 * P) >> 232]
    a = norm(P - 1)
    for g in range(64):
        a = [u32(x + y) for x, y in zip(a, part)]
        if g & 3 == 3:
            a = qnorm(a)
    canon(qnorm(a))
    print("ok: lazy sums of 128 all-ones products (renormalised every 6) and of 64 partials (every 4) stay in 32-bit limbs and below 2^261")


def main():
    rng = random.Random(29)
    check_constants()
    check_pack(rng)
    check_sub_k(rng)
    check_qnorm(rng)
    check_reduce(rng)
    check_montmul(rng)
    check_accumulation()
    print("ok: all checks passed")


if __name__ == "__main__":
    main()
