"""CPU: the extremal input families (tests/extremal.py) are what they claim to be, and the oracle alone proves every trace the
GPU tests of tests/test_gpu_extremal_rows.py compare against it."""
import numpy as np
import pytest

import extremal as ex
import oracle_lib as ol

P = ol.P
MASK = (1 << 29) - 1


def limbs29(v):
    return [(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232]


@pytest.mark.parametrize("name", ex.FAMILIES)
@pytest.mark.parametrize("count", [1, 5, 320, 513])
def test_every_family_is_canonical(name, count):
    a = ex.family(name, count, k=512, shift=3)
    assert a.shape == (count, 8) and a.dtype == np.uint32
    vals = ol.from_limbs(a)
    assert all(0 <= v < P for v in vals)
    want = {"zero": [0] * count, "one": [1] * count, "pm1": [P - 1] * count, "delta": [P - 1] + [0] * (count - 1),
            "alt": [(P - 1) * (1 - i % 2) for i in range(count)]}
    if name in want:
        assert vals == want[name]
    if name == "geom":
        g = ex.omega(512)
        assert vals == [(P - 1) * pow(g, i, P) % P for i in range(count)]


def test_limb_edges_hold_the_stated_values():
    v = ex.limb_edge_values()
    assert len(v) == 16 + 14 + 9 + 1 + 2 and len(set(v)) == len(v)
    assert all(0 < x < P for x in v)
    for i in range(1, 9):
        assert 1 << (29 * i) in v and (1 << (29 * i)) - 1 in v
        assert limbs29((1 << (29 * i)) - 1)[:i] == [MASK] * i
    for i in range(1, 8):
        assert 1 << (32 * i) in v and (1 << (32 * i)) - 1 in v
    for i in range(9):
        assert P - (1 << (29 * i)) in v
    top = ((P >> 232) << 232) - 1
    assert top in v and limbs29(top) == [MASK] * 8 + [(P >> 232) - 1]
    assert (P - 1) // 2 in v and (P + 1) // 2 in v and (P - 1) // 2 + (P + 1) // 2 == P
    # the cyclic vector visits every value, from any shift
    got = set(ol.from_limbs(ex.family("limb_edges", len(v), shift=11)))
    assert got == set(v)


@pytest.mark.parametrize("plain", [False, True])
def test_allones_products_identities(plain):
    T = ex.T_ALLONES
    assert T < P and limbs29(T) == [MASK] * 8 + [(P >> 232) - 1]
    u, r = ex.allones_products(300, np.random.default_rng(1), plain=plain)
    U, Rr = ol.from_limbs(u), ol.from_limbs(r)
    assert all(0 < a < P and 0 <= b < P for a, b in zip(U, Rr))
    rinv = pow(ex.RP, -1, P)
    for a, b in zip(U, Rr):
        if plain:
            assert a * b % P == T
        else:
            assert a * b * rinv % P == T
            # the device's Montgomery product is (a*b + m*p) / R' with m < R': the representative in [ab/R', ab/R' + p)
            m = (-a * b * pow(P, -1, ex.RP)) % ex.RP
            assert (a * b + m * P) % ex.RP == 0 and (a * b + m * P) // ex.RP == T
    # the oracle's own Montgomery product (radix 2^256) of u and r * 2^-5 agrees: independent of the Python above
    if not plain:
        r5 = ex.limbs([b * pow(32, -1, P) % P for b in Rr[:8]])
        out = np.zeros((8, 8), dtype=np.uint32)
        for i in range(8):
            ol.lib().lo_fr_montmul(ol.ptr(out[i:i + 1]), ol.ptr(u[i:i + 1]), ol.ptr(r5[i:i + 1]))
        assert ol.from_limbs(out) == [T] * 8


def test_trace_layout():
    l, k, n = ex.SMALL
    kinds, rows, masks, rands = ex.build_extremal_trace(l, k, n, 130, 2, "mixed")
    assert len(kinds) == 136 and rows.shape == rands.shape == (136, k, 8)
    assert [m.shape[0] for m in masks] == [k, 2 * k, 2 * k]
    assert not rands[:, l:].any()                                   # randomness is zero outside the data slots
    assert all(v < P for v in ol.from_limbs(rows.reshape(-1, 8))) and all(v < P for v in ol.from_limbs(rands.reshape(-1, 8)))
    tri = np.flatnonzero(kinds == 1)
    assert len(tri) == 2
    for r in tri:
        assert list(kinds[r:r + 3]) == [1, 2, 3]
        x, y, z = (ol.from_limbs(rows[r + d]) for d in range(3))
        assert z == [a * b % P for a, b in zip(x, y)]               # over all k slots
    # mixed cycles the families row by row; pads are the family's, not the oracle's draws
    assert ol.from_limbs(rows[0]) == [P - 1] * k and not rows[1].any() and ol.from_limbs(rows[7]) == [1] * k
    r = 6                                                            # an allones_products row: data slot x randomness = T
    assert ex.MIXED_CYCLE[r] == "allones_products"
    rinv = pow(ex.RP, -1, P)
    assert all(a * b * rinv % P == ex.T_ALLONES for a, b in zip(ol.from_limbs(rows[r, :l]), ol.from_limbs(rands[r, :l])))
    kinds, rows, _, rands = ex.build_extremal_trace(l, k, n, 130, 2, "pm1")
    assert ol.from_limbs(rows[kinds != 3].reshape(-1, 8)) == [P - 1] * (134 * k)
    assert ol.from_limbs(rows[kinds == 3].reshape(-1, 8)) == [1] * (2 * k)        # z = (p - 1)^2
    assert ol.from_limbs(rands[:, :l].reshape(-1, 8)) == [P - 1] * (136 * l)


@pytest.mark.parametrize("case", ex.ALL_TRACES, ids=lambda c: "-".join(str(x) for x in c))
def test_oracle_alone_proves_every_extremal_trace(case):
    """the reference side handles these inputs: lo_prove_rows accepts the stream and returns an envelope.  Its valid flags are
    whatever it says (the GPU tests compare against them); for rows that satisfy z = x * y slot by slot, with the linear constant
    derived from the rows, they are all set."""
    want = ex.oracle_proof(*case)
    assert len(want["proof"]) > 3 * 32 * case[2] and want["rows"] == case[3] + 3 * case[4] + 3
    assert len(want["root"]) == 32 and want["root"] != bytes(32)
    assert all(v in (0, 1) for v in want["valid"])
    assert int.from_bytes(want["const_sum"], "little") < P
