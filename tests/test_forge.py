"""CPU: the forging prover of tests/forge.py is right before a GPU is involved.

For every forged envelope the predicates stated in Python integers (forge.Forger.model / model_envelope) equal the vector the
forgery was built for, the oracle's restated verifier rejects it where it has a check for it, and the searches end within
their caps.  tests/test_gpu_verifier_predicates.py then asks the HIP verifier for the same vectors.
"""
import numpy as np
import pytest

import forge

SHAPES = [(320, 512, 2048, 640, 330), (832, 1024, 4096, 2000, 900)]
IDS = ["k%d" % s[1] for s in SHAPES]


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def fg(request):
    return forge.forger(*request.param)


def test_round_trip_is_byte_identical(fg):
    """the matrix rebuilt from lo_form_rows hashes to the proof's root, and the envelope assembled around the honest
    polynomials is lo_prove's, byte for byte; the model accepts it"""
    assert fg.rebuilt_root == fg.root == fg.env.root
    envelope, idx = fg.assemble(fg.poly["code"], fg.poly["lin"], fg.poly["quad"])
    assert envelope == fg.honest
    assert [int(i) for i in idx] == fg.env.idx
    assert fg.matrix.shape == (fg.R + 3, fg.n, 8)
    assert forge.pb_write(fg.env.top) == fg.honest              # the writer inverts the reader
    assert fg.model_envelope(fg.honest) == forge.ACCEPTED
    assert fg.model(fg.poly["code"], fg.poly["lin"], fg.poly["quad"], idx) == dict.fromkeys(forge.FLAGS[3:9], 1)


def test_expected_vectors_are_the_table():
    """the expected vectors written out once, so that a slip in forge.expect cannot move both sides of a comparison"""
    e = forge.expect
    #                                                  parsed idx merkle vcode vlin vquad ceq leq qeq accept
    assert e("valid_code") ==                          (1, 1, 1, 0, 1, 1, 1, 1, 1, 0)
    assert e("code_equal") ==                          (1, 1, 1, 1, 1, 1, 0, 1, 1, 0)
    assert e("valid_linear") ==                        (1, 1, 1, 1, 0, 1, 1, 1, 1, 0)
    assert e("linear_equal") ==                        (1, 1, 1, 1, 1, 1, 1, 0, 1, 0)
    assert e("valid_quad") ==                          (1, 1, 1, 1, 1, 0, 1, 1, 1, 0)
    assert e("quad_equal") ==                          (1, 1, 1, 1, 1, 1, 1, 1, 0, 0)
    assert e("valid_merkle") ==                        (1, 1, 0, 1, 1, 1, 1, 1, 1, 0)
    assert e("valid_quad", "quad_equal") ==            (1, 1, 1, 1, 1, 0, 1, 1, 0, 0)
    assert forge.STOPS_AT_INDICES ==                   (1, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert forge.STOPS_AT_PARSE ==                     (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("name", forge.NAMES)
def test_forgery_fails_what_it_was_built_to_fail(fg, name):
    f = fg.forgeries()[name]
    want = {
        "code_degree": forge.expect("valid_code"), "code_equal": forge.expect("code_equal"),
        "lin_sum": forge.expect("valid_linear"), "lin_equal": forge.expect("linear_equal"),
        "quad_slots": forge.expect("valid_quad"), "quad_equal": forge.expect("quad_equal"),
        "code_coef_first": forge.expect("valid_code", "code_equal"), "code_coef_last": forge.expect("valid_code", "code_equal"),
        "lin_slot_last": forge.expect("valid_linear"), "quad_slot_last": forge.expect("valid_quad"),
        "code_spike_opened_first": forge.expect("valid_code", "code_equal"), "code_spike_opened_last": forge.expect("valid_code", "code_equal"),
        "lin_spike_opened_first": forge.expect("valid_linear", "linear_equal"), "lin_spike_opened_last": forge.expect("valid_linear", "linear_equal"),
        "quad_spike_opened_first": forge.expect("valid_quad", "quad_equal"), "quad_spike_opened_last": forge.expect("valid_quad", "quad_equal"),
        "sibling_flipped": forge.expect("valid_merkle"), "sibling_dropped": forge.expect("valid_merkle"), "sibling_appended": forge.expect("valid_merkle"),
        "indices_swapped": forge.STOPS_AT_INDICES, "index_duplicated": forge.STOPS_AT_INDICES,
        "noncanonical_code": forge.STOPS_AT_PARSE, "noncanonical_sample": forge.STOPS_AT_PARSE, "meta_k_doubled": forge.STOPS_AT_PARSE,
    }[name]
    assert f.expected == want
    assert f.envelope != fg.honest
    assert fg.model_envelope(f.envelope) == want
    if f.polys is not None:
        # the polynomial predicates alone, on the polynomials the forger holds (not re-read from the envelope)
        m = fg.model(*f.polys, f.idx)
        assert tuple(m[flag] for flag in forge.FLAGS[3:9]) == want[3:9]
    if f.oracle_rejects:
        assert fg.oracle_accepts(f.envelope) == 0
    else:
        assert name in ("noncanonical_code", "noncanonical_sample")      # the oracle has no canonical check: nothing is asserted about it


def test_spikes_sit_where_they_were_aimed(fg):
    """unopened spikes are on a column the forged transcript does not open; opened spikes are on its first / last sorted
    index, inside the 64 outermost columns; every polynomial of a forgery differs from the honest one in that column only"""
    F = fg.forgeries()
    which = {"code_degree": "code", "lin_sum": "lin", "quad_slots": "quad", "lin_slot_last": "lin", "quad_slot_last": "quad"}
    for name in forge.TABLE + forge.EDGES + forge.SPIKES:
        f = F[name]
        p = which.get(name, name.split("_")[0])
        at = forge.POLYS.index(p)
        changed = np.flatnonzero((f.polys[at] != fg.poly[p]).any(axis=1))
        assert all(f.polys[i] is fg.poly[q] for i, q in enumerate(forge.POLYS) if i != at), name
        if name in ("code_equal", "lin_equal", "quad_equal"):
            assert len(changed) > fg.n - fg.k, name                      # a nonzero codeword of degree < k has fewer than k zeros
            assert np.isin(f.idx, changed).any(), name
            continue
        if name in ("code_coef_first", "code_coef_last"):
            assert len(changed) == fg.n, name                            # a monomial vanishes nowhere
            continue
        assert len(changed) == 1, name
        j = int(changed[0])
        if name.endswith("slot_last"):
            assert j not in f.idx and j == 4 * (fg.k - fg.l + 1), name
        elif name in which:
            assert j not in f.idx and j < 2 * forge.UNOPENED_CAP, name
        elif name.endswith("first"):
            assert j == int(f.idx[0]) and j < 64, name
        else:
            assert j == int(f.idx[-1]) and j >= fg.n - 64, name


def test_edge_forgeries_touch_one_end_of_a_range(fg):
    """decode(forged - honest): code_coef_first / _last have the coefficient k / n - 1 alone among [k, n); lin_slot_last and
    quad_slot_last move the data slot l - 1 alone among the l data slots; lin_sum and quad_slots move slot 0 alone"""
    F = fg.forgeries()
    l, k, n = fg.l, fg.k, fg.n

    def decoded_delta(name, which):
        forged, honest = F[name].polys[forge.POLYS.index(which)], fg.poly[which]
        delta = [(a - b) % forge.P for a, b in zip(ol_ints(forged), ol_ints(honest))]
        return ol_ints(fg.ctx.decode(forge.ol.to_limbs(delta)))

    ol_ints = forge.ol.from_limbs
    for name, e in (("code_coef_first", k), ("code_coef_last", n - 1)):
        dec = decoded_delta(name, "code")
        assert [i for i in range(k, n) if dec[i]] == [e], name
    for name, which, slot in (("lin_slot_last", "lin", l - 1), ("quad_slot_last", "quad", l - 1), ("lin_sum", "lin", 0), ("quad_slots", "quad", 0)):
        dec = decoded_delta(name, which)
        assert [i for i in range(l) if dec[i]] == [slot], name


def test_searches_end_within_their_caps(fg):
    tries = fg.tries()
    assert set(tries) == {"code_degree", "lin_sum", "quad_slots", "lin_slot_last", "quad_slot_last", "noncanonical_code"} | set(forge.SPIKES)
    print("tries (l, k, n) = (%d, %d, %d): %s" % (fg.l, fg.k, fg.n, tries))
    for name, n_tries in tries.items():
        assert 1 <= n_tries <= (forge.SPIKE_CAP if name in forge.SPIKES else forge.UNOPENED_CAP), name


def test_spike_reaches_slots_rule(fg):
    """the rule that places lin / quad spikes, checked against the decode: a spike at a column = 2 mod 4, or on a pad slot's
    own column, leaves both slot predicates at 1; every other placement breaks them"""
    l, k, n = fg.l, fg.k, fg.n
    first_data = 4 * (k - l + 1)                                          # the column of slot l - 1; the one before it is slot l, a pad
    for j in (0, 1, 2, 3, 4, 5, 6, 60, first_data - 4, first_data, n - 4, n - 3, n - 2, n - 1):
        for which in ("lin", "quad"):
            broken = fg._poly_pred(which, fg.add_at(fg.poly[which], j, 5)) == 0
            assert broken == fg.spike_reaches_slots(which, j), (which, j)
        assert fg._poly_pred("code", fg.add_at(fg.poly["code"], j, 5)) == 0
