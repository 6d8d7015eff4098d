"""GPU: every acceptance predicate of the HIP verifier is seen to return 0, alone.

tests/forge.py builds envelopes that are well formed and consistent after the forgery (the transcript is re-derived), so that
each fails exactly the predicate it was built to fail; tests/test_forge.py proves that on the CPU.  Here lig_synth_verify and
lig_rows_verify_begin / _finish must return the same full vector [parsed, indices_match, valid_merkle, valid_code,
valid_linear, valid_quad, code_equal, linear_equal, quad_equal, accept] -- never just accept = 0.
"""
import numpy as np
import pytest

import forge
import hip_lib
import oracle_lib as ol

pytestmark = pytest.mark.gpu

SHAPES = [
    (320, 512, 2048, 640, 330),
    (832, 1024, 4096, 2000, 900),                              # tile length 128, the extra radix-2 stage in the decode
    (8000, 8192, 32768, 2 * 8000 + 123, 8000 + 5),             # the production packing
]
IDS = ["k%d" % s[1] for s in SHAPES]
K512 = SHAPES[0]


@pytest.fixture(scope="module")
def amd():
    return hip_lib.load()


class Bench:
    """one shape: its forger, a context, the library's job and the honest envelope proved by the library"""

    def __init__(self, amd, shape):
        l, k, n, n_linear, n_quad = shape
        self.fg = forge.forger(*shape)
        self.c = amd.Context(l, k, n)
        self.job = amd.Context.make_job(n_linear, n_quad, generated_at=99)
        tr = self.c.synth_prepare_job(self.job)
        try:
            self.proof, self.info = self.c.synth_prove(tr)
        finally:
            self.c.trace_destroy(tr)
        self.F = self.fg.forgeries()

    def verify(self, envelope, const_sum="given"):
        return forge.vector(self.c.synth_verify(self.job, self.fg.const_sum if const_sum == "given" else const_sum, envelope))


@pytest.fixture(scope="module")
def benches(amd):
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = Bench(amd, shape)
        return made[shape]

    yield get
    for b in made.values():
        b.c.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_honest_envelope_is_the_provers_and_is_accepted(benches, shape):
    b = benches(shape)
    assert b.proof == b.fg.honest                              # synth_prove's envelope is the one the forger starts from
    assert bytes(b.info.const_sum) == b.fg.const_sum and bytes(b.info.root) == b.fg.root
    assert b.verify(b.fg.honest) == forge.ACCEPTED
    assert b.verify(b.fg.honest, const_sum=None) == forge.ACCEPTED


@pytest.mark.parametrize("name", forge.NAMES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_synth_verify_fails_exactly_the_forged_predicate(benches, shape, name):
    b = benches(shape)
    f = b.F[name]
    got = b.verify(f.envelope)
    print("%s %s: got %s, expected %s" % (IDS[SHAPES.index(shape)], name, got, f.expected))
    assert got == f.expected


@pytest.mark.parametrize("name", ["lin_sum", "lin_equal"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_derived_constant_gives_the_same_vector(benches, shape, name):
    """lig_synth_verify(job, NULL, ...): the constant of the linear test derived from the public statement"""
    b = benches(shape)
    assert b.verify(b.F[name].envelope, const_sum=None) == b.F[name].expected


@pytest.fixture(scope="module")
def rows_side(benches):
    """the verifier's side of the k = 512 job as a rows job: kinds, the driver's randomness rows (host and device) and constant"""
    b = benches(K512)
    kinds = ol.row_kinds(b.fg.job)
    rands, const_sum = ol.rand_rows(b.fg.job, b.fg.seed1)
    assert const_sum == b.fg.const_sum
    d_rands = b.c.upload(rands)
    yield b, kinds, rands, d_rands, const_sum
    b.c.free(d_rands)


@pytest.mark.parametrize("where", ["host_rands", "device_rands"])
@pytest.mark.parametrize("name", ("honest",) + forge.TABLE)
def test_rows_verify_gives_the_same_vector(rows_side, name, where):
    b, kinds, rands, d_rands, const_sum = rows_side
    envelope, expected = (b.fg.honest, forge.ACCEPTED) if name == "honest" else (b.F[name].envelope, b.F[name].expected)
    vt, seed1, begun = b.c.rows_verify_begin(kinds, envelope)
    assert vt is not None and seed1 == b.fg.seed1              # the root is the honest one in every table forgery
    assert (begun.parsed, begun.indices_match) == (1, 1)
    on_device = where == "device_rands"
    got = forge.vector(b.c.rows_verify_finish(vt, d_rands if on_device else rands, const_sum, on_device=on_device))
    assert got == expected


@pytest.mark.parametrize("name", forge.INDEX_LIST + forge.UNPARSED)
def test_rows_verify_begin_returns_no_trace(rows_side, name):
    b, kinds = rows_side[0], rows_side[1]
    vt, _, begun = b.c.rows_verify_begin(kinds, b.F[name].envelope)
    assert vt is None
    assert forge.vector(begun) == b.F[name].expected


def test_workspace_reuse_keeps_accepting_the_honest_envelope(amd):
    """the verifier reuses its device buffers between calls: a rejected envelope leaves nothing behind that the next call reads"""
    l, k, n = K512[:3]
    fg = forge.forger(*K512)
    F = fg.forgeries()
    c = amd.Context(l, k, n)
    try:
        job = amd.Context.make_job(K512[3], K512[4], generated_at=99)
        verify = lambda envelope: forge.vector(c.synth_verify(job, fg.const_sum, envelope))
        assert verify(fg.honest) == forge.ACCEPTED
        assert verify(F["code_degree"].envelope) == F["code_degree"].expected
        assert verify(fg.honest) == forge.ACCEPTED
        c.verify_release()
        assert verify(F["quad_equal"].envelope) == F["quad_equal"].expected
        assert verify(fg.honest) == forge.ACCEPTED
    finally:
        c.close()
