"""A forging prover over the CPU oracle (test kit): envelopes that break exactly one acceptance predicate of the verifier.

The verifier re-derives the stage-2 seed from the root and the three polynomials of the envelope, so a byte changed inside a
polynomial moves the sampled columns and the verification ends at `indices_match`.  A forger that wants to reach a predicate
has to re-derive the transcript after the forgery: new seed, new columns, their opened elements and sibling hashes from the
committed matrix.  This module rebuilds that matrix on the CPU (lo_form_rows -> encode -> column hash -> Merkle tree, the
root must be the proof's), re-assembles an envelope around any three polynomials, and states in Python integers which
predicates such an envelope satisfies (`model`, `model_envelope`).

Every forgery is well formed or cleanly malformed input for a host parser.  The list in `Forger.forgeries` is the whole set.
"""
import ctypes as C
import functools
import hashlib

import numpy as np

import oracle_lib as ol
import pydef

P = ol.P
T = 192
FLAGS = ("parsed", "indices_match", "valid_merkle", "valid_code", "valid_linear", "valid_quad",
         "code_equal", "linear_equal", "quad_equal", "accept")
POLYS = ("code", "lin", "quad")
VALID = {"code": "valid_code", "lin": "valid_linear", "quad": "valid_quad"}
EQUAL = {"code": "code_equal", "lin": "linear_equal", "quad": "quad_equal"}
UNOPENED_CAP = 16             # tries for a column that the forged transcript does not open
SPIKE_CAP = 4096              # tries for a spike that lands on the first / last opened column

TABLE = ("code_degree", "code_equal", "lin_sum", "lin_equal", "quad_slots", "quad_equal")
EDGES = ("code_coef_first", "code_coef_last", "lin_slot_last", "quad_slot_last")      # the ends of the ranges that self_check reads
SPIKES = tuple("%s_spike_opened_%s" % (p, e) for p in POLYS for e in ("first", "last"))
MERKLE = ("sibling_flipped", "sibling_dropped", "sibling_appended")
INDEX_LIST = ("indices_swapped", "index_duplicated")
UNPARSED = ("noncanonical_code", "noncanonical_sample", "meta_k_doubled")
NAMES = TABLE + EDGES + SPIKES + MERKLE + INDEX_LIST + UNPARSED


def expect(*zero):
    """the vector of FLAGS with the named predicates (and accept) at 0"""
    return tuple(0 if (f in zero or f == "accept") else 1 for f in FLAGS)


ACCEPTED = (1,) * len(FLAGS)
STOPS_AT_INDICES = (1,) + (0,) * (len(FLAGS) - 1)      # the verifier returns before it evaluates a predicate
STOPS_AT_PARSE = (0,) * len(FLAGS)


def vector(info):
    """a VerifyInfo of the library as the tuple of FLAGS"""
    return tuple(int(getattr(info, f)) for f in FLAGS)


# ---- protobuf wire writer, the counterpart of pydef.pb_fields
def _varint(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _field(f, wt, v):
    tag = _varint(f << 3 | wt)
    if wt == 0:
        return tag + _varint(v)
    if wt == 2:
        return tag + _varint(len(v)) + v
    return tag + v                                     # fixed32 / fixed64: the raw bytes


def pb_write(fields):
    return b"".join(_field(*x) for x in fields)


def _one(fields, f):
    vals = [v for g, _, v in fields if g == f]
    assert len(vals) == 1, "field %d appears %d times" % (f, len(vals))
    return vals[0]


class Envelope:
    """the parts of a proof envelope the verifier reads (proto/ligero_proof.proto restated in pydef / oracle)"""

    def __init__(self, b):
        self.top = pydef.pb_fields(b)
        self.meta = pydef.pb_fields(_one(self.top, 1))
        self.k, self.n, self.t = (_one(self.meta, f) for f in (6, 7, 8))
        body = pydef.pb_fields(_one(self.top, 2))
        assert all(wt == 2 for _, wt, _ in body)
        self.merkle = pydef.pb_fields(_one(body, 1))
        self.root = _one(pydef.pb_fields(_one(self.merkle, 2)), 1)
        self.sib = [_one(pydef.pb_fields(v), 1) for f, _, v in self.merkle if f == 3]
        packed, self.idx = _one(self.merkle, 4), []
        i = 0
        while i < len(packed):
            v, i = pydef._varint(packed, i)
            self.idx.append(v)
        self.code, self.lin, self.quad, self.samples = (_one(pydef.pb_fields(_one(body, f)), 1) for f in (2, 3, 4, 5))


class Forgery:
    def __init__(self, name, envelope, expected, oracle_rejects, tries=None, polys=None, idx=None):
        self.name, self.envelope, self.expected, self.oracle_rejects, self.tries = name, envelope, expected, oracle_rejects, tries
        self.polys, self.idx = polys, idx              # the three polynomials and the opened columns, where `model` applies

    def __repr__(self):
        return "Forgery(%s)" % self.name


def _ints(arr):
    return ol.from_limbs(arr)


def _elem(v):
    return ol.to_limbs([v])[0]


class Forger:
    def __init__(self, l, k, n, n_linear, n_quad, generated_at=99, threads=8):
        self.l, self.k, self.n, self.t = l, k, n, T
        self.job = ol.make_job(l, k, n, T, n_linear, n_quad, generated_at=generated_at, threads=threads)
        pr = ol.Proof()
        assert ol.lib().lo_prove(C.byref(self.job), C.byref(pr)) == 0
        try:
            self.honest = bytes(pr.proof[:pr.proof_len])
            self.root, self.seed1, self.const_sum = bytes(pr.root), bytes(pr.stage1_seed), bytes(pr.const_sum)
            assert (pr.valid_code, pr.valid_linear, pr.valid_quad) == (1, 1, 1)
        finally:
            ol.lib().lo_proof_free(C.byref(pr))
        self.cs = int.from_bytes(self.const_sum, "little")
        assert self.oracle_accepts(self.honest) == 1
        env = Envelope(self.honest)
        assert (env.k, env.n, env.t) == (k, n, T) and env.root == self.root
        self.env = env
        # ---- the committed matrix: message rows and the three masks, encoded; its column hashes and Merkle tree
        self.ctx = ol.Ctx(l, k, n)
        rows, mc, ml, mq = ol.form_rows(self.job)
        self.R = rows.shape[0]
        masks = np.stack([self.ctx.encode(mc), self.ctx.encode_2k(ml), self.ctx.encode_2k(mq)])
        self.matrix = np.concatenate([self.ctx.encode_rows(rows, threads=threads), masks]) if self.R else masks
        self.nodes = ol.merkle_build(ol.colsha(self.matrix))
        self.rebuilt_root = self.nodes[0].tobytes()
        assert self.rebuilt_root == self.root, "the matrix rebuilt from lo_form_rows does not hash to the proof's root"
        self.poly = {p: np.frombuffer(getattr(env, p), dtype=np.uint32).reshape(n, 8).copy() for p in POLYS}
        self.H = {p: _ints(self.poly[p]) for p in POLYS}       # honest polynomials = the true combinations of the matrix
        self._pred = {}
        self._forgeries = None

    # ---- the oracle's restated verifier
    def oracle_accepts(self, envelope, const_sum=None):
        cs = (C.c_uint64 * 4).from_buffer_copy(self.const_sum if const_sum is None else bytes(const_sum))
        buf = (C.c_uint8 * len(envelope)).from_buffer_copy(envelope)
        return ol.lib().lo_verify(C.byref(self.job), cs, buf, len(envelope))

    # ---- transcript
    def stage2_seed(self, code, lin, quad):
        out = np.zeros(32, np.uint8)
        root = np.frombuffer(self.root, dtype=np.uint8).copy()
        ol.lib().lo_stage2_seed(ol.ptr(root), *[ol.ptr(np.ascontiguousarray(a, dtype=np.uint32)) for a in (code, lin, quad)], self.n, ol.ptr(out))
        return out.tobytes()

    def indices(self, seed2):
        idx = ol.sample_indices(seed2, self.n, self.t)
        assert np.all(idx[1:] > idx[:-1]), "the sampled columns are sorted and distinct"
        return idx

    def pack(self, code, lin, quad, idx, sib, samples, meta_k=None):
        """an envelope with the honest one's metadata around the given parts"""
        env = self.env
        merkle = [x for x in env.merkle if x[0] not in (3, 4)]
        merkle += [(3, 2, _field(1, 2, bytes(d))) for d in sib]
        merkle.append((4, 2, b"".join(_varint(int(i)) for i in idx)))
        body = [(1, 2, pb_write(merkle))] + [(f, 2, _field(1, 2, bytes(v))) for f, v in ((2, code), (3, lin), (4, quad), (5, samples))]
        meta = [(f, wt, (meta_k if (f == 6 and meta_k is not None) else v)) for f, wt, v in env.meta]
        return pb_write([(f, wt, (pb_write(meta) if f == 1 else pb_write(body) if f == 2 else v)) for f, wt, v in env.top])

    def parts(self, code, lin, quad):
        """the transcript an honest prover's stage 3 writes around these three polynomials"""
        idx = self.indices(self.stage2_seed(code, lin, quad))
        sib = [d.tobytes() for d in ol.merkle_decommit(self.nodes, self.n, idx)]
        samples = np.ascontiguousarray(self.matrix[:, idx])
        return dict(code=code.tobytes(), lin=lin.tobytes(), quad=quad.tobytes(), idx=[int(i) for i in idx], sib=sib, samples=samples.tobytes())

    def assemble(self, code, lin, quad):
        """-> (envelope bytes, sorted indices)"""
        p = self.parts(code, lin, quad)
        return self.pack(**p), np.array(p["idx"], dtype=np.uint32)

    # ---- the predicates in Python integers
    def _poly_pred(self, which, arr):
        key = (which, hashlib.sha256(arr.tobytes()).digest())
        if key not in self._pred:
            dec = _ints(self.ctx.decode(arr))
            if which == "code":
                v = all(x == 0 for x in dec[self.k:self.n])
            elif which == "lin":
                v = (self.cs + sum(dec[:self.l])) % P == 0
            else:
                v = all(x == 0 for x in dec[:self.l])
            self._pred[key] = int(v)
        return self._pred[key]

    def model(self, code, lin, quad, idx):
        """the six polynomial predicates of an envelope assembled around (code, lin, quad) that opens the columns idx"""
        out = {}
        for which, arr in zip(POLYS, (code, lin, quad)):
            out[VALID[which]] = self._poly_pred(which, arr)
            got = _ints(arr[np.asarray(idx, dtype=np.int64)])
            out[EQUAL[which]] = int(all(g == self.H[which][int(j)] for g, j in zip(got, idx)))
        return out

    def model_envelope(self, envelope):
        """all of FLAGS for envelope bytes, in the order the verifier evaluates them.  The opened elements must be the
        committed ones: the *_equal predicates are then `the polynomial agrees with the honest one on the opened columns`."""
        n, t = self.n, self.t
        out = dict.fromkeys(FLAGS, 0)
        done = lambda: tuple(out[f] for f in FLAGS)
        try:
            env = Envelope(envelope)
        except (AssertionError, IndexError, ValueError):
            return done()
        if (env.k, env.n, env.t) != (self.k, n, t) or len(env.idx) != t or any(len(d) != 32 for d in env.sib):
            return done()
        if any(len(b) != 32 * n for b in (env.code, env.lin, env.quad)) or len(env.samples) != 32 * (self.R + 3) * t:
            return done()
        polys = [np.frombuffer(b, dtype=np.uint32).reshape(n, 8) for b in (env.code, env.lin, env.quad)]
        samples = np.frombuffer(env.samples, dtype=np.uint32).reshape(self.R + 3, t, 8)
        if any(v >= P for a in polys + [samples] for v in _ints(a)):
            return done()
        out["parsed"] = 1
        idx = self.indices(self.stage2_seed(*polys))
        out["indices_match"] = int([int(i) for i in idx] == env.idx)
        if not out["indices_match"]:
            return done()
        assert np.array_equal(samples, self.matrix[:, idx]), "model_envelope: the opened elements are not the committed ones"
        leaves = ol.colsha(samples)
        sib = np.frombuffer(b"".join(env.sib) or bytes(32), dtype=np.uint8).copy()
        vroot = np.zeros(32, np.uint8)
        ok = ol.lib().lo_merkle_recommit(n, ol.ptr(idx), t, ol.ptr(leaves), ol.ptr(sib), len(env.sib), ol.ptr(vroot))
        out["valid_merkle"] = int(bool(ok) and vroot.tobytes() == env.root)
        out.update(self.model(*polys, idx))
        out["accept"] = int(all(out[f] for f in FLAGS[2:9]))
        return done()

    # ---- deltas
    def add_at(self, arr, j, v):
        q = arr.copy()
        q[j] = _elem((_ints(arr[j:j + 1])[0] + v) % P)
        return q

    def add_vec(self, arr, delta):
        return ol.to_limbs([(a + d) % P for a, d in zip(_ints(arr), delta)])

    def enc(self, d):
        """Enc(d): the codeword of a length-k message given as {slot: value}; degree < k, decode(Enc(d)) = d || 0"""
        msg = np.zeros((self.k, 8), np.uint32)
        for i, v in d.items():
            msg[i] = _elem(v % P)
        return _ints(self.ctx.encode(msg))

    def _with(self, which, arr):
        return [arr if p == which else self.poly[p] for p in POLYS]

    def spike_reaches_slots(self, which, j):
        """whether a spike at column j moves the decoded slots that valid_linear / valid_quad read.
        The spike v e_j has the coefficients c_i = (v / n) w^(-ij), w = omega_4k, all of them nonzero, so it always breaks the
        degree test of the code polynomial.  The decode keeps c_i + c_(i+k) for i < k and drops the coefficients from 2k on
        (SURVEY.md A.2); here that is c_i (1 + w^(-kj)) with w^k a primitive 4th root of unity, and slot s becomes
        (v / n)(1 + w^(-kj)) sum_(i<k) w^(-i (4s + j)), the slots being read at omega_k^(-s):
          j = 2 mod 4: 1 + w^(-kj) = 0, no slot moves, and only the comparison on the opened columns can see the spike;
          j = 0 mod 4: only slot s = (k - j / 4) mod k moves, which the two predicates read when it is a data slot (s < l);
          j odd:       every slot moves.
        A spike on a linear or quadratic polynomial is therefore placed where it reaches a data slot
        (tests/test_forge.py checks this rule against the decode)."""
        return which == "code" or j % 2 == 1 or (j % 4 == 0 and (self.k - j // 4) % self.k < self.l)

    def spike_unopened(self, which, column=None):
        """poly + v at a column that the forged transcript does not open -> (polys, envelope, idx, tries).
        column=None: v = 1 at the first of the columns j = 0, 1, 2, ... (those from which the spike reaches a data slot) that
        stays unopened; column 0 moves data slot 0 alone.  A given column: v = 1, 2, 3, ... there until it stays unopened."""
        if column is None:
            candidates = [(j, 1) for j in range(2 * UNOPENED_CAP) if self.spike_reaches_slots(which, j)][:UNOPENED_CAP]
        else:
            candidates = [(column, v) for v in range(1, UNOPENED_CAP + 1)]
        for tries, (j, v) in enumerate(candidates, 1):
            polys = self._with(which, self.add_at(self.poly[which], j, v))
            envelope, idx = self.assemble(*polys)
            if j not in idx:
                return polys, envelope, idx, tries
        raise AssertionError("%s: no unopened column within %d tries" % (which, UNOPENED_CAP))

    def spike_opened(self, which, end):
        """poly + v at a column that the forged transcript opens as its first (end = 'first') or last sorted index.
        v runs over 1..64 and, for each v, the column over those of the 64 outermost columns of that end from which the spike
        reaches a data slot (spike_reaches_slots; columns left out are not counted as tries); only the seed and the
        sample are recomputed per try (hashlib, checked against the oracle's seed when the envelope is assembled)."""
        n, raw = self.n, {p: self.poly[p].tobytes() for p in POLYS}
        at = POLYS.index(which)
        pre = hashlib.sha256(b"LigetronStage2\0" + self.root + b"".join(raw[p] for p in POLYS[:at]))
        post = b"".join(raw[p] for p in POLYS[at + 1:])
        mine = memoryview(raw[which])
        cols = [j for j in (range(64) if end == "first" else range(n - 1, n - 65, -1)) if self.spike_reaches_slots(which, j)]
        candidates = [(v, j) for v in range(1, 65) for j in cols][:SPIKE_CAP]
        for tries, (v, j) in enumerate(candidates, 1):
            h = pre.copy()
            h.update(mine[:32 * j])
            h.update(((self.H[which][j] + v) % P).to_bytes(32, "little"))
            h.update(mine[32 * j + 32:])
            h.update(post)
            idx = self.indices(h.digest())
            if int(idx[0] if end == "first" else idx[-1]) == j:
                polys = self._with(which, self.add_at(self.poly[which], j, v))
                envelope, idx2 = self.assemble(*polys)
                assert np.array_equal(idx, idx2), "the hashlib seed and the oracle's seed disagree"
                return polys, envelope, idx2, tries
        raise AssertionError("%s: no spike on the %s opened column within %d tries" % (which, end, SPIKE_CAP))

    # ---- the whole set
    def forgeries(self):
        """-> {name: Forgery} for NAMES, in that order; computed once"""
        if self._forgeries is not None:
            return self._forgeries
        l, k, n, t = self.l, self.k, self.n, self.t
        F = {}

        def put(name, envelope, expected, oracle_rejects=True, **kw):
            F[name] = Forgery(name, envelope, expected, oracle_rejects, **kw)

        # the table: one polynomial + a delta, the transcript re-derived
        d01 = {0: 1, 1: P - 1}                                 # slots sum to 0 over the l data slots
        deltas = {"code_equal": ("code", d01), "lin_equal": ("lin", d01), "quad_equal": ("quad", {l: 7})}      # slot l: a pad slot
        spikes = {"code_degree": "code", "lin_sum": "lin", "quad_slots": "quad"}
        for name in TABLE:
            if name in spikes:
                which = spikes[name]
                polys, envelope, idx, tries = self.spike_unopened(which)
                put(name, envelope, expect(VALID[which]), tries=tries, polys=polys, idx=idx)
            else:
                which, d = deltas[name]
                delta = self.enc(d)
                polys = self._with(which, self.add_vec(self.poly[which], delta))
                envelope, idx = self.assemble(*polys)
                assert any(delta[int(j)] for j in idx), "%s: the delta vanishes on every opened column" % name
                put(name, envelope, expect(EQUAL[which]), polys=polys, idx=idx)
        # the ends of the ranges self_check reads.  A spike has every coefficient nonzero and, from column 0 or an odd column,
        # moves slot 0 or every slot; these four touch the first and the last coefficient of the degree test alone (the
        # monomials x^k and x^(n-1): never zero on a column, so code_equal goes with them) and the last data slot alone
        for name, e in (("code_coef_first", k), ("code_coef_last", n - 1)):
            delta = [pow(pydef.omegas(k)[2], j * e, P) for j in range(n)]
            polys = self._with("code", self.add_vec(self.poly["code"], delta))
            envelope, idx = self.assemble(*polys)
            put(name, envelope, expect("valid_code", "code_equal"), polys=polys, idx=idx)
        for which in ("lin", "quad"):
            polys, envelope, idx, tries = self.spike_unopened(which, column=4 * (k - l + 1))      # moves slot l - 1 alone
            put("%s_slot_last" % which, envelope, expect(VALID[which]), tries=tries, polys=polys, idx=idx)
        for which in POLYS:
            for end in ("first", "last"):
                polys, envelope, idx, tries = self.spike_opened(which, end)
                put("%s_spike_opened_%s" % (which, end), envelope, expect(VALID[which], EQUAL[which]), tries=tries, polys=polys, idx=idx)
        # transcript and parser forgeries around the honest polynomials
        hp = self.parts(*[self.poly[p] for p in POLYS])
        assert self.pack(**hp) == self.honest
        sib = hp["sib"]
        mid = len(sib) // 2
        flipped = sib[:mid] + [bytes([sib[mid][0] ^ 1]) + sib[mid][1:]] + sib[mid + 1:]
        put("sibling_flipped", self.pack(**dict(hp, sib=flipped)), expect("valid_merkle"))
        put("sibling_dropped", self.pack(**dict(hp, sib=sib[:-1])), expect("valid_merkle"))
        put("sibling_appended", self.pack(**dict(hp, sib=sib + [sib[-1]])), expect("valid_merkle"))
        idx = hp["idx"]
        swapped = idx[:40] + [idx[41], idx[40]] + idx[42:]
        put("indices_swapped", self.pack(**dict(hp, idx=swapped)), STOPS_AT_INDICES)
        dup = idx[:100] + [idx[100], idx[100]] + idx[102:]
        put("index_duplicated", self.pack(**dict(hp, idx=dup)), STOPS_AT_INDICES)
        # a residue + p (2p < 2^256, so it fits the 32 bytes): no statement about the oracle, which has no canonical check
        for tries, j in enumerate(range(UNOPENED_CAP), 1):
            code = self.poly["code"].copy()
            assert self.H["code"][j] + P < 1 << 256
            code[j] = _elem(self.H["code"][j] + P)
            envelope, nidx = self.assemble(code, self.poly["lin"], self.poly["quad"])
            if j not in nidx:
                put("noncanonical_code", envelope, STOPS_AT_PARSE, oracle_rejects=None, tries=tries)
                break
        else:
            raise AssertionError("noncanonical_code: no unopened column within %d tries" % UNOPENED_CAP)
        samples = bytearray(hp["samples"])
        at = 32 * ((self.R // 2) * t + 17)                     # row R/2, the 18th opened column
        v = int.from_bytes(samples[at:at + 32], "little") + P
        assert v < 1 << 256
        samples[at:at + 32] = v.to_bytes(32, "little")
        put("noncanonical_sample", self.pack(**dict(hp, samples=bytes(samples))), STOPS_AT_PARSE, oracle_rejects=None)
        put("meta_k_doubled", self.pack(**dict(hp, meta_k=2 * k)), STOPS_AT_PARSE)
        assert tuple(F) == NAMES
        self._forgeries = F
        return F

    def tries(self):
        """{name: tries} of the searches"""
        return {name: f.tries for name, f in self.forgeries().items() if f.tries is not None}


@functools.lru_cache(maxsize=None)
def forger(l, k, n, n_linear, n_quad):
    """one Forger per shape and process: the CPU and the GPU tests share it"""
    return Forger(l, k, n, n_linear, n_quad)
