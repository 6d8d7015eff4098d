"""The yardstick of derived slots (lig_rows_set_derived), in Python integers: a seeded narrow trace of 330 rows (three stage-1 chunks:
[0, 128), [128, 234), [234, 330)), a hand-built list of derived slots over it, the witness with every derived value filled in

    w[t] = b_c - sum_{j != t} a_j w[s_j]   (coefficient +1)        w[t] = sum_{j != t} a_j w[s_j] - b_c   (coefficient -1)

wave by wave, and the oracle's envelope over the rows that carry those integers.  Nothing here calls the library under test (amd is used
for its constants and for pack_rows / narrowest_widths, which only lay bytes out)."""
import numpy as np

import linear_ref as lr
import oracle_lib as ol

P = ol.P
ONE, NEG_ONE = lr.ONE, lr.NEG_ONE
L, K, N = 320, 512, 2048
N_LIN_ROWS, N_TRIPLES = 150, 60
CHUNKS = [(0, 128), (128, 234), (234, 330)]          # head 128, tail 96 (chunk_schedule, prover_common.hpp)
LANE_MAX = 64                                        # DERIVE_LANE_MAX (csrc/derive_plan.hpp): more other terms than this -> a workgroup


def limbs(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint32).reshape(-1, 8).copy()


def waves_of(system, pairs):
    """the Python restatement of the waves: 1 + the longest path through derived slots below a target -> {slot: wave}"""
    by_slot = dict(pairs)
    memo = {}

    def wave(s, open_=()):
        if s in memo:
            return memo[s]
        assert s not in open_, "cycle"
        c = by_slot[s]
        deps = [system.slots[t] for t in range(system.term_begin[c], system.term_begin[c + 1]) if system.slots[t] != s and system.slots[t] in by_slot]
        memo[s] = 1 + max([wave(d, open_ + (s,)) for d in deps], default=0)
        return memo[s]

    return {s: wave(s) for s in by_slot}


class World:
    """amd: the binding (constants, packing).  Attributes: kinds, rows (the seeded trace), widths, system (lr.System: the defining
    constraints and one CHECK constraint through every target), pairs [(slot, defining constraint)], expected_rows (rows with the Python
    integers at every target), shipped_rows (rows with GARBAGE at every target), check_of {target: its check constraint}, input_of_b (a
    slot only the defining constraint of target `b` reads)"""

    def __init__(self, amd, seed):
        l = L
        self.kinds, self.rows, self.masks = lr.build_trace(L, K, N, N_LIN_ROWS * l, N_TRIPLES * l, seed=seed, narrow=True)
        kinds, rows = self.kinds, self.rows
        R = len(kinds)
        assert R == CHUNKS[-1][1]
        lin = lr.linear_rows(kinds)
        tri = [r for r in range(R) if kinds[r] == 1]
        assert lin == list(range(N_LIN_ROWS)) and len(tri) == N_TRIPLES
        self.widths = amd.narrowest_widths(rows, kinds, l)
        for t, r in enumerate(tri):
            if t % 2 == 0:
                self.widths[r + 2] = amd.ELEM_PRODUCT                 # every other triple: z is formed on the device
        bit_rows = [r for r in lin if self.widths[r] == amd.ELEM_BIT]
        word_rows = [r for r in lin if self.widths[r] == 2]
        assert len(bit_rows) > 60 and len(word_rows) > 60
        plain = [r for t, r in enumerate(tri) if t % 2 == 1]         # triples whose z is shipped
        derived = [r for t, r in enumerate(tri) if t % 2 == 0]
        w = lr.witness(rows, l)
        rng = np.random.default_rng(seed + 100)
        full = int(ol.from_limbs(ol.rand_field(rng, 1))[0])
        assert full.bit_length() > 240
        coefs = [0, full] + [1 << e for e in range(33)] + [3]
        ZERO_C, FULL_C, POW0, THREE_C = 0, 1, 2, 35
        term_begin, slots, cidx, rhs_c, rhs_b = [0], [], [], [], []
        self.pairs, self.check_of, targets = [], {}, set()

        def value(ci):
            return 1 if ci == ONE else P - 1 if ci == NEG_ONE else coefs[ci]

        def add(terms, b):
            for s, ci in terms:
                slots.append(s)
                cidx.append(ci)
            term_begin.append(len(slots))
            c = len(term_begin) - 2
            if b:
                rhs_c.append(c)
                rhs_b.append(len(coefs))
                coefs.append(b)
            return c

        def define(row, col, sign, others, b, pos=None):
            t = row * l + col
            assert t not in targets and all(s != t for s, _ in others)
            targets.add(t)
            acc = sum(value(ci) * w[s] for s, ci in others) % P
            w[t] = (b - acc) % P if sign == ONE else (acc - b) % P
            terms = list(others)
            terms.insert(len(terms) // 2 if pos is None else pos, (t, sign))
            self.pairs.append((t, add(terms, b)))
            # the check constraint: a second constraint through the target that holds for the derived value only
            v = (word_rows[40] * l + col, ONE)
            self.check_of[t] = add([(t, THREE_C), v], (3 * w[t] + w[v[0]]) % P)
            return t

        some = lambda n, rws: [(int(rws[int(rng.integers(0, len(rws)))]) * l + int(rng.integers(100, l)), ci)
                               for ci in [[ONE, NEG_ONE, FULL_C, POW0 + 5, POW0 + 31][i % 5] for i in range(n)]]
        # 0 other terms: a constant (+1, b != 0) and a zero (-1, b == 0)
        self.t_const = define(lin[0], 5, ONE, [], 123456789)
        self.t_zero = define(lin[1], 7, NEG_ONE, [], 0)
        # 1 other term, the special -1, on a QX row; its input is read by nothing else
        self.input_of_b = word_rows[41] * l + 9
        self.t_b = define(plain[0], 11, NEG_ONE, [(self.input_of_b, NEG_ONE)], 0)
        # 3 other terms on a QY row: a table entry of 0, a full-width entry, a slot repeated; b != 0
        rep = word_rows[3] * l + 20
        self.t_c = define(plain[1] + 1, 13, ONE, [(rep, FULL_C), (bit_rows[2] * l + 4, ZERO_C), (rep, NEG_ONE)], 77)
        # 33 other terms: a word recomposed from bits, on a shipped QZ row (the eval of i32_add: sum 2^i bit_i - w = 0)
        self.t_word = define(plain[2] + 2, 17, NEG_ONE, [(bit_rows[30] * l + i, POW0 + i) for i in range(33)], 0, pos=33)
        # the per-lane threshold: 64 other terms (a lane), 65 (a workgroup), 700 (a workgroup striding its segment)
        self.t_light = define(lin[4], 19, ONE, some(LANE_MAX, bit_rows + word_rows), 5)
        self.t_heavy = define(lin[5], 21, NEG_ONE, some(LANE_MAX + 1, bit_rows + word_rows), 0)
        self.t_long = define(lin[6], 23, ONE, some(700, bit_rows + word_rows), 9)
        # a chain of 3 waves
        h1 = define(lin[7], 25, NEG_ONE, [(word_rows[5] * l + 1, ONE), (word_rows[6] * l + 2, POW0 + 7)], 0)
        h2 = define(lin[8], 27, ONE, [(h1, FULL_C), (self.t_const, NEG_ONE)], 31)
        self.t_chain = define(lin[9], 29, NEG_ONE, [(h2, ONE), (self.t_word, POW0 + 3), (self.t_heavy, NEG_ONE)], 0)
        # a target in the first chunk whose terms lie on rows of the last chunk, one of them a LIG_ELEM_PRODUCT slot
        last_derived, last_plain = derived[-1], plain[-1]
        assert lin[10] < CHUNKS[0][1] and last_derived + 2 >= CHUNKS[-1][0] and last_plain >= CHUNKS[-1][0]
        assert self.widths[last_derived + 2] == amd.ELEM_PRODUCT
        ones = [c for c in range(l) if w[(last_derived + 2) * l + c] == 1][:3]
        assert len(ones) == 3
        self.t_far = define(lin[10], 31, ONE, [((last_derived + 2) * l + ones[0], FULL_C), ((last_derived + 2) * l + ones[1], ONE),
                                                (last_plain * l + 3, POW0 + 9), ((last_plain + 1) * l + 3, NEG_ONE)], 1)
        self.system = lr.System(term_begin, slots, cidx, rhs_c, rhs_b, coefs, 0)
        self.targets = sorted(targets)
        self.w = w
        self.expected_rows = rows.copy()
        for t in self.targets:
            self.expected_rows[t // l, t % l] = limbs([w[t]])[0]
        assert lr.holds(self.system, self.expected_rows, l)
        # what is shipped: garbage that fits the row's width at every target, never the expected value
        self.shipped_rows = rows.copy()
        for t in self.targets:
            g = 1 if self.widths[t // l] == amd.ELEM_BIT else 0xBEEF
            assert g != w[t]
            self.shipped_rows[t // l, t % l] = limbs([g])[0]
        self.waves = waves_of(self.system, self.pairs)
        assert max(self.waves.values()) == 3 and self.waves[self.t_chain] == 3
        rng.shuffle(self.pairs)                                        # d may be in any order

    def ship(self, amd, rows=None):
        """-> (kinds | ROW_DRAW_PAD, packed bytes of `rows` (default: shipped_rows) in the narrow format)"""
        kk = self.kinds.copy()
        kk[self.kinds <= 3] |= amd.ROW_DRAW_PAD
        return kk, amd.pack_rows(self.shipped_rows if rows is None else rows, self.widths, L)

    def oracle(self, rows):
        """the oracle's envelope over `rows` under the system -> dict(proof, root, stage1_seed, valid, ...)"""
        return lr.oracle_envelope(L, K, N, self.kinds, rows, self.masks, self.system)[3]


_worlds = {}


def world(amd, seed=5):
    if seed not in _worlds:
        _worlds[seed] = World(amd, seed)
    return _worlds[seed]
