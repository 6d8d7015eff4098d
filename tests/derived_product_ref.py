"""The yardstick of PRODUCT ENTRIES of derived slots ((slot, DERIVED_PRODUCT) in the list of lig_rows_set_derived /
lig_shard_rows_set_derived), in Python integers: the seeded narrow trace of tests/derived_ref.py (330 rows, three stage-1 chunks, the
LINEAR rows in front, the triples behind them, every other triple's z row LIG_ELEM_PRODUCT), a hand-built list that mixes linear targets and
product entries over it, the witness with every listed value filled in wave by wave

    linear   w[t] = b_c - sum_{j != t} a_j w[s_j]  (coefficient +1)    w[t] = sum_{j != t} a_j w[s_j] - b_c  (coefficient -1)
    product  w[r l + i] = w[(r - 2) l + i] * w[(r - 1) l + i] mod p

the oracle's envelope over the rows that carry those integers, and Python restatements of the waves and of the per-rank counts and
exchange schedule on a shard.  With world > 1 the list is placed against the deal of shard_rows_plan(kinds, world).  Nothing here calls the
library's derived path (amd is used for its constants, for pack_rows_mixed / narrowest_widths, which only lay bytes out, and for the deal)."""
import numpy as np

import derived_ref as dr
import linear_ref as lr
import oracle_lib as ol
import shard_derived_ref as sdr

P = ol.P
ONE, NEG_ONE = lr.ONE, lr.NEG_ONE
L, K, N = dr.L, dr.K, dr.N
N_LIN_ROWS, N_TRIPLES, CHUNKS = dr.N_LIN_ROWS, dr.N_TRIPLES, dr.CHUNKS
PRODUCT = 0xFFFFFFFF                                 # LIG_DERIVED_PRODUCT
limbs = dr.limbs


def reads_of(system, pairs, l):
    """{listed slot: the slots its entry reads}: the other terms of a defining constraint, the two operands of a product entry"""
    out = {}
    for t, c in pairs:
        if c == PRODUCT:
            out[t] = [t - 2 * l, t - l]
        else:
            terms = [system.slots[i] for i in range(system.term_begin[c], system.term_begin[c + 1])]
            assert terms.count(t) == 1
            terms.remove(t)
            out[t] = terms
    return out


def waves_of(system, pairs, l):
    """the Python restatement of the waves over both kinds of entry: 1 + the longest path through listed slots below an entry"""
    reads = reads_of(system, pairs, l)
    memo = {}

    def wave(s, open_=()):
        if s not in memo:
            assert s not in open_, "cycle"
            memo[s] = 1 + max([wave(d, open_ + (s,)) for d in reads[s] if d in reads], default=0)
        return memo[s]

    return {s: wave(s) for s in reads}


def shard_info(system, pairs, owner, l, rank, world):
    """shard_derived_ref.shard_info with product entries: -> (the dict of lig_derived_shard_info for `rank`, E) with E[w][q] = the sorted
    slots rank q sends in wave w + 1.  A product entry reads its two operands, which lie on its own rank"""
    waves = waves_of(system, pairs, l)
    reads = reads_of(system, pairs, l)
    n_waves = max(waves.values(), default=0)
    shipped, E = set(), []
    for w in range(1, n_waves + 1):
        need = [set() for _ in range(world)]
        for t in reads:
            if waves[t] == w:
                for s in reads[t]:
                    if owner[s // l] != owner[t // l] and s not in shipped:
                        need[owner[s // l]].add(s)
        for v in need:
            shipped |= v
        E.append([sorted(v) for v in need])
    blocks = [max(len(v) for v in e) for e in E]
    mine = [t for t in reads if owner[t // l] == rank]
    info = dict(n_slots=len(pairs), n_terms=sum(len(v) for v in reads.values()), n_waves=n_waves, n_exchanges=sum(1 for b in blocks if b),
                local_targets=len(mine), local_terms=sum(1 for t in mine for s in reads[t] if owner[s // l] == rank),
                imported_terms=sum(1 for t in mine for s in reads[t] if owner[s // l] != rank),
                imports=len({s for t in mine for s in reads[t] if owner[s // l] != rank}), exports=sum(len(e[rank]) for e in E),
                exchange_bytes=32 * world * sum(blocks))
    return info, E


class World:
    """amd: the binding (constants, packing, the deal).  Attributes: kinds, rows, widths, wide (records per row: one mixed row), system
    (the defining constraints and one CHECK constraint through every listed slot, product slots included), pairs [(slot, constraint or
    PRODUCT)], listed (all listed slots, sorted), w, expected_rows (the Python integers at every listed slot), shipped_rows (GARBAGE at every
    linear target; what a LIG_ELEM_PRODUCT row holds is never shipped), check_of, waves, owner (rank of every row) and the named slots the
    tests speak about"""

    def __init__(self, amd, seed=5, world=1):
        l = L
        self.world = world
        self.kinds, self.rows, self.masks = lr.build_trace(L, K, N, N_LIN_ROWS * l, N_TRIPLES * l, seed=seed, narrow=True)
        kinds, rows = self.kinds, self.rows
        R = len(kinds)
        assert R == CHUNKS[-1][1]
        self.rounds, self.boundaries = amd.shard_rows_plan(kinds, world)
        self.owner = owner = sdr.owner_of(self.boundaries, world, R)
        lin = lr.linear_rows(kinds)
        tri = [r for r in range(R) if kinds[r] == 1]
        assert lin == list(range(N_LIN_ROWS)) and len(tri) == N_TRIPLES
        for r in tri:
            assert owner[r] == owner[r + 1] == owner[r + 2]            # the deal never splits a triple
        self.widths = amd.narrowest_widths(rows, kinds, l)
        for t, r in enumerate(tri):
            assert self.widths[r] == self.widths[r + 1] == amd.ELEM_BIT   # the operand rows of the narrow trace are bit rows
            if t % 2 == 0:
                self.widths[r + 2] = amd.ELEM_PRODUCT                 # every other triple: z is formed on the device
        word_rows = [r for r in lin if self.widths[r] == 2]
        derived = [r for t, r in enumerate(tri) if t % 2 == 0]       # x rows of the triples whose z is LIG_ELEM_PRODUCT
        self.wide = np.zeros(R, dtype=np.uint32)
        rng = np.random.default_rng(seed + 300)
        full, full2 = (int(v) for v in ol.from_limbs(ol.rand_field(rng, 2)))
        assert full.bit_length() > 240 and full2.bit_length() > 240
        coefs = [0, full, 3, 1 << 9]
        FULL_C, THREE_C, POW_C = 1, 2, 3
        term_begin, slots, cidx, rhs_c, rhs_b = [0], [], [], [], []
        self.pairs, self.check_of, listed = [], {}, set()
        vrow = word_rows[40]                                          # the second slot of every check constraint; never a target row

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

        def check(t):
            """a second constraint through t that holds for the listed value only"""
            v = (vrow * l + t % l, ONE)
            self.check_of[t] = add([(t, THREE_C), v], (3 * w[t] + w[v[0]]) % P)

        def define(row, col, sign, others, b):
            t = row * l + col
            assert t not in listed and row != vrow and all(s != t for s, _ in others)
            listed.add(t)
            acc = sum(value(ci) * w[s] for s, ci in others) % P
            w[t] = (b - acc) % P if sign == ONE else (acc - b) % P
            terms = list(others)
            terms.insert(len(terms) // 2, (t, sign))
            self.pairs.append((t, add(terms, b)))
            check(t)
            return t

        def product(xrow, col):
            """the product entry of column col of the triple whose x row is xrow; its operands hold their final values by now"""
            assert self.widths[xrow + 2] == amd.ELEM_PRODUCT
            t = (xrow + 2) * l + col
            assert t not in listed
            listed.add(t)
            w[t] = w[xrow * l + col] * w[(xrow + 1) * l + col] % P
            self.pairs.append((t, PRODUCT))
            check(t)
            return t

        # rows to read inputs from: 16-bit LINEAR rows on the rank of `home` where it has some, `far`: on another rank (any row at world == 1)
        def inputs(n, home, far=False, first_chunk=False):
            pool = [r for r in word_rows if r != vrow and (not first_chunk or r < CHUNKS[0][1])]
            rws = [r for r in pool if (owner[r] != owner[home] if far and world > 1 else owner[r] == owner[home])]
            assert rws or not far
            rws = rws or pool                                         # a rank that was dealt triples only reads its inputs from other ranks
            return [(int(rws[int(rng.integers(0, len(rws)))]) * l + int(rng.integers(100, l)), ci) for ci in [FULL_C, ONE, NEG_ONE, POW_C][:n]]

        T0, T1, T2, T3 = derived[0], derived[1], derived[2], derived[3]
        Tlast = derived[-1]
        assert Tlast >= CHUNKS[-1][0] and T3 + 2 < CHUNKS[-1][0]
        # shipped operands the cases need: y = 1 where only x is derived, x = 1 where only y is; one full-width y as the RECORD of a mixed row
        for r, c in ((T0 + 1, 5), (T0, 9), (T2 + 1, 19), (T3, 19), (Tlast + 1, 17), (T2, 21), (T2 + 1, 21)):
            rows[r, c] = 0
            rows[r, c, 0] = 1
        rows[T1 + 1, 11] = limbs([full2])[0]
        self.wide[T1 + 1] = 1
        w = lr.witness(rows, l)
        # a full-width x on a bit row, times the shipped bit 1: the product reads the matrix, not the packed bits; its input is read by
        # nothing else
        self.input_of_a = inputs(1, T0)[0][0]
        self.x_a = define(T0, 5, NEG_ONE, [(self.input_of_a, FULL_C), (word_rows[3] * l + 7, ONE)], 0)
        assert w[self.x_a].bit_length() > 240
        self.z_a = product(T0, 5)
        # both operands derived at one column, in different waves
        xb = define(T0, 7, ONE, inputs(3, T0), 77)
        self.y_b = define(T0 + 1, 7, NEG_ONE, [(xb, FULL_C)] + inputs(2, T0), 0)
        self.z_b = product(T0, 7)
        # only y derived
        define(T0 + 1, 9, NEG_ONE, inputs(4, T0), 5)
        self.z_c = product(T0, 9)
        # x derived, y the record of a mixed row
        define(T1, 11, ONE, inputs(2, T1), 9)
        self.z_d = product(T1, 11)
        assert w[(T1 + 1) * l + 11] == full2 and w[self.z_d] not in (0, w[T1 * l + 11])
        # (p - 1) * (p - 1) = 1, both constants of their constraints; 0 * x
        define(T1, 13, ONE, [], P - 1)
        define(T1 + 1, 13, NEG_ONE, [], 1)
        self.z_e = product(T1, 13)
        assert w[T1 * l + 13] == w[(T1 + 1) * l + 13] == P - 1 and w[self.z_e] == 1
        define(T1, 15, NEG_ONE, [], 0)
        define(T1 + 1, 15, ONE, inputs(2, T1), 31)
        self.z_f = product(T1, 15)
        assert w[T1 * l + 15] == 0 and w[(T1 + 1) * l + 15] > 1 and w[self.z_f] == 0
        # a triple of the last chunk whose x reads first-chunk rows (of another rank, where there is one), and a first-chunk target (on another
        # rank than the triple, where there is one) that reads the re-formed z
        self.x_far = define(Tlast, 17, NEG_ONE, inputs(2, Tlast, far=True, first_chunk=True), 0)
        self.z_far = product(Tlast, 17)
        back = next(r for r in lin[10:] if r not in word_rows[:50] and r < CHUNKS[0][1] and (world == 1 or owner[r] != owner[Tlast]))
        self.t_back = define(back, 31, ONE, [(self.z_far, FULL_C), (self.z_far, ONE)] + inputs(1, back), 1)
        # five waves: x -> z -> a linear target that is the y of the next triple -> its z -> a last linear target
        c1 = define(T2, 19, NEG_ONE, inputs(2, T2), 0)
        self.c2 = product(T2, 19)
        c3 = define(T3 + 1, 19, ONE, [(self.c2, FULL_C)] + inputs(1, T3), 123456789)
        self.c4 = product(T3, 19)
        last = next(r for r in lin[20:] if r not in word_rows[:50] and r != back)
        self.c5 = define(last, 33, NEG_ONE, [(self.c4, ONE), (c1, POW_C)], 0)
        # a product entry whose operands are both shipped: wave 1, the value the row's own pass formed
        self.z_plain = product(T2, 21)
        assert w[self.z_plain] == 1
        self.system = lr.System(term_begin, slots, cidx, rhs_c, rhs_b, coefs, 0)
        self.listed = sorted(listed)
        assert slots.count(self.input_of_a) == 1 and w[self.input_of_a] > 1
        self.linear_targets = sorted(t for t, c in self.pairs if c != PRODUCT)
        self.w = w
        self.expected_rows = rows.copy()
        for t in self.listed:
            self.expected_rows[t // l, t % l] = limbs([w[t]])[0]
        # every LIG_ELEM_PRODUCT row of the statement is x * y in every column, listed or not
        for r in derived:
            x, y, z = (lr.witness(self.expected_rows[r + d:r + d + 1], l) for d in range(3))
            assert all(a * b % P == c for a, b, c in zip(x, y, z)), r
        assert lr.holds(self.system, self.expected_rows, l)
        # what is shipped: garbage that fits the row's width at every linear target, never the expected value
        self.shipped_rows = rows.copy()
        for t in self.linear_targets:
            g = (0 if w[t] == 1 else 1) if self.widths[t // l] == amd.ELEM_BIT else 0xBEEF
            assert g != w[t]
            self.shipped_rows[t // l, t % l] = limbs([g])[0]
        self.waves = waves_of(self.system, self.pairs, l)
        assert [self.waves[t] for t in (c1, self.c2, c3, self.c4, self.c5)] == [1, 2, 3, 4, 5] and max(self.waves.values()) == 5
        assert (self.waves[xb], self.waves[self.y_b], self.waves[self.z_b], self.waves[self.z_plain]) == (1, 2, 3, 1)
        assert self.waves[self.t_back] == 3 and self.t_back // l < CHUNKS[0][1] and all(s // l < CHUNKS[0][1] for s in reads_of(self.system, self.pairs, l)[self.x_far])
        if world > 1:
            reads = reads_of(self.system, self.pairs, l)
            assert any(owner[s // l] != owner[self.x_far // l] for s in reads[self.x_far])       # a derived x that imports a term
            assert owner[self.t_back // l] != owner[self.z_far // l]                             # a re-formed z read by another rank
            _, E = shard_info(self.system, self.pairs, owner, l, 0, world)
            assert self.z_far in E[2][owner[self.z_far // l]]                                    # ... sent in the reader's wave, 3
        rng.shuffle(self.pairs)                                        # d may be in any order

    def ship(self, amd, rows=None):
        """-> (kinds | ROW_DRAW_PAD, packed bytes of `rows` (default: shipped_rows) with the one mixed row)"""
        kk = self.kinds.copy()
        kk[self.kinds <= 3] |= amd.ROW_DRAW_PAD
        return kk, amd.pack_rows_mixed(self.shipped_rows if rows is None else rows, self.widths, self.wide, L)

    def pack_local(self, amd, rows, mine):
        """the packed bytes of the rows `mine` (global indices, commit order)"""
        if not len(mine):
            return np.zeros(0, dtype=np.uint8)
        return np.frombuffer(amd.pack_rows_mixed(rows[mine], self.widths[mine], self.wide[mine], L), dtype=np.uint8).copy()

    def oracle(self, rows):
        """the oracle's envelope over `rows` under the system -> dict(proof, root, stage1_seed, valid, ...)"""
        return lr.oracle_envelope(L, K, N, self.kinds, rows, self.masks, self.system)[3]


_worlds = {}


def world(amd, seed=5, world_size=1):
    if (seed, world_size) not in _worlds:
        _worlds[seed, world_size] = World(amd, seed, world_size)
    return _worlds[seed, world_size]
