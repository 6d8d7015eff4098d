"""The yardstick of derived slots on a rows shard (lig_shard_rows_set_derived), in Python integers: the seeded narrow trace of
tests/derived_ref.py at a size the case chooses, a list of derived slots PLACED AGAINST THE DEAL of shard_rows_plan(kinds, W) -- so that which
operand crosses which ranks in which wave holds by construction and is asserted here, on the host -- the witness with every derived value
filled in wave by wave, the oracle's envelope over the rows that carry those integers, and a Python restatement of the per-rank counts and
of the exchange schedule (shard_info).  Nothing here calls the sharded derived path (amd is used for its constants, for pack_rows /
narrowest_widths, which only lay bytes out, and for the deal: shard_rows_plan / local_rows_of)."""
import numpy as np

import derived_ref as dr
import linear_ref as lr
import oracle_lib as ol

P, L, K, N = dr.P, dr.L, dr.K, dr.N
ONE, NEG_ONE = lr.ONE, lr.NEG_ONE
LANE_MAX = dr.LANE_MAX
limbs = dr.limbs


def owner_of(boundaries, world, n_rows):
    """the rank of every row: chunk g of the deal belongs to rank g mod world"""
    owner = np.zeros(n_rows, dtype=np.int64)
    for g in range(len(boundaries) - 1):
        owner[int(boundaries[g]):int(boundaries[g + 1])] = g % world
    return owner


def shard_info(system, pairs, owner, l, rank, world):
    """the Python restatement of lig_derived_shard_info for `rank`, and of the schedule: -> (dict of the counts, E) with E[w][q] = the sorted
    slots rank q sends in wave w + 1 (those another rank's wave-(w + 1) target reads and no earlier wave has sent)"""
    waves = dr.waves_of(system, pairs)
    n_waves = max(waves.values(), default=0)
    others = {}
    for t, c in pairs:
        terms = [system.slots[i] for i in range(system.term_begin[c], system.term_begin[c + 1])]
        assert terms.count(t) == 1
        terms.remove(t)
        others[t] = terms
    shipped, E = set(), []
    for w in range(1, n_waves + 1):
        need = [set() for _ in range(world)]
        for t in others:
            if waves[t] == w:
                for s in others[t]:
                    if owner[s // l] != owner[t // l] and s not in shipped:
                        need[owner[s // l]].add(s)
        for v in need:
            shipped |= v
        E.append([sorted(v) for v in need])
    blocks = [max(len(v) for v in e) for e in E]
    mine = [t for t in others if owner[t // l] == rank]
    info = dict(n_slots=len(pairs), n_terms=sum(len(v) for v in others.values()), n_waves=n_waves, n_exchanges=sum(1 for b in blocks if b),
                local_targets=len(mine), local_terms=sum(1 for t in mine for s in others[t] if owner[s // l] == rank),
                imported_terms=sum(1 for t in mine for s in others[t] if owner[s // l] != rank),
                imports=len({s for t in mine for s in others[t] if owner[s // l] != rank}), exports=sum(len(e[rank]) for e in E),
                exchange_bytes=32 * world * sum(blocks))
    return info, E


class ShardWorld:
    """amd: the binding (constants, packing, the deal).  world ranks; `idle` (or None) is dealt rows but no target.  Attributes as
    derived_ref.World (kinds, rows, widths, system, pairs, expected_rows, shipped_rows, check_of, targets, w, waves) plus owner (rank of every
    row), boundaries, rounds, and the named targets the assertions of conditions() speak about."""

    def __init__(self, amd, world, n_lin_rows, n_triples, seed=5, idle=None):
        l = L
        self.world, self.idle = world, idle
        self.kinds, self.rows, self.masks = lr.build_trace(L, K, N, n_lin_rows * l, n_triples * l, seed=seed, narrow=True)
        kinds, rows = self.kinds, self.rows
        R = len(kinds)
        self.rounds, self.boundaries = amd.shard_rows_plan(kinds, world)
        self.owner = owner = owner_of(self.boundaries, world, R)
        lin = lr.linear_rows(kinds)
        tri = [r for r in range(R) if kinds[r] == 1]
        self.widths = amd.narrowest_widths(rows, kinds, l)
        for t, r in enumerate(tri):
            if t % 2 == 0:
                self.widths[r + 2] = amd.ELEM_PRODUCT                 # every other triple: z is formed on the device
        plain = [r for t, r in enumerate(tri) if t % 2 == 1]         # triples whose z is shipped
        product = [r + 2 for t, r in enumerate(tri) if t % 2 == 0]   # the LIG_ELEM_PRODUCT rows
        home = 0
        ranks = [q for q in range(world) if q != idle]
        # the plain triple that gets targets on its QX, QY and QZ rows (on the last rank that has targets and such a triple).  z = x * y stays
        # true there: y = z = 0 in the column of the QX target, x = z = 0 in that of the QY target, and the QZ target is given the value x * y
        tq = next(q for q in ranks[::-1] if any(owner[r] == q for r in plain))
        trip = next(r for r in plain if owner[r] == tq)
        QX_COL, QY_COL = 1, 3
        rows[trip + 1, QX_COL] = rows[trip + 2, QX_COL] = 0
        rows[trip, QY_COL] = rows[trip + 2, QY_COL] = 0
        w = lr.witness(rows, l)
        rng = np.random.default_rng(seed + 200)
        full = int(ol.from_limbs(ol.rand_field(rng, 1))[0])
        coefs = [0, full] + [1 << e for e in range(33)] + [3]
        FULL_C, POW0, THREE_C = 1, 2, 35
        term_begin, slots, cidx, rhs_c, rhs_b = [0], [], [], [], []
        self.pairs, self.check_of, targets = [], {}, set()
        away = [q for q in range(world) if q != home]                # ranks whose slots a target on `home` imports (the idle rank among them)
        peer = next(q for q in ranks if q != home)                   # the other end of the chain
        vrow = lin[-1]                                               # never a target row: the second slot of every check constraint
        # target rows per rank, in the order they are used: LINEAR rows (bit rows and 16-bit rows alternate), then the rows of plain triples
        pool = {q: [r for r in lin[:-1] if owner[r] == q] + [r + d for r in plain for d in range(3) if owner[r] == q] for q in range(world)}
        used = {q: 0 for q in range(world)}
        next_col = [5]

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

        def define(q, sign, others, b, row=None, col=None, want=None):
            """a target on the next unused row of rank q (or on `row`), in a column no operand uses (targets: odd columns < 100); want: the
            value the target is to have -- the right-hand side is chosen for it"""
            if row is None:
                row = pool[q][used[q]]
                used[q] += 1
            assert owner[row] == q and row != vrow
            if col is None:
                col = next_col[0]
                next_col[0] += 2
            assert col < 98
            t = row * l + col
            assert t not in targets and all(s != t for s, _ in others)
            targets.add(t)
            acc = sum(value(ci) * w[s] for s, ci in others) % P
            if want is not None:
                b = (want + acc) % P if sign == ONE else (acc - want) % P
            w[t] = (b - acc) % P if sign == ONE else (acc - b) % P
            terms = list(others)
            terms.insert(len(terms) // 2, (t, sign))
            self.pairs.append((t, add(terms, b)))
            # the check constraint: a second constraint through the target that holds for the derived value only
            v = (vrow * l + col, ONE)
            self.check_of[t] = add([(t, THREE_C), v], (3 * w[t] + w[v[0]]) % P)
            return t

        kinds_ok = lambda r: kinds[r] <= 3
        held = {q: [r for r in range(R) if owner[r] == q and kinds_ok(r)] for q in range(world)}

        def some(n, qs):
            """n operands (slot, coefficient index) on rows of the ranks qs, in turn; columns >= 100: never a target"""
            out = []
            for i in range(n):
                rws = held[qs[i % len(qs)]]
                out.append((int(rws[int(rng.integers(0, len(rws)))]) * l + int(rng.integers(100, l)), [ONE, NEG_ONE, FULL_C, POW0 + 5, POW0 + 31][i % 5]))
            return out

        # every operand local | operands on two other ranks (on the other rank at W = 2) and one at home; `twice` is read again in wave 3
        self.t_local = define(home, ONE, some(3, [home]), 123456789)
        self.twice = some(1, [away[0]])[0][0]
        self.t_cross = define(home, NEG_ONE, some(2, away[:2]) + [(self.twice, POW0 + 2)] + some(1, [home]), 0)
        # a slot only the defining constraint of t_in reads, on another rank than t_in (column 98: no target, no operand of some())
        in_rows = [r for r in pool[peer] if kinds[r] == 0] or pool[peer]
        self.input_of_in = in_rows[-1] * l + 98
        self.t_in = define(home, NEG_ONE, [(self.input_of_in, NEG_ONE)], 0)
        # the rows of one plain triple of a rank that has targets, and a LINEAR row: targets on QX, QY, shipped QZ
        for d in range(3):
            pool[tq].remove(trip + d)
        self.t_qx = define(tq, ONE, some(2, [q for q in range(world) if q != tq]) + some(1, [tq]), 77, row=trip, col=QX_COL)
        self.t_qy = define(tq, NEG_ONE, some(3, [tq]), 0, row=trip + 1, col=QY_COL)
        bits = next(r for r in lin if self.widths[r] == amd.ELEM_BIT and owner[r] != tq)
        self.t_word = define(tq, NEG_ONE, [(bits * l + 100 + i, POW0 + i) for i in range(33)], 0, row=trip + 2,
                                  want=w[trip * l + next_col[0]] * w[(trip + 1) * l + next_col[0]])      # a word recomposed from another rank's bits
        # the per-lane threshold with both sources: 65 other terms, 40 local and 25 imported; 700 imported terms
        self.t_heavy = define(home, NEG_ONE, some(40, [home]) + some(25, away), 0)
        self.t_long = define(home, ONE, some(700, away), 9)
        # a LIG_ELEM_PRODUCT slot of another rank
        prow = next(r for r in product if owner[r] != home)
        self.t_prod = define(home, ONE, [(prow * l + 150, FULL_C), (prow * l + 151, ONE)] + some(1, [home]), 1)
        # a chain of three waves that alternates ranks: each link reads a DERIVED slot of the other rank; the last reads `twice` again
        self.c1 = define(home, NEG_ONE, some(2, [home]), 0)
        self.c2 = define(peer, ONE, [(self.c1, FULL_C)] + some(1, [peer]), 31)
        self.c3 = define(home, NEG_ONE, [(self.c2, ONE), (self.twice, NEG_ONE), (self.t_heavy, POW0 + 3)], 0)
        # wave 4 reads nothing of another rank: its collective is skipped
        self.t_quiet = define(home, ONE, [(self.c3, ONE)] + some(2, [home]), 5)
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
            g = (0 if w[t] == 1 else 1) if self.widths[t // l] == amd.ELEM_BIT else 0xBEEF
            assert g != w[t]
            self.shipped_rows[t // l, t % l] = limbs([g])[0]
        self.waves = dr.waves_of(self.system, self.pairs)
        rng.shuffle(self.pairs)                                        # d may be in any order
        self.conditions(amd)

    def conditions(self, amd):
        """what the cases rely on, asserted from the deal and the list alone"""
        l, owner, s, world = L, self.owner, self.system, self.world
        by_slot = dict(self.pairs)
        ranks_of = lambda t: [int(owner[x // l]) for x in s.slots[s.term_begin[by_slot[t]]:s.term_begin[by_slot[t] + 1]] if x != t]
        me = lambda t: int(owner[t // l])
        assert set(ranks_of(self.t_local)) == {me(self.t_local)}
        assert len(set(ranks_of(self.t_cross)) - {me(self.t_cross)}) >= min(2, world - 1)
        assert [self.waves[t] for t in (self.c1, self.c2, self.c3, self.t_quiet)] == [1, 2, 3, 4] and max(self.waves.values()) == 4
        assert me(self.c1) != me(self.c2) and me(self.c2) != me(self.c3)
        rh = ranks_of(self.t_heavy)
        assert len(rh) > LANE_MAX and 0 < rh.count(me(self.t_heavy)) < len(rh)
        rl = ranks_of(self.t_long)
        assert len(rl) == 700 and me(self.t_long) not in rl
        _, E = shard_info(s, self.pairs, owner, l, 0, world)
        sent = [x for e in E for v in e for x in v]
        assert len(sent) == len(set(sent))                             # a slot is shipped once ...
        assert self.twice in E[0][owner[self.twice // l]] and self.waves[self.t_cross] == 1 and self.waves[self.c3] == 3      # ... though two waves read it across ranks
        assert all(not v for v in E[3]) and all(any(v for v in e) for e in E[:3])      # wave 4 has no collective, waves 1 to 3 have one
        assert self.c1 in E[1][me(self.c1)] and self.c2 in E[2][me(self.c2)]           # derived slots travel
        kinds_hit = {int(self.kinds[t // l]) for t in self.targets}
        assert kinds_hit == {0, 1, 2, 3} and self.widths[self.t_word // l] != amd.ELEM_PRODUCT
        prow = [x // l for x in s.slots[s.term_begin[by_slot[self.t_prod]]:s.term_begin[by_slot[self.t_prod] + 1]] if self.widths[x // l] == amd.ELEM_PRODUCT]
        assert prow and owner[prow[0]] != me(self.t_prod)
        x, y, z = (lr.witness(self.expected_rows[r:r + 1], l) for r in range(self.t_qx // l, self.t_qx // l + 3))
        assert all(a * b % P == c for a, b, c in zip(x, y, z))                         # the triple with targets is still a product
        assert any(self.widths[t // l] == amd.ELEM_BIT for t in self.targets)          # a bit row with garbage (a 1) shipped at its target
        assert owner[self.input_of_in // l] != me(self.t_in) and s.slots.count(self.input_of_in) == 1
        if self.idle is not None:
            assert all(me(t) != self.idle for t in self.targets) and (owner == self.idle).any()

    def ship(self, amd, rows=None):
        """-> (kinds | ROW_DRAW_PAD, the rows to ship (default: shipped_rows)); a rank packs its own with pack_local"""
        kk = self.kinds.copy()
        kk[self.kinds <= 3] |= amd.ROW_DRAW_PAD
        return kk, self.shipped_rows if rows is None else rows

    def pack_local(self, amd, rows, mine):
        """the packed bytes of the rows `mine` (global indices, commit order) of `rows` in the narrow format"""
        if not len(mine):
            return np.zeros(0, dtype=np.uint8)
        return np.frombuffer(amd.pack_rows(rows[mine], self.widths[mine], L), dtype=np.uint8).copy()

    def oracle(self, rows):
        """the oracle's envelope over `rows` under the system -> dict(proof, root, stage1_seed, valid, ...)"""
        return lr.oracle_envelope(L, K, N, self.kinds, rows, self.masks, self.system)[3]


_worlds = {}


def world(amd, world_size, n_lin_rows=150, n_triples=60, seed=5, idle=None):
    key = (world_size, n_lin_rows, n_triples, seed, idle)
    if key not in _worlds:
        _worlds[key] = ShardWorld(amd, world_size, n_lin_rows, n_triples, seed, idle)
    return _worlds[key]
