// derive_shard_plan_prog.cpp -- the per-rank program and the exchange schedule of derived slots on a rows shard (plan_derived_shard,
// ligero-prover_amd/csrc/derive_plan.hpp) as a stand-alone host program: no GPU, no library.  tests/test_shard_derived_plan.py builds it with
// AddressSanitizer and UBSan and runs it.  One list of six targets in four waves over 6 LINEAR rows (l = 8), planned under hand-written
// deals at W = 1, 2, 3 and 4; every expected number below was worked out by hand from the list and the deal:
//   A  t =  0 (row 0) = w[1] + w[2]                      wave 1   every operand on its own row
//   B  t =  8 (row 1) = w[16] + w[24] + w[9]             wave 1   operands on rows 2 and 3
//   C1 t = 17 (row 2) = w[10]                            wave 1   |
//   C2 t = 11 (row 1) = w[17] + w[16]                    wave 2   | a chain that alternates rows 2, 1, 2; C2 reads slot 16 again
//   C3 t = 18 (row 2) = w[11] + w[0]                     wave 3   |
//   D  t = 40 (row 5) = w[18] + w[41]                    wave 4
// Checked per deal and rank: the targets it keeps (local row, column), the split into local terms (local slot) and imported terms
// (absolute import position), E_q(w) ascending and shipped once, B(w), skipped waves, the import offsets, the counts.  The deals include a
// rank with no rows and a rank with rows but no targets; a second list checks light before heavy with a target whose 65 terms are split.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ligero-prover_amd/csrc/derive_plan.hpp"

#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

namespace {
using U = std::vector<uint32_t>;
struct Sys {
    U tb{0};
    std::vector<lig_lin_term> terms;
    uint32_t add(std::vector<lig_lin_term> t) {
        for (const lig_lin_term& x : t) terms.push_back(x);
        tb.push_back((uint32_t)terms.size());
        return (uint32_t)tb.size() - 2;
    }
    lig_linear_system view() const {
        lig_linear_system s;
        std::memset(&s, 0, sizeof s);
        s.struct_bytes = sizeof s;
        s.n_constraints = tb.size() - 1; s.n_terms = terms.size();
        s.term_begin = tb.data(); s.terms = terms.data();
        return s;
    }
};
const uint32_t ONE = LIG_COEF_ONE, NEG = LIG_COEF_NEG_ONE, l = 8, ROWS = 6;
const uint8_t kinds[ROWS] = {0, 0, 0, 0, 0, 0};

U sends_of(const lig::DeriveShardPlan& sp, uint32_t q, uint32_t w) {
    const size_t i = (size_t)q * sp.n_waves + w;
    return U(sp.sends.begin() + sp.send_begin[i], sp.sends.begin() + sp.send_begin[i + 1]);
}
// the terms [b, e) of a rank's program as their slots
U slots_of(const lig::DeriveShardPlan& sp, uint32_t b, uint32_t e) {
    U v;
    for (uint32_t t = b; t < e; t++) v.push_back(sp.terms[t].slot);
    return v;
}
bool target_is(const lig::DeriveShardPlan& sp, size_t i, uint32_t row, uint32_t col, const U& local, const U& imported) {
    const lig::DeriveShardTarget& t = sp.targets[i];
    return t.row == row && t.col == col && t.negate == 1 && t.rhs == lig::DERIVE_RHS_ZERO && slots_of(sp, t.begin, t.mid) == local && slots_of(sp, t.mid, t.end) == imported;
}
}  // namespace

int main() {
    using lig::DerivePlan;
    using lig::DeriveShardPlan;
    Sys S;
    const uint32_t cA = S.add({{1, ONE}, {0, NEG}, {2, ONE}}), cB = S.add({{16, ONE}, {24, ONE}, {8, NEG}, {9, ONE}}), cC1 = S.add({{17, NEG}, {10, ONE}});
    const uint32_t cC2 = S.add({{17, ONE}, {11, NEG}, {16, ONE}}), cC3 = S.add({{11, ONE}, {0, ONE}, {18, NEG}}), cD = S.add({{18, ONE}, {41, ONE}, {40, NEG}});
    const lig_linear_system sys = S.view();
    const lig_derived_slot d[] = {{0, cA}, {8, cB}, {17, cC1}, {11, cC2}, {18, cC3}, {40, cD}};
    DerivePlan p;
    CHECK(!lig::plan_derived(sys, kinds, ROWS, l, nullptr, d, 6, p));
    CHECK(p.n_waves == 4 && p.wave_of == U({1, 1, 1, 2, 3, 4}) && p.terms.size() == 12);
    DeriveShardPlan sp;
    {   // W = 1: everything is local, nothing is exchanged
        const lig::DeriveDeal deal = lig::derive_deal_of(U({0, 0, 0, 0, 0, 0}), 1);
        CHECK(deal.local_of == U({0, 1, 2, 3, 4, 5}));
        CHECK(!lig::plan_derived_shard(p, deal, l, 0, 1, sp));
        CHECK(sp.n_waves == 4 && sp.n_exchanges == 0 && sp.block == U({0, 0, 0, 0}) && sp.import_begin == U({0, 0, 0, 0, 0}) && sp.import_elems() == 0);
        CHECK(sp.wave_begin == U({0, 3, 4, 5, 6}) && sp.wave_light == U({3, 1, 1, 1}));
        CHECK(sp.local_terms == 12 && sp.imported_terms == 0 && sp.n_imports == 0 && sp.n_exports == 0 && sp.sends.empty());
        CHECK(target_is(sp, 1, 1, 0, U({16, 24, 9}), U()) && target_is(sp, 5, 5, 0, U({18, 41}), U()));
        CHECK(lig::plan_derived_shard(p, deal, l, 1, 1, sp));                  // rank >= world
    }
    {   // W = 2, rows 0 1 4 5 | 2 3: a rank's local rows are not a contiguous global range
        const lig::DeriveDeal deal = lig::derive_deal_of(U({0, 0, 1, 1, 0, 0}), 2);
        CHECK(deal.local_of == U({0, 1, 0, 1, 2, 3}));
        CHECK(!lig::plan_derived_shard(p, deal, l, 0, 2, sp));
        // wave 1: B reads 16, 24 of rank 1, C1 reads 10 of rank 0; wave 2: C2 reads 17 (16 was shipped in wave 1); wave 3: C3 reads 0, 11;
        // wave 4: D reads 18
        CHECK(sp.block == U({2, 1, 2, 1}) && sp.import_begin == U({0, 4, 6, 10, 12}) && sp.n_exchanges == 4);
        CHECK(sends_of(sp, 0, 0) == U({10}) && sends_of(sp, 1, 0) == U({16, 24}) && sends_of(sp, 0, 1).empty() && sends_of(sp, 1, 1) == U({17}));
        CHECK(sends_of(sp, 0, 2) == U({0, 11}) && sends_of(sp, 1, 2).empty() && sends_of(sp, 0, 3).empty() && sends_of(sp, 1, 3) == U({18}));
        CHECK(sp.sends.size() == 7);                                           // slot 16 is read across ranks in two waves and shipped once
        CHECK(sp.wave_begin == U({0, 2, 3, 3, 4}) && sp.wave_light == U({2, 1, 0, 1}));
        CHECK(target_is(sp, 0, 0, 0, U({1, 2}), U()));                         // A
        CHECK(target_is(sp, 1, 1, 0, U({1 * l + 1}), U({2, 3})));              // B: 9 is local slot 9; 16 -> 0 + 1 * 2 + 0, 24 -> 0 + 1 * 2 + 1
        CHECK(target_is(sp, 2, 1, 3, U(), U({5, 2})));                         // C2: 17 -> 4 + 1 * 1 + 0; 16 where wave 1 put it
        CHECK(target_is(sp, 3, 3, 0, U({3 * l + 1}), U({11})));                // D on local row 3: 41 -> local slot 25; 18 -> 10 + 1 * 1 + 0
        CHECK(sp.export_begin == U({0, 1, 1, 3, 3}) && sp.exports == U({1 * l + 2, 0, 1 * l + 3}));      // 10 | 0, 11 as local slots
        CHECK(sp.local_terms == 4 && sp.imported_terms == 5 && sp.n_imports == 4 && sp.n_exports == 3);
        CHECK(!lig::plan_derived_shard(p, deal, l, 1, 2, sp));
        CHECK(sp.block == U({2, 1, 2, 1}) && sp.import_begin == U({0, 4, 6, 10, 12}));      // the schedule is the same on every rank
        CHECK(sp.wave_begin == U({0, 1, 1, 2, 2}) && sp.wave_light == U({1, 0, 1, 0}));
        CHECK(target_is(sp, 0, 0, 1, U(), U({0})));                            // C1 on local row 0: 10 -> 0 + 0 * 2 + 0
        CHECK(target_is(sp, 1, 0, 2, U(), U({7, 6})));                         // C3: 11 -> 6 + 0 * 2 + 1, 0 -> 6 + 0 * 2 + 0
        CHECK(sp.export_begin == U({0, 2, 3, 3, 4}) && sp.exports == U({0, 1 * l + 0, 1, 2}));          // 16, 24 | 17 | 18 as local slots
        CHECK(sp.local_terms == 0 && sp.imported_terms == 3 && sp.n_imports == 3 && sp.n_exports == 4);
    }
    {   // W = 2, rows 0 1 2 3 | 4 5: waves 1 to 3 are local to rank 0 and have no collective, on either rank
        const lig::DeriveDeal deal = lig::derive_deal_of(U({0, 0, 0, 0, 1, 1}), 2);
        for (uint32_t r = 0; r < 2; r++) {
            CHECK(!lig::plan_derived_shard(p, deal, l, r, 2, sp));
            CHECK(sp.block == U({0, 0, 0, 1}) && sp.import_begin == U({0, 0, 0, 0, 2}) && sp.n_exchanges == 1);
            CHECK(sends_of(sp, 0, 3) == U({18}) && sp.sends.size() == 1);
        }
        CHECK(sp.wave_begin == U({0, 0, 0, 0, 1}) && target_is(sp, 0, 1, 0, U({1 * l + 1}), U({0})));
        CHECK(sp.local_terms == 1 && sp.imported_terms == 1 && sp.n_imports == 1 && sp.n_exports == 0);
    }
    {   // W = 3, rows 0 1 4 5 | none | 2 3: rank 1 was dealt no row
        const lig::DeriveDeal deal = lig::derive_deal_of(U({0, 0, 2, 2, 0, 0}), 3);
        CHECK(!lig::plan_derived_shard(p, deal, l, 1, 3, sp));
        CHECK(sp.block == U({2, 1, 2, 1}) && sp.import_begin == U({0, 6, 9, 15, 18}) && sp.n_exchanges == 4);
        CHECK(sp.targets.empty() && sp.terms.empty() && sp.exports.empty() && sp.wave_begin == U({0, 0, 0, 0, 0}) && sp.export_begin == U({0, 0, 0, 0, 0}));
        CHECK(sp.local_terms == 0 && sp.imported_terms == 0 && sp.n_imports == 0 && sp.n_exports == 0);
        for (uint32_t w = 0; w < 4; w++) CHECK(sends_of(sp, 1, w).empty());
        CHECK(sends_of(sp, 0, 0) == U({10}) && sends_of(sp, 2, 0) == U({16, 24}) && sends_of(sp, 2, 1) == U({17}) && sends_of(sp, 0, 2) == U({0, 11}) && sends_of(sp, 2, 3) == U({18}));
        CHECK(!lig::plan_derived_shard(p, deal, l, 0, 3, sp));
        CHECK(target_is(sp, 1, 1, 0, U({1 * l + 1}), U({4, 5})));              // B: 16 -> 0 + 2 * 2 + 0, 24 -> 0 + 2 * 2 + 1
        CHECK(target_is(sp, 2, 1, 3, U(), U({8, 4})));                         // C2: 17 -> 6 + 2 * 1 + 0
        CHECK(target_is(sp, 3, 3, 0, U({3 * l + 1}), U({17})));                // D: 18 -> 15 + 2 * 1 + 0
        CHECK(!lig::plan_derived_shard(p, deal, l, 2, 3, sp));
        CHECK(target_is(sp, 0, 0, 1, U(), U({0})) && target_is(sp, 1, 0, 2, U(), U({10, 9})));      // C3: 11 -> 9 + 0 * 2 + 1, 0 -> 9 + 0
    }
    {   // W = 4, rows 0 4 | 1 5 | 2 | 3: B reads two other ranks; rank 3 has a row and no target
        const lig::DeriveDeal deal = lig::derive_deal_of(U({0, 1, 2, 3, 0, 1}), 4);
        CHECK(deal.local_of == U({0, 0, 0, 0, 1, 1}));
        CHECK(!lig::plan_derived_shard(p, deal, l, 1, 4, sp));
        CHECK(sp.block == U({1, 1, 1, 1}) && sp.import_begin == U({0, 4, 8, 12, 16}) && sp.n_exchanges == 4);
        CHECK(sends_of(sp, 1, 0) == U({10}) && sends_of(sp, 2, 0) == U({16}) && sends_of(sp, 3, 0) == U({24}) && sends_of(sp, 0, 0).empty());
        CHECK(sends_of(sp, 2, 1) == U({17}) && sends_of(sp, 0, 2) == U({0}) && sends_of(sp, 1, 2) == U({11}) && sends_of(sp, 2, 3) == U({18}) && sp.sends.size() == 7);
        CHECK(sp.wave_begin == U({0, 1, 2, 2, 3}));
        CHECK(target_is(sp, 0, 0, 0, U({1}), U({2, 3})));                      // B on local row 0: 9 -> local slot 1; 16 -> 0 + 2, 24 -> 0 + 3
        CHECK(target_is(sp, 1, 0, 3, U(), U({6, 2})));                         // C2: 17 -> 4 + 2
        CHECK(target_is(sp, 2, 1, 0, U({1 * l + 1}), U({14})));                // D on local row 1: 18 -> 12 + 2
        CHECK(sp.export_begin == U({0, 1, 1, 2, 2}) && sp.exports == U({2, 3}));
        CHECK(sp.local_terms == 2 && sp.imported_terms == 5 && sp.n_imports == 4 && sp.n_exports == 2);
        CHECK(!lig::plan_derived_shard(p, deal, l, 3, 4, sp));
        CHECK(sp.targets.empty() && sp.export_begin == U({0, 1, 1, 1, 1}) && sp.exports == U({0}) && sp.n_exports == 1 && sp.n_imports == 0);
        CHECK(!lig::plan_derived_shard(p, deal, l, 2, 4, sp));
        CHECK(sp.wave_begin == U({0, 1, 1, 2, 2}) && target_is(sp, 0, 0, 1, U(), U({1})) && target_is(sp, 1, 0, 2, U(), U({9, 8})));
        uint64_t targets = 0, terms = 0;
        for (uint32_t r = 0; r < 4; r++) {
            CHECK(!lig::plan_derived_shard(p, deal, l, r, 4, sp));
            targets += sp.targets.size();
            terms += sp.local_terms + sp.imported_terms;
        }
        CHECK(targets == 6 && terms == 12);
        lig::DeriveDeal shorter = deal;                                        // a deal that does not cover the rows of the list is refused, not read past
        shorter.owner.resize(5); shorter.local_of.resize(5);
        CHECK(lig::plan_derived_shard(p, shorter, l, 0, 4, sp));
    }
    {   // light before heavy in a rank's wave, and a heavy target whose 65 terms are 33 local (row 4) and 32 imported (the 8 slots of row 3)
        Sys H;
        std::vector<lig_lin_term> big;
        for (uint32_t i = 0; i < 33; i++) { big.push_back({32 + i % 8, ONE}); if (i < 32) big.push_back({24 + i % 8, ONE}); }
        big.push_back({42, NEG});
        const uint32_t cH = H.add(big), cA2 = H.add({{1, ONE}, {0, NEG}, {2, ONE}});
        const lig_linear_system hs = H.view();
        const lig_derived_slot hd[] = {{42, cH}, {0, cA2}};
        CHECK(!lig::plan_derived(hs, kinds, ROWS, l, nullptr, hd, 2, p) && p.n_waves == 1 && p.wave_light[0] == 1);
        const lig::DeriveDeal deal = lig::derive_deal_of(U({0, 0, 1, 1, 0, 0}), 2);
        CHECK(!lig::plan_derived_shard(p, deal, l, 0, 2, sp));
        CHECK(sp.wave_begin == U({0, 2}) && sp.wave_light == U({1}) && sp.block == U({8}) && sp.import_begin == U({0, 16}));
        CHECK(sends_of(sp, 1, 0) == U({24, 25, 26, 27, 28, 29, 30, 31}) && sends_of(sp, 0, 0).empty());
        CHECK(sp.targets[0].row == 0 && sp.targets[0].col == 0 && sp.targets[1].row == 3 && sp.targets[1].col == 2);
        CHECK(sp.targets[1].mid - sp.targets[1].begin == 33 && sp.targets[1].end - sp.targets[1].mid == 32);
        for (uint32_t i = 0; i < 33; i++) CHECK(sp.terms[sp.targets[1].begin + i].slot == 2 * l + i % 8);      // row 4 is local row 2
        for (uint32_t i = 0; i < 32; i++) CHECK(sp.terms[sp.targets[1].mid + i].slot == 8 + i % 8);            // 0 + 1 * 8 + index
        CHECK(sp.local_terms == 35 && sp.imported_terms == 32 && sp.n_imports == 8);
        CHECK(!lig::plan_derived_shard(p, deal, l, 1, 2, sp));
        CHECK(sp.targets.empty() && sp.exports == U({1 * l + 0, 1 * l + 1, 1 * l + 2, 1 * l + 3, 1 * l + 4, 1 * l + 5, 1 * l + 6, 1 * l + 7}));
    }
    std::printf("derive shard plan ok\n");
    return 0;
}
