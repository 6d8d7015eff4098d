// derive_plan_prog.cpp -- the host-side rules of derived slots (ligero-prover_amd/csrc/derive_plan.hpp) as a stand-alone host program: no
// GPU, no library.  tests/test_derived_slots_api.py builds it with AddressSanitizer and UBSan and runs it.  Checked here, on a system of
// 5 rows (LINEAR, QX, QY, QZ, LINEAR; l = 8) that satisfies the rules of lig_linear_check:
//   plan_derived   accepts the base list and lays the program out wave-major (targets, signs, right-hand sides, the OTHER terms in the order
//                  of the constraint, the table as passed); the empty list is the empty program; any order of the list gives the same waves
//   every refusal  a slot listed twice; a constraint >= n_constraints; a target absent from its constraint / present twice; a table index as
//                  the target's coefficient; a cycle of two; a target on a LIG_ELEM_PRODUCT row / on its QX / QY operand row
//   waves          a chain of 16 is accepted, one of 17 refused; light targets (<= DERIVE_LANE_MAX other terms) come before heavy ones
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ligero-prover_amd/csrc/derive_plan.hpp"

#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

namespace {
struct Sys {
    std::vector<uint32_t> tb{0}, rhs_c, rhs_b;
    std::vector<lig_lin_term> terms;
    std::vector<uint8_t> coefs;
    uint32_t add(std::vector<lig_lin_term> t, int rhs = -1) {
        for (const lig_lin_term& x : t) terms.push_back(x);
        tb.push_back((uint32_t)terms.size());
        if (rhs >= 0) { rhs_c.push_back((uint32_t)tb.size() - 2); rhs_b.push_back((uint32_t)rhs); }
        return (uint32_t)tb.size() - 2;
    }
    lig_linear_system view() const {
        lig_linear_system s;
        std::memset(&s, 0, sizeof s);
        s.struct_bytes = sizeof s;
        s.n_constraints = tb.size() - 1; s.n_terms = terms.size();
        s.term_begin = tb.data(); s.terms = terms.empty() ? nullptr : terms.data();
        s.rhs_constraint = rhs_c.empty() ? nullptr : rhs_c.data(); s.rhs_coef = rhs_b.empty() ? nullptr : rhs_b.data(); s.n_rhs = rhs_c.size();
        s.coefs = coefs.empty() ? nullptr : coefs.data(); s.n_coefs = coefs.size() / 32;
        return s;
    }
};
const uint32_t ONE = LIG_COEF_ONE, NEG = LIG_COEF_NEG_ONE;
const uint32_t l = 8;
const uint8_t kinds[5] = {LIG_ROW_LINEAR | LIG_ROW_DRAW_PAD, LIG_ROW_QX | LIG_ROW_DRAW_PAD, LIG_ROW_QY | LIG_ROW_DRAW_PAD, LIG_ROW_QZ | LIG_ROW_DRAW_PAD, LIG_ROW_LINEAR};
}  // namespace

int main() {
    using lig::DerivePlan;
    Sys S;
    S.coefs.assign(3 * 32, 0);
    S.coefs[0] = 1; S.coefs[32] = 7; S.coefs[64] = 9;                     // table: 1, 7, 9
    // c0: w[0] - w[8] - 7 w[16] = 9 (target 0, +1)      c1: w[1] + w[0] - w[2] = 0 (target 2, -1; reads target 0)      c2: w[33] = 7
    const uint32_t c0 = S.add({{8, NEG}, {0, ONE}, {16, 1}}, 2), c1 = S.add({{1, ONE}, {0, ONE}, {2, NEG}}), c2 = S.add({{33, ONE}}, 1);
    const uint32_t c3 = S.add({{3, 0}, {4, ONE}});                        // w[3] has the table index of the value 1
    const uint32_t c4 = S.add({{5, ONE}, {5, ONE}, {6, NEG}});            // slot 5 twice
    const uint32_t c5 = S.add({{24, NEG}, {4, ONE}}), c6 = S.add({{9, NEG}, {4, ONE}}), c7 = S.add({{17, NEG}, {4, ONE}});      // on QZ / QX / QY
    const uint32_t c8 = S.add({{34, ONE}, {35, NEG}}), c9 = S.add({{35, ONE}, {34, NEG}});      // a cycle of two
    const lig_linear_system sys = S.view();
    DerivePlan p;
    {
        const lig_derived_slot d[] = {{2, c1}, {33, c2}, {0, c0}};
        CHECK(!lig::plan_derived(sys, kinds, 5, l, nullptr, d, 3, p));
        CHECK(p.n_waves == 2 && p.wave_of == std::vector<uint32_t>({2, 1, 1}));
        CHECK(p.wave_begin == std::vector<uint32_t>({0, 2, 3}) && p.wave_light == std::vector<uint32_t>({2, 1}));
        CHECK(p.targets.size() == 3 && p.terms.size() == 4 && p.coefs == S.coefs);
        // wave 1 in list order: slot 33 (no other term, b = table entry 1), slot 0 (others 8 and 16, b = table entry 2); wave 2: slot 2
        CHECK(p.targets[0].slot == 33 && p.targets[0].negate == 0 && p.targets[0].rhs == 1 && p.targets[0].begin == p.targets[0].end);
        CHECK(p.targets[1].slot == 0 && p.targets[1].negate == 0 && p.targets[1].rhs == 2 && p.targets[1].end - p.targets[1].begin == 2);
        CHECK(p.terms[p.targets[1].begin].slot == 8 && p.terms[p.targets[1].begin].coef == NEG && p.terms[p.targets[1].begin + 1].slot == 16 && p.terms[p.targets[1].begin + 1].coef == 1);
        CHECK(p.targets[2].slot == 2 && p.targets[2].negate == 1 && p.targets[2].rhs == lig::DERIVE_RHS_ZERO && p.targets[2].end - p.targets[2].begin == 2);
        CHECK(p.terms[p.targets[2].begin].slot == 1 && p.terms[p.targets[2].begin + 1].slot == 0);
        const lig_derived_slot e[] = {{0, c0}, {2, c1}, {33, c2}};
        CHECK(!lig::plan_derived(sys, kinds, 5, l, nullptr, e, 3, p) && p.wave_of == std::vector<uint32_t>({1, 2, 1}));
        CHECK(!lig::plan_derived(sys, kinds, 5, l, nullptr, nullptr, 0, p) && p.n_waves == 0 && p.targets.empty() && p.wave_begin == std::vector<uint32_t>({0}));
        CHECK(lig::plan_derived(sys, kinds, 5, l, nullptr, nullptr, 1, p));
    }
    {   // every refusal on its own, next to the accepted neighbour
        auto one = [&](lig_derived_slot a, const uint8_t* eb = nullptr) { const lig_derived_slot d[] = {a}; return lig::plan_derived(sys, kinds, 5, l, eb, d, 1, p); };
        auto two = [&](lig_derived_slot a, lig_derived_slot b) { const lig_derived_slot d[] = {a, b}; return lig::plan_derived(sys, kinds, 5, l, nullptr, d, 2, p); };
        CHECK(!one({0, c0}));
        CHECK(two({0, c0}, {0, c0}));                                     // a slot listed twice
        CHECK(two({0, c0}, {0, c1}));                                     // ... with another constraint
        CHECK(one({0, (uint32_t)sys.n_constraints}));                     // a constraint >= n_constraints
        CHECK(one({7, c0}));                                              // absent from its constraint
        CHECK(one({5, c4}) && !one({6, c4}));                             // present twice | its neighbour in the same constraint
        CHECK(one({3, c3}) && !one({4, c3}));                             // a table index, even of the value 1
        CHECK(!one({34, c8}) && !one({35, c9}) && two({34, c8}, {35, c9}));      // a cycle of two
        CHECK(two({34, c8}, {35, c8}));                                   // ... through one constraint
        const uint8_t eb[5] = {LIG_ELEM_BIT, 1, 2, LIG_ELEM_PRODUCT, 0}, plain[5] = {LIG_ELEM_BIT, 1, 2, 4, 0};
        CHECK(one({24, c5}, eb) && !one({24, c5}, plain) && !one({24, c5}));      // on a LIG_ELEM_PRODUCT row
        CHECK(one({9, c6}, eb) && !one({9, c6}, plain));                  // on its QX operand row
        CHECK(one({17, c7}, eb) && !one({17, c7}, plain));                // on its QY operand row
        CHECK(!one({0, c0}, eb) && !one({33, c2}, eb));                   // LINEAR rows next to the triple are fine
    }
    {   // chains: slot i + 1 = slot i + slot 39 (row 4), wave i + 1; 16 waves accepted, 17 refused; and the light / heavy order of a wave
        Sys C;
        std::vector<lig_derived_slot> d;
        d.push_back({0, C.add({{0, ONE}, {39, NEG}})});
        for (uint32_t i = 1; i < 17; i++) d.push_back({i, C.add({{i - 1, ONE}, {i, NEG}, {39, ONE}})});
        std::vector<lig_lin_term> big;
        for (uint32_t i = 0; i < lig::DERIVE_LANE_MAX + 1; i++) big.push_back({32 + i % 7, ONE});
        big.push_back({20, NEG});
        const uint32_t cb = C.add(big);
        big.erase(big.begin());
        big.back().slot = 21;
        const uint32_t cl = C.add(big);
        const lig_linear_system cs = C.view();
        CHECK(!lig::plan_derived(cs, kinds, 5, l, nullptr, d.data(), 16, p) && p.n_waves == 16);
        for (uint32_t i = 0; i < 16; i++) CHECK(p.wave_of[i] == i + 1 && p.targets[i].slot == i);
        std::vector<lig_derived_slot> r(d.rbegin() + 1, d.rend());        // the same 16 listed backwards: forward references
        CHECK(!lig::plan_derived(cs, kinds, 5, l, nullptr, r.data(), 16, p) && p.n_waves == 16);
        for (uint32_t i = 0; i < 16; i++) CHECK(p.wave_of[i] == 16 - i && p.targets[i].slot == i);
        CHECK(lig::plan_derived(cs, kinds, 5, l, nullptr, d.data(), 17, p));
        const lig_derived_slot m[] = {{20, cb}, {0, d[0].constraint}, {21, cl}};      // heavy first in the list, last in its wave
        CHECK(!lig::plan_derived(cs, kinds, 5, l, nullptr, m, 3, p) && p.n_waves == 1 && p.wave_light[0] == 2);
        CHECK(p.targets[0].slot == 0 && p.targets[1].slot == 21 && p.targets[2].slot == 20);
        CHECK(p.targets[1].end - p.targets[1].begin == lig::DERIVE_LANE_MAX && p.targets[2].end - p.targets[2].begin == lig::DERIVE_LANE_MAX + 1);
    }
    std::printf("derive plan ok\n");
    return 0;
}
