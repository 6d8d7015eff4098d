// derive_product_plan_prog.cpp -- product entries of derived slots ({slot, LIG_DERIVED_PRODUCT}; ligero-prover_amd/csrc/derive_plan.hpp) as
// a stand-alone host program: no GPU, no library.  tests/test_derived_products_api.py builds it with AddressSanitizer and UBSan and runs
// it.  The trace has 11 rows, l = 8:
//   row 0 LINEAR | 1 2 3 = QX QY QZ, z derived (triple A) | 4 5 6 = triple B, z derived | 7 8 9 = triple C, z SHIPPED | 10 LINEAR
// slot = row * 8 + column.  Checked here:
//   waves     x derived -> z (2) -> a linear target that reads z (3) and is the y operand of triple B -> its z (4) -> a last linear target
//             (5); both operands derived in different waves; a product entry without a derived operand (1); any order of the list; a
//             chain that alternates linear and product entries: 16 accepted, 17 refused
//   program   the product entries of a wave as (row, column) in list order next to the linear targets, which keep their layout; n_terms
//   refusals  each on its own next to an accepted neighbour: a product entry on a LINEAR slot, on the shipped QZ row, with elem_bytes ==
//             NULL, listed twice, next to a linear entry of the same slot; an operand target without its product entry; a cycle through a
//             product
//   shard     (hand-written deals at W = 2 and W = 3) a rank keeps the product entries of its own triples as local rows, counts 2 local terms each and imports nothing for them;
//             a re-formed z read from another rank is sent in the reader's wave; a deal that splits the triple is refused
#include <algorithm>
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
const uint32_t ONE = LIG_COEF_ONE, NEG = LIG_COEF_NEG_ONE, PROD = LIG_DERIVED_PRODUCT, l = 8, ROWS = 11;
const uint8_t D = LIG_ROW_DRAW_PAD;
const uint8_t kinds[ROWS] = {LIG_ROW_LINEAR | D, LIG_ROW_QX | D, LIG_ROW_QY | D, LIG_ROW_QZ | D, LIG_ROW_QX | D, LIG_ROW_QY | D, LIG_ROW_QZ | D,
                             LIG_ROW_QX,     LIG_ROW_QY,     LIG_ROW_QZ,     LIG_ROW_LINEAR};
const uint8_t eb[ROWS] = {LIG_ELEM_BIT, 2, LIG_ELEM_BIT, LIG_ELEM_PRODUCT, 2, 2, LIG_ELEM_PRODUCT, 2, 2, 4, 0};
uint32_t at(uint32_t row, uint32_t col) { return row * l + col; }
}  // namespace

int main() {
    using lig::DerivePlan;
    Sys S;
    // column 0, the five waves: x_A = w[0] + w[1] | z_A | y_B = z_A + w[2] | z_B | w[80] = z_B + w[3]
    const uint32_t cX = S.add({{0, ONE}, {at(1, 0), NEG}, {1, ONE}}), cT = S.add({{at(3, 0), ONE}, {2, ONE}, {at(5, 0), NEG}});
    const uint32_t cF = S.add({{at(10, 0), NEG}, {at(6, 0), ONE}, {3, ONE}});
    // column 1: x_A = w[4] (wave 1), y_A = x_A + w[5] (wave 2), z_A (wave 3)
    const uint32_t cX1 = S.add({{at(1, 1), ONE}, {4, NEG}}), cY1 = S.add({{at(1, 1), ONE}, {5, ONE}, {at(2, 1), NEG}});
    // column 2: a constraint through z_A that could define it (a linear entry on a LIG_ELEM_PRODUCT row is refused), and x_A = z_A + w[0]: a cycle
    const uint32_t cZ = S.add({{at(3, 2), NEG}, {6, ONE}}), cCyc = S.add({{at(1, 2), NEG}, {at(3, 2), ONE}, {0, ONE}});
    // column 3 of triple C (z shipped): its x may be derived without more
    const uint32_t cXC = S.add({{at(7, 3), NEG}, {7, ONE}});
    const lig_linear_system sys = S.view();
    DerivePlan p;
    auto plan = [&](const std::vector<lig_derived_slot>& d, const uint8_t* widths = eb) { return lig::plan_derived(sys, kinds, ROWS, l, widths, d.data(), d.size(), p); };
    {   // the five waves, the two-wave operands and the lone product in one list
        const std::vector<lig_derived_slot> d = {{at(10, 0), cF}, {at(3, 0), PROD}, {at(1, 0), cX}, {at(6, 0), PROD}, {at(5, 0), cT},
                                                 {at(3, 1), PROD}, {at(2, 1), cY1}, {at(1, 1), cX1}, {at(3, 2), PROD}};
        CHECK(!plan(d));
        CHECK(p.n_waves == 5 && p.wave_of == U({5, 2, 1, 4, 3, 3, 2, 1, 1}));
        // linear targets keep their layout: wave 1 {x_A col 0, x_A col 1}, wave 2 {y_A col 1}, wave 3 {y_B}, wave 4 none, wave 5 {w[80]}
        CHECK(p.wave_begin == U({0, 2, 3, 4, 4, 5}) && p.wave_light == U({2, 1, 1, 0, 1}) && p.targets.size() == 5);
        CHECK(p.targets[0].slot == at(1, 0) && p.targets[1].slot == at(1, 1) && p.targets[2].slot == at(2, 1) && p.targets[3].slot == at(5, 0) && p.targets[4].slot == at(10, 0));
        CHECK(p.terms.size() == 2 + 1 + 2 + 2 + 2 && p.n_terms() == 9 + 2 * 4);
        // product entries: wave 1 {z_A col 2}, wave 2 {z_A col 0}, wave 3 {z_A col 1}, wave 4 {z_B col 0}, wave 5 none
        CHECK(p.prod_begin == U({0, 1, 2, 3, 4, 4}) && p.products.size() == 4);
        CHECK(p.products[0].row == 3 && p.products[0].col == 2 && p.products[1].row == 3 && p.products[1].col == 0);
        CHECK(p.products[2].row == 3 && p.products[2].col == 1 && p.products[3].row == 6 && p.products[3].col == 0);
        // any order: every rotation and the reverse give the same wave per slot
        std::vector<lig_derived_slot> e = d;
        for (size_t r = 0; r <= d.size(); r++) {
            if (r == d.size()) std::reverse(e.begin(), e.end()); else std::rotate(e.begin(), e.begin() + 1, e.end());
            DerivePlan q;
            CHECK(!lig::plan_derived(sys, kinds, ROWS, l, eb, e.data(), e.size(), q) && q.n_waves == 5 && q.products.size() == 4 && q.n_terms() == 17);
            for (size_t i = 0; i < e.size(); i++)
                for (size_t j = 0; j < d.size(); j++)
                    if (e[i].slot == d[j].slot) CHECK(q.wave_of[i] == p.wave_of[j]);
        }
        // two product entries of one wave keep the order of the list
        CHECK(!plan({{at(6, 5), PROD}, {at(3, 7), PROD}, {at(3, 4), PROD}}));
        CHECK(p.n_waves == 1 && p.wave_of == U({1, 1, 1}) && p.targets.empty() && p.terms.empty() && p.wave_begin == U({0, 0}) && p.wave_light == U({0}) && p.prod_begin == U({0, 3}));
        CHECK(p.products[0].row == 6 && p.products[0].col == 5 && p.products[1].row == 3 && p.products[1].col == 7 && p.products[2].col == 4 && p.n_terms() == 6);
        CHECK(!plan({}) && p.n_waves == 0 && p.prod_begin == U({0}) && p.products.empty());
    }
    {   // every refusal on its own, next to the accepted neighbour
        CHECK(!plan({{at(3, 2), PROD}}) && p.wave_of == U({1}));              // no derived operand: wave 1
        CHECK(plan({{at(0, 2), PROD}}) && plan({{at(10, 2), PROD}}));         // on a LINEAR slot
        CHECK(plan({{at(1, 2), PROD}}) && plan({{at(2, 2), PROD}}));          // ... on the operand rows
        CHECK(plan({{at(9, 2), PROD}}));                                      // on the shipped QZ row of triple C
        CHECK(plan({{at(3, 2), PROD}}, nullptr));                             // elem_bytes == NULL
        CHECK(plan({{at(11, 0), PROD}}));                                     // beyond the rows
        CHECK(plan({{at(3, 2), PROD}, {at(3, 2), PROD}}));                    // listed twice
        CHECK(plan({{at(3, 2), PROD}, {at(3, 2), cZ}}) && plan({{at(3, 2), cZ}, {at(3, 2), PROD}}));      // a product and a linear entry of one slot
        CHECK(plan({{at(3, 2), cZ}}) && !plan({{at(3, 2), cZ}}, nullptr));    // a linear entry on the LIG_ELEM_PRODUCT row stays refused
        CHECK(plan({{at(1, 0), cX}}) && !plan({{at(1, 0), cX}, {at(3, 0), PROD}}) && p.wave_of == U({1, 2}));      // an operand target without | with its product entry
        CHECK(plan({{at(1, 0), cX}, {at(3, 1), PROD}}));                      // ... the product entry of another column does not do
        CHECK(plan({{at(1, 0), cX}, {at(6, 0), PROD}}));                      // ... nor that of another triple
        CHECK(plan({{at(2, 1), cY1}}) && !plan({{at(2, 1), cY1}, {at(3, 1), PROD}}) && p.wave_of == U({1, 2}));    // the same for a y operand
        CHECK(!plan({{at(7, 3), cXC}}));                                      // the x of a triple whose z is shipped needs none
        CHECK(plan({{at(1, 2), cCyc}, {at(3, 2), PROD}}) && plan({{at(3, 2), PROD}, {at(1, 2), cCyc}}));          // a cycle through a product
    }
    {   // a chain that alternates linear and product entries: x_j = z_(j - 1) + w[0] on triple j % 2, column j / 2; z_j its product
        Sys C;
        std::vector<lig_derived_slot> d;
        for (uint32_t j = 0; j < 8; j++) {
            const uint32_t xrow = j % 2 ? 4 : 1, col = j / 2;
            std::vector<lig_lin_term> t = {{at(xrow, col), NEG}, {0, ONE}};
            if (j) t.push_back({d.back().slot, ONE});
            d.push_back({at(xrow, col), C.add(t)});
            d.push_back({at(xrow + 2, col), PROD});
        }
        d.push_back({at(10, 0), C.add({{at(10, 0), NEG}, {d.back().slot, ONE}})});      // the 17th: reads z_7
        const lig_linear_system cs = C.view();
        CHECK(!lig::plan_derived(cs, kinds, ROWS, l, eb, d.data(), 16, p) && p.n_waves == 16);
        for (uint32_t i = 0; i < 16; i++) CHECK(p.wave_of[i] == i + 1);
        CHECK(p.targets.size() == 8 && p.products.size() == 8 && p.n_terms() == 1 + 7 * 2 + 16);
        for (uint32_t w = 0; w < 16; w++) CHECK(p.wave_begin[w + 1] - p.wave_begin[w] == (w % 2 ? 0u : 1u) && p.prod_begin[w + 1] - p.prod_begin[w] == (w % 2 ? 1u : 0u));
        std::vector<lig_derived_slot> r(d.rbegin() + 1, d.rend());            // the same 16 listed backwards: forward references
        CHECK(!lig::plan_derived(cs, kinds, ROWS, l, eb, r.data(), 16, p) && p.n_waves == 16);
        for (uint32_t i = 0; i < 16; i++) CHECK(p.wave_of[i] == 16 - i);
        CHECK(lig::plan_derived(cs, kinds, ROWS, l, eb, d.data(), 17, p));
        CHECK(!lig::plan_derived(cs, kinds, ROWS, l, eb, d.data() + 1, 16, p) && p.n_waves == 16 && p.wave_of[0] == 1 && p.wave_of[15] == 16);      // x_0 shipped: the chain starts at z_0
    }
    {   // the shard: W = 2, rows 0 .. 3 and 10 on rank 0, triples B and C on rank 1
        const std::vector<lig_derived_slot> d = {{at(10, 0), cF}, {at(3, 0), PROD}, {at(1, 0), cX}, {at(6, 0), PROD}, {at(5, 0), cT}, {at(3, 2), PROD}};
        CHECK(!plan(d) && p.n_waves == 5);
        const lig::DeriveDeal deal = lig::derive_deal_of(U({0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0}), 2);
        lig::DeriveShardPlan sp;
        CHECK(!lig::plan_derived_shard(p, deal, l, 0, 2, sp));
        // wave 3: y_B on rank 1 reads z_A (re-formed in wave 2 on rank 0) and w[2]; wave 5: w[80] on rank 0 reads z_B (wave 4, rank 1)
        CHECK(sp.block == U({0, 0, 2, 0, 1}) && sp.n_exchanges == 2 && sp.import_begin == U({0, 0, 0, 4, 4, 6}));
        CHECK(sp.exports == U({2, at(3, 0)}) && sp.export_begin == U({0, 0, 0, 2, 2, 2}));
        CHECK(sp.prod_begin == U({0, 1, 2, 2, 2, 2}) && sp.products.size() == 2 && sp.products[0].row == 3 && sp.products[0].col == 2 && sp.products[1].row == 3 && sp.products[1].col == 0);
        CHECK(sp.targets.size() == 2 && sp.local_targets() == 4 && sp.local_terms == 2 + 1 + 2 * 2 && sp.imported_terms == 1 && sp.n_imports == 1 && sp.n_exports == 2);
        CHECK(!lig::plan_derived_shard(p, deal, l, 1, 2, sp));
        CHECK(sp.block == U({0, 0, 2, 0, 1}) && sp.prod_begin == U({0, 0, 0, 0, 1, 1}) && sp.products.size() == 1 && sp.products[0].row == 2 && sp.products[0].col == 0);      // row 6 is local row 2
        CHECK(sp.targets.size() == 1 && sp.targets[0].row == 1 && sp.local_targets() == 2 && sp.local_terms == 2 && sp.imported_terms == 2 && sp.n_imports == 2);
        CHECK(sp.exports == U({at(2, 0)}) && sp.export_begin == U({0, 0, 0, 0, 0, 1}));
        CHECK(sp.terms[sp.targets[0].mid].slot == 1 && sp.terms[sp.targets[0].mid + 1].slot == 0);      // z_A at 0 + 0 * 2 + 1 (slots 2, 24 ascending), w[2] at 0
        // W = 3: row 0, triple C and row 10 on rank 0, triple A on rank 1, triple B on rank 2
        const lig::DeriveDeal three = lig::derive_deal_of(U({0, 1, 1, 1, 2, 2, 2, 0, 0, 0, 0}), 3);
        CHECK(!lig::plan_derived_shard(p, three, l, 1, 3, sp));
        // wave 1: x_A on rank 1 reads w[0], w[1] of rank 0; wave 3: y_B on rank 2 reads z_A of rank 1 and w[2] of rank 0; wave 5: w[80] reads z_B
        CHECK(sp.block == U({2, 0, 1, 0, 1}) && sp.n_exchanges == 3 && sp.import_begin == U({0, 6, 6, 9, 9, 12}));
        CHECK(sp.prod_begin == U({0, 1, 2, 2, 2, 2}) && sp.products[0].row == 2 && sp.products[0].col == 2 && sp.products[1].row == 2 && sp.products[1].col == 0);
        CHECK(sp.targets.size() == 1 && sp.targets[0].row == 0 && sp.targets[0].mid == sp.targets[0].begin && sp.terms[0].slot == 0 && sp.terms[1].slot == 1);
        CHECK(sp.local_targets() == 3 && sp.local_terms == 4 && sp.imported_terms == 2 && sp.n_imports == 2);      // the two products: 2 local terms each, nothing imported
        CHECK(sp.exports == U({at(2, 0)}) && sp.export_begin == U({0, 0, 0, 1, 1, 1}) && sp.n_exports == 1);      // z_A (local row 2) leaves in wave 3, one wave after it was re-formed
        CHECK(!lig::plan_derived_shard(p, three, l, 2, 3, sp));
        CHECK(sp.prod_begin == U({0, 0, 0, 0, 1, 1}) && sp.products[0].row == 2 && sp.products[0].col == 0 && sp.local_terms == 2 && sp.imported_terms == 2);
        CHECK(sp.targets[0].row == 1 && sp.terms[sp.targets[0].mid].slot == 7 && sp.terms[sp.targets[0].mid + 1].slot == 6);      // z_A at 6 + 1 * 1, w[2] at 6 + 0 * 1
        CHECK(sp.exports == U({at(2, 0)}) && sp.export_begin == U({0, 0, 0, 0, 0, 1}));
        CHECK(!lig::plan_derived_shard(p, three, l, 0, 3, sp));
        CHECK(sp.products.empty() && sp.targets.size() == 1 && sp.local_terms == 1 && sp.imported_terms == 1 && sp.exports == U({0, 1, 2}) && sp.export_begin == U({0, 2, 2, 3, 3, 3}));
        const lig::DeriveDeal split =lig::derive_deal_of(U({0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0}), 2);
        CHECK(lig::plan_derived_shard(p, split, l, 0, 2, sp));                 // a deal that splits triple A
    }
    std::printf("derive product plan ok\n");
    return 0;
}
