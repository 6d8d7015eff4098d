// rows_plan_prog -- the host-side rules of a rows job (ligero-prover_amd/csrc/rows_plan.hpp) without a GPU and without the library:
// the kinds parser as the provers and as the verifier use it, and the narrow plan of one GPU and of a two-rank deal.
// Build: g++ -std=c++17 -fsanitize=address,undefined tests/cpp/rows_plan_prog.cpp   (tests/test_rows_plan.py)
#include <cstdio>

#include "../../include/lig_hip.h"
#include "../../ligero-prover_amd/csrc/rows_plan.hpp"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static const uint32_t L = 320, K = 512;

struct Parsed { const char* why; std::vector<RowDesc> rows; std::vector<uint8_t> draw; std::vector<uint64_t> pos; };
static Parsed parse(const std::vector<uint8_t>& kinds, bool prover, uint32_t l = L, uint32_t k = K, const std::vector<uint32_t>* dense = nullptr) {
    lig_rows_job job = {};
    job.rows = kinds.size();
    job.kinds = kinds.data();
    job.dense_rands_per_row = dense ? dense->data() : nullptr;
    Parsed p;
    p.why = lig::parse_row_kinds(job, l, k, prover, p.rows, p.draw, p.pos);
    return p;
}

int main() {
    const uint8_t F = LIG_ROW_DRAW_PAD;
    // ---- the refusal table of the rows entry (tests/test_gpu_rows_api.py: test_rows_entry_rejects_malformed_jobs), l = 320, k = 512
    const std::vector<std::vector<uint8_t>> refused = {{1, 2}, {2, 3, 0}, {0, 3}, {6}, {7, 0}, {8, 9}, {11}, {(uint8_t)(5 | F)}, {(uint8_t)(6 | F), 7}};
    for (size_t i = 0; i < refused.size(); i++) {
        CHECK(parse(refused[i], true).why != nullptr);
        // the group structure binds the verifier too; where the flag may stand is a rule of forming rows, which it does not do
        CHECK((parse(refused[i], false).why != nullptr) == (i < 7));
    }
    // ---- rules of the provers alone: refused there, accepted by the verifier, which ignores the dense counts (data = 0)
    {
        CHECK(parse({RK_INIT}, true, 300, 512).why != nullptr);               // on_batch_init draws 192 pads: k - l must be 192
        CHECK(parse({RK_INIT}, false, 300, 512).why == nullptr);
        CHECK(parse({RK_INIT}, true).why == nullptr);
        const std::vector<uint32_t> over = {K + 1}, at = {K}, one = {1};
        CHECK(parse({0}, true, L, K, &over).why != nullptr);                  // a dense count > k
        CHECK(parse({0}, true, L, K, &at).why == nullptr);
        CHECK(parse({0}, true, L, K, &at).rows[0].data == K);
        const Parsed v = parse({0}, false, L, K, &over);
        CHECK(v.why == nullptr && v.rows[0].data == 0);
        CHECK(parse({RK_BIT}, true, L, K, &one).why != nullptr);              // a dense count on a batch row
        const Parsed vb = parse({RK_BIT}, false, L, K, &one);
        CHECK(vb.why == nullptr && vb.rows[0].kind == RK_BIT && vb.rows[0].data == 0);
    }
    // ---- an accepted plan with every kind: 15 rows, pad = 192
    const std::vector<uint8_t> kinds = {F, (uint8_t)(1 | F), (uint8_t)(2 | F), (uint8_t)(3 | F), RK_INIT, RK_BIT, RK_EQX, RK_EQY, RK_BQX, RK_BQY, RK_BQZ,
                                        0, (uint8_t)(1 | F), (uint8_t)(2 | F), (uint8_t)(3 | F)};
    const size_t R = kinds.size();
    const Parsed p = parse(kinds, true);
    CHECK(p.why == nullptr);
    if (p.why) { std::printf("%s\n", p.why); return 1; }
    // linear / x / y / z and init rows take 192 elements of the encoding stream each, flagged or not; the others take none
    const std::vector<uint8_t> want_draw = {1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1};
    const std::vector<uint64_t> want_pos = {0, 192, 384, 576, 768, 960, 960, 960, 960, 960, 960, 960, 1152, 1344, 1536, 1728};
    CHECK(p.draw == want_draw);
    CHECK(p.pos == want_pos);
    for (size_t r = 0; r < R; r++) CHECK(p.rows[r].kind == (kinds[r] & 0x7f) && p.rows[r].data == 0);
    {
        const Parsed v = parse(kinds, false);
        CHECK(v.why == nullptr && v.pos == want_pos && v.rows.size() == R);
    }
    // (x, y, z) of every term, in hook order: two triples, a bit, an equality (y = ~0), a batch triple
    const std::vector<uint32_t> want_terms = {1, 2, 3, 5, 5, 5, 6, 0xFFFFFFFFu, 7, 8, 9, 10, 12, 13, 14};
    CHECK(quad_terms(p.rows) == want_terms);

    // ---- the narrow plan.  Widths: 1 byte, bits, 2 bytes, derived | eight full rows | full, 8 bytes, 4 bytes, derived
    std::vector<uint8_t> eb = {1, LIG_ELEM_BIT, 2, LIG_ELEM_PRODUCT, 0, 0, 32, 0, 0, 0, 0, 0, 8, 4, LIG_ELEM_PRODUCT};
    std::vector<size_t> all(R);
    for (size_t r = 0; r < R; r++) all[r] = r;
    lig::NarrowPlan one;
    CHECK(lig::plan_narrow_rows(eb.data(), p.rows, p.draw, L, K, all, one) == nullptr);
    CHECK(one.packed);
    // 320 one-byte slots; 320 bits = 10 dwords; 640 bytes; nothing; 8 x 512 x 32; 2560; 1280; nothing
    const std::vector<uint64_t> want_off = {0, 320, 360, 1000, 1000, 17384, 33768, 50152, 66536, 82920, 99304, 115688, 132072, 134632, 135912, 135912};
    const std::vector<uint8_t> want_w = {1, LIG_ELEM_BIT, 2, LIG_ELEM_PRODUCT, 32, 32, 32, 32, 32, 32, 32, 32, 8, 4, LIG_ELEM_PRODUCT};
    CHECK(one.src_off == want_off);
    CHECK(one.widths == want_w);
    CHECK((one.prod_rows == std::vector<uint32_t>{3, 14}));
    // a deal over two ranks that never splits a group: rank 0 holds rows 0-3 and 8-10, rank 1 rows 4-7 and 11-14
    const std::vector<size_t> deal[2] = {{0, 1, 2, 3, 8, 9, 10}, {4, 5, 6, 7, 11, 12, 13, 14}};
    const std::vector<uint32_t> want_prod[2] = {{3}, {7}};
    const std::vector<uint64_t> want_total = {1000 + 3 * 16384, 4 * 16384 + 16384 + 2560 + 1280};
    for (int h = 0; h < 2; h++) {
        lig::NarrowPlan rk;
        CHECK(lig::plan_narrow_rows(eb.data(), p.rows, p.draw, L, K, deal[h], rk) == nullptr);
        CHECK(rk.packed);
        CHECK(rk.widths.size() == deal[h].size() && rk.src_off.size() == deal[h].size() + 1 && rk.src_off[0] == 0);
        std::vector<uint32_t> prod_of_one;               // the identity plan restricted to the rank's rows
        for (size_t lr = 0; lr < deal[h].size(); lr++) {
            const size_t g = deal[h][lr];
            CHECK(rk.widths[lr] == one.widths[g]);
            CHECK(rk.src_off[lr + 1] - rk.src_off[lr] == one.src_off[g + 1] - one.src_off[g]);
            if (one.widths[g] == LIG_ELEM_PRODUCT) prod_of_one.push_back((uint32_t)lr);
        }
        CHECK(rk.prod_rows == prod_of_one);
        CHECK(rk.prod_rows == want_prod[h]);
        CHECK(rk.src_off.back() == want_total[h]);
        // the x and y of a derived local row are the two local rows in front of it
        for (uint32_t lr : rk.prod_rows) CHECK(lr >= 2 && deal[h][lr - 1] == deal[h][lr] - 1 && deal[h][lr - 2] == deal[h][lr] - 2);
    }
    // every row full width: the plain path, nothing to upload; a rank without rows of a packed job still has one width entry
    {
        const std::vector<uint8_t> full(R, 0);
        lig::NarrowPlan pl;
        CHECK(lig::plan_narrow_rows(full.data(), p.rows, p.draw, L, K, all, pl) == nullptr);
        CHECK(!pl.packed && pl.widths.empty() && pl.src_off.empty() && pl.prod_rows.empty());
        CHECK(lig::plan_narrow_rows(eb.data(), p.rows, p.draw, L, K, {}, pl) == nullptr);
        CHECK(pl.packed && pl.widths.size() == 1 && pl.src_off == std::vector<uint64_t>{0} && pl.prod_rows.empty());
    }
    // LIG_ELEM_PRODUCT off a flagged QZ row is refused -- by every rank, whoever holds the row; so are a width outside the format
    // and a narrow row that does not draw its pads or is a batch row
    {
        lig::NarrowPlan pl;
        auto refused_everywhere = [&](const std::vector<uint8_t>& e, const Parsed& q) {
            return lig::plan_narrow_rows(e.data(), q.rows, q.draw, L, K, all, pl) != nullptr &&
                   lig::plan_narrow_rows(e.data(), q.rows, q.draw, L, K, deal[0], pl) != nullptr &&
                   lig::plan_narrow_rows(e.data(), q.rows, q.draw, L, K, deal[1], pl) != nullptr;
        };
        std::vector<uint8_t> e = eb;
        e[0] = LIG_ELEM_PRODUCT;                         // on a linear row
        CHECK(refused_everywhere(e, p));
        e = eb; e[13] = LIG_ELEM_PRODUCT;                // on a QY row
        CHECK(refused_everywhere(e, p));
        e = eb; e[10] = LIG_ELEM_PRODUCT;                // on the z of a batch triple
        CHECK(refused_everywhere(e, p));
        std::vector<uint8_t> k2 = kinds;
        k2[14] = 3;                                      // the QZ row carries its own pads: not flagged
        const Parsed q = parse(k2, true);
        CHECK(q.why == nullptr && q.pos == want_pos && q.draw[14] == 0);
        CHECK(refused_everywhere(eb, q));
        e = eb; e[14] = 0;
        CHECK(lig::plan_narrow_rows(e.data(), q.rows, q.draw, L, K, all, pl) == nullptr && (pl.prod_rows == std::vector<uint32_t>{3}));
        e = eb; e[1] = 3;                                // no width of the format
        CHECK(refused_everywhere(e, p));
        e = eb; e[11] = 4;                               // a narrow linear row without LIG_ROW_DRAW_PAD
        CHECK(refused_everywhere(e, p));
        e = eb; e[5] = 1;                                // a narrow bit row
        CHECK(refused_everywhere(e, p));
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("rows plan ok\n");
    return 0;
}
