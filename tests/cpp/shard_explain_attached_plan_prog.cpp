// shard_explain_attached_plan_prog.cpp -- the host-only pieces of lig_shard_rows_explain_attached (ligero-prover_amd/csrc/explain_plan.hpp)
// as a stand-alone host program: no GPU, no library.  tests/test_shard_explain_attached_plan.py builds it with AddressSanitizer and UBSan
// and runs it.  A small world is simulated: every rank's share is a list of (ask, slot, coef) terms and the right-hand sides it holds; the
// header blocks and the padded record blocks are laid out as the ranks would send them, and the value of a term is a function of its slot.
//   the schedule   explain_header_merge + explain_record_schedule for m_r = {0, 0}, {5, 0}, {64, 65} at slice 64, a rank whose count is
//                  the maximum, W = 4 with one empty rank: M, P, the number of all-gathers, the offsets
//   the merge      explain_records_walk + explain_merge: the blocks in every rank order give the same ordered heads, the same first[] and
//                  the same permuted value list; a repeated term is kept twice; a right-hand side held by a rank with no term is found
//   the refusals   a valid record with ask >= n_asked, a valid record past m_r, a record before m_r that is not valid, two holders of one
//                  right-hand side, a non-zero reserved word, a coefficient index without presence, sum m_r >= 2^32
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../ligero-prover_amd/csrc/explain_plan.hpp"

#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

using lig::ExplainItem;
struct Rhs { uint32_t ask, coef; };
struct Rank { std::vector<ExplainItem> terms; std::vector<Rhs> rhs; };

static uint64_t value_of(uint32_t slot) { return 1000003ull * slot + 17; }

// the W header blocks as the ranks send them
static std::vector<uint32_t> headers_of(const std::vector<Rank>& world, uint64_t n_asked) {
    const uint64_t words = lig::explain_header_words(n_asked);
    std::vector<uint32_t> h(world.size() * words, 0);
    for (size_t g = 0; g < world.size(); g++) {
        h[g * words] = (uint32_t)world[g].terms.size();
        for (const Rhs& r : world[g].rhs) { h[g * words + lig::explain_header_held(r.ask)] = 1; h[g * words + lig::explain_header_held(r.ask) + 1] = r.coef; }
    }
    return h;
}
// the heads and the values of the pieces x W x P received records
static void records_of(const std::vector<Rank>& world, const lig::ExplainRecordSchedule& x, std::vector<uint32_t>& heads, std::vector<uint64_t>& values) {
    const size_t W = world.size();
    heads.assign(x.pieces * W * x.P * 4, 0);
    values.assign(x.pieces * W * x.P, 0);
    for (uint64_t j = 0; j < x.pieces; j++)
        for (size_t g = 0; g < W; g++)
            for (uint64_t r = 0; r < x.P; r++) {
                const uint64_t i = j * x.P + r, at = (j * W + g) * x.P + r;
                if (i >= world[g].terms.size()) continue;
                const ExplainItem& it = world[g].terms[i];
                heads[at * 4] = it.ask; heads[at * 4 + 1] = it.slot; heads[at * 4 + 2] = it.coef; heads[at * 4 + 3] = 1;
                values[at] = value_of(it.slot);
            }
}
struct Merged { std::vector<ExplainItem> items; std::vector<uint64_t> first, values; std::vector<uint32_t> rhs_index, rhs_coef, holder; lig::ExplainRecordSchedule x; };
// everything a rank does on the host, and the value list the permute kernel would leave; 0 ok, 1 refused by the header, 2 by the walk, 3 by the merge
static int run_world(const std::vector<Rank>& world, uint64_t n_asked, uint64_t slice, Merged& out) {
    const uint32_t W = (uint32_t)world.size();
    const std::vector<uint32_t> h = headers_of(world, n_asked);
    std::vector<uint64_t> m;
    if (!lig::explain_header_merge(h.data(), W, n_asked, m, out.rhs_index, out.rhs_coef, out.holder)) return 1;
    out.x = lig::explain_record_schedule(m, slice);
    std::vector<uint32_t> heads, perm;
    std::vector<uint64_t> values, unordered(out.x.off[W], 0);
    records_of(world, out.x, heads, values);
    // (k_explain_keep: record i of rank g -> unordered[off[g] + i])
    for (uint64_t j = 0; j < out.x.pieces; j++)
        for (uint32_t g = 0; g < W; g++)
            for (uint64_t r = 0; r < out.x.P; r++)
                if (j * out.x.P + r < m[g]) unordered[out.x.off[g] + j * out.x.P + r] = values[(j * W + g) * out.x.P + r];
    if (!lig::explain_records_walk(heads.data(), W, out.x, m, n_asked, out.items)) return 2;
    if (!lig::explain_merge(out.items, n_asked, out.first, perm)) return 3;
    if (perm.size() != out.items.size()) return 4;
    out.values.resize(perm.size());
    for (size_t i = 0; i < perm.size(); i++) { if (perm[i] >= unordered.size()) return 4; out.values[i] = unordered[perm[i]]; }
    return 0;
}
static std::vector<Rank> counts_world(const std::vector<uint64_t>& counts) {
    std::vector<Rank> world(counts.size());
    uint32_t slot = 0;
    for (size_t g = 0; g < counts.size(); g++)
        for (uint64_t i = 0; i < counts[g]; i++) world[g].terms.push_back(ExplainItem{(uint32_t)(i % 3), slot++, (uint32_t)g});
    return world;
}
static int schedule_case(const std::vector<uint64_t>& counts, uint64_t slice, uint64_t M, uint64_t P, uint64_t pieces) {
    Merged r;
    CHECK(run_world(counts_world(counts), 3, slice, r) == 0);
    CHECK(r.x.M == M && r.x.P == P && r.x.pieces == pieces);
    CHECK(r.x.off.size() == counts.size() + 1 && r.x.off[0] == 0);
    for (size_t g = 0; g < counts.size(); g++) CHECK(r.x.off[g + 1] - r.x.off[g] == counts[g]);
    CHECK(r.items.size() == r.x.off.back() && r.first.back() == r.items.size());
    std::printf("schedule");
    for (uint64_t c : counts) std::printf(" %llu", (unsigned long long)c);
    std::printf(" -> M %llu P %llu pieces %llu terms %llu\n", (unsigned long long)r.x.M, (unsigned long long)r.x.P, (unsigned long long)r.x.pieces,
                (unsigned long long)r.items.size());
    return 0;
}

int main() {
    {
        CHECK(lig::explain_header_words(0) == 4 && lig::explain_header_words(1) == 8 && lig::explain_header_words(2) == 8 && lig::explain_header_words(3) == 12);
        for (uint64_t n = 0; n < 9; n++) CHECK(lig::explain_header_words(n) % 4 == 0 && lig::explain_header_held(n) <= lig::explain_header_words(n));
        if (schedule_case({0, 0}, 64, 0, 0, 0)) return 1;                   // nothing held anywhere: no record all-gather
        if (schedule_case({5, 0}, 64, 5, 5, 1)) return 1;
        if (schedule_case({64, 65}, 64, 65, 64, 2)) return 1;               // the second piece carries one record of rank 1 and padding
        if (schedule_case({7, 200, 9}, 64, 200, 64, 4)) return 1;           // the count of the middle rank is the maximum
        if (schedule_case({10, 0, 33, 17}, 16, 33, 16, 3)) return 1;        // W = 4, rank 1 is empty
        if (schedule_case({3}, 0, 3, 1, 3)) return 1;                       // a slice of 0 counts as 1
    }
    // three ranks, four asked constraints: constraint 0 spans all ranks and holds (slot 40, coef 2) twice -- once on rank 0, once on rank 2
    // --, constraint 1 lies on rank 1 alone, constraint 2 has a right-hand side (held by rank 2, which has no term of it) and terms on rank 0,
    // constraint 3 has a right-hand side and no term anywhere (held by rank 1)
    std::vector<Rank> world(3);
    world[0].terms = {{2, 90, 0}, {0, 40, 2}, {0, 7, LIG_COEF_ONE}, {2, 3, LIG_COEF_NEG_ONE}};
    world[1].terms = {{1, 55, 1}, {0, 41, 0}, {1, 54, 1}};
    world[2].terms = {{0, 40, 2}, {0, 7, 3}};
    world[1].rhs = {{3, LIG_COEF_ONE}};
    world[2].rhs = {{2, 0}};
    {
        std::vector<int> order = {0, 1, 2};
        Merged ref;
        bool have = false;
        do {
            std::vector<Rank> w;
            for (int g : order) w.push_back(world[g]);
            for (uint64_t slice : {1ull, 2ull, 3ull, 64ull}) {
                Merged r;
                CHECK(run_world(w, 4, slice, r) == 0);
                if (!have) {
                    ref = r; have = true;
                    std::printf("items");
                    for (const ExplainItem& it : r.items) std::printf(" %u:%u:%u", it.ask, it.slot, it.coef);
                    std::printf("\nfirst");
                    for (uint64_t f : r.first) std::printf(" %llu", (unsigned long long)f);
                    std::printf("\n");
                }
                CHECK(r.items.size() == 9 && r.items.size() == ref.items.size());
                for (size_t i = 0; i < r.items.size(); i++) {
                    CHECK(!lig::explain_item_less(r.items[i], ref.items[i]) && !lig::explain_item_less(ref.items[i], r.items[i]));
                    CHECK(r.values[i] == value_of(r.items[i].slot) && r.values[i] == ref.values[i]);      // the permutation brings every value to its head
                }
                CHECK(r.first == ref.first && r.rhs_index == ref.rhs_index && r.rhs_coef == ref.rhs_coef);
                // the right-hand sides: found whichever rank holds them, with or without a term there
                CHECK(r.rhs_index == (std::vector<uint32_t>{0, 0, 3, 4}) && r.rhs_coef == (std::vector<uint32_t>{0, 0, 0, LIG_COEF_ONE}));
                CHECK(r.holder[0] == 3 && r.holder[1] == 3 && (int)r.holder[2] == (int)(std::find(order.begin(), order.end(), 2) - order.begin()));
                CHECK((int)r.holder[3] == (int)(std::find(order.begin(), order.end(), 1) - order.begin()));
            }
        } while (std::next_permutation(order.begin(), order.end()));
        // the repeated term is kept twice, next to each other; constraint 3 owns no term
        CHECK(ref.first == (std::vector<uint64_t>{0, 5, 7, 9, 9}));
        CHECK(ref.items[2].slot == 40 && ref.items[3].slot == 40 && ref.items[2].coef == 2 && ref.items[3].coef == 2 && ref.items[2].ask == 0 && ref.items[3].ask == 0);
    }
    {
        // malformed blocks
        Merged r;
        std::vector<Rank> bad = world;
        bad[1].terms[0].ask = 4;                                            // a valid record that names no asked constraint
        CHECK(run_world(bad, 4, 2, r) == 2);
        bad = world;
        bad[0].rhs = {{2, 5}};                                              // two holders of the right-hand side of constraint 2
        CHECK(run_world(bad, 4, 2, r) == 1);

        const std::vector<uint32_t> h = headers_of(world, 4);
        std::vector<uint64_t> m;
        std::vector<uint32_t> ri, rc, holder, heads, perm;
        std::vector<uint64_t> values;
        std::vector<ExplainItem> items;
        CHECK(lig::explain_header_merge(h.data(), 3, 4, m, ri, rc, holder));
        const lig::ExplainRecordSchedule x = lig::explain_record_schedule(m, 3);
        CHECK(x.M == 4 && x.P == 3 && x.pieces == 2);
        records_of(world, x, heads, values);
        CHECK(lig::explain_records_walk(heads.data(), 3, x, m, 4, items));
        std::vector<uint32_t> t = heads;
        t[((1 * 3 + 2) * 3 + 0) * 4 + 3] = 1;                               // rank 2 holds 2 records: entry 0 of its second piece lies past m_r
        CHECK(!lig::explain_records_walk(t.data(), 3, x, m, 4, items));
        t = heads;
        t[((0 * 3 + 1) * 3 + 1) * 4 + 3] = 0;                               // record 1 of rank 1 is not valid although m_r = 3
        CHECK(!lig::explain_records_walk(t.data(), 3, x, m, 4, items));
        t = heads;
        t[((0 * 3 + 1) * 3 + 1) * 4 + 3] = 2;                               // valid is 0 or 1
        CHECK(!lig::explain_records_walk(t.data(), 3, x, m, 4, items));
        std::vector<uint32_t> hb = h;
        hb[lig::explain_header_words(4) + 2] = 1;                           // a reserved word of rank 1
        CHECK(!lig::explain_header_merge(hb.data(), 3, 4, m, ri, rc, holder));
        hb = h;
        hb[lig::explain_header_held(0) + 1] = 9;                            // a coefficient index without presence
        CHECK(!lig::explain_header_merge(hb.data(), 3, 4, m, ri, rc, holder));
        hb = h;
        hb[lig::explain_header_held(1)] = 2;                                // presence is 0 or 1
        CHECK(!lig::explain_header_merge(hb.data(), 3, 4, m, ri, rc, holder));
        hb = h;
        hb[0] = 0xFFFFFFF0u; hb[lig::explain_header_words(4)] = 0x10;       // the counts add up to 2^32 and more
        CHECK(!lig::explain_header_merge(hb.data(), 3, 4, m, ri, rc, holder));
        hb[lig::explain_header_words(4)] = 0x3;                             // just below: accepted
        hb[2 * lig::explain_header_words(4)] = 0x2;
        CHECK(lig::explain_header_merge(hb.data(), 3, 4, m, ri, rc, holder) && m[0] == 0xFFFFFFF0u);
        // explain_merge refuses what explain_order refuses
        items = {{4, 0, 0}};
        std::vector<uint64_t> first;
        CHECK(!lig::explain_merge(items, 4, first, perm));
    }
    std::printf("shard explain attached plan ok\n");
    return 0;
}
