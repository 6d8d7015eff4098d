// mixed_plan_prog -- mixed rows (lig_rows_job.wide_per_row) in the host-side rules of a rows job (ligero-prover_amd/csrc/rows_plan.hpp)
// without a GPU and without the library: the offsets of a plan with mixed rows, the local view of a two-rank deal, every refusal the
// format names, and the check of the records of host rows.
// Build: g++ -std=c++17 -fsanitize=address,undefined tests/cpp/mixed_plan_prog.cpp   (tests/test_mixed_plan.py)
#include <cstdio>
#include <cstring>

#include "../../include/lig_hip.h"
#include "../../ligero-prover_amd/csrc/rows_plan.hpp"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static const uint32_t L = 317, K = 512;

int main() {
    const uint8_t F = LIG_ROW_DRAW_PAD;
    static_assert(LIG_WIDE_RECORD_BYTES == 4 + LIG_ELEM_BYTES, "a record is a column and one element");
    // linear x 3, a triple with a derived z, a full linear row, a triple of bits
    const std::vector<uint8_t> kinds = {F, F, F, (uint8_t)(1 | F), (uint8_t)(2 | F), (uint8_t)(3 | F), 0, (uint8_t)(1 | F), (uint8_t)(2 | F), (uint8_t)(3 | F)};
    const size_t R = kinds.size();
    lig_rows_job job = {};
    job.rows = R;
    job.kinds = kinds.data();
    std::vector<RowDesc> rows;
    std::vector<uint8_t> draw;
    std::vector<uint64_t> pos;
    CHECK(lig::parse_row_kinds(job, L, K, true, rows, draw, pos) == nullptr);
    const std::vector<uint8_t> eb = {LIG_ELEM_BIT, 1, 8, 2, 4, LIG_ELEM_PRODUCT, 32, LIG_ELEM_BIT, LIG_ELEM_BIT, LIG_ELEM_BIT};
    const std::vector<uint32_t> wide = {3, 0, 1, 2, L, 0, 0, 0, 5, 0};
    std::vector<size_t> all(R);
    for (size_t r = 0; r < R; r++) all[r] = r;

    // ---- one GPU.  l = 317: bits 40 bytes, bytes 320 (317 rounded up), 8 bytes 2536, 2 bytes 636 (634 rounded up), 4 bytes 1268; + 36 per record
    lig::NarrowPlan one;
    CHECK(lig::plan_narrow_rows(eb.data(), rows, draw, L, K, all, one, wide.data()) == nullptr);
    const std::vector<uint64_t> want_off = {0, 40 + 108, 148 + 320, 468 + 2536 + 36, 3040 + 636 + 72, 3748 + 1268 + 36ull * L, 16428, 16428 + 16384, 32812 + 40, 32852 + 40 + 180, 33072 + 40};
    CHECK(one.packed && one.src_off == want_off);
    CHECK(one.wide == wide);
    CHECK((one.mixed_rows == std::vector<uint32_t>{0, 2, 3, 4, 8}));
    CHECK((one.prod_rows == std::vector<uint32_t>{5}));
    for (uint64_t o : one.src_off) CHECK(o % 4 == 0);
    // the same widths without the member, with a null member and with all counts 0: today's plan, nothing mixed
    {
        lig::NarrowPlan a, b, z;
        const std::vector<uint32_t> zero(R, 0);
        CHECK(lig::plan_narrow_rows(eb.data(), rows, draw, L, K, all, a) == nullptr);
        CHECK(lig::plan_narrow_rows(eb.data(), rows, draw, L, K, all, b, nullptr) == nullptr);
        CHECK(lig::plan_narrow_rows(eb.data(), rows, draw, L, K, all, z, zero.data()) == nullptr);
        CHECK(a.src_off == b.src_off && a.src_off == z.src_off && a.wide.empty() && z.wide.empty() && z.mixed_rows.empty());
        CHECK(a.src_off.back() == want_off.back() - 36ull * (3 + 1 + 2 + L + 5));
    }
    // ---- a two-rank deal (groups stay whole): the counts are of ALL rows, a rank keeps those of its own
    const std::vector<size_t> deal[2] = {{0, 1, 6}, {2, 3, 4, 5, 7, 8, 9}};
    const std::vector<uint32_t> want_mixed[2] = {{0}, {0, 1, 2, 5}};
    for (int h = 0; h < 2; h++) {
        lig::NarrowPlan rk;
        CHECK(lig::plan_narrow_rows(eb.data(), rows, draw, L, K, deal[h], rk, wide.data()) == nullptr);
        CHECK(rk.packed && rk.wide.size() == deal[h].size() && rk.mixed_rows == want_mixed[h]);
        for (size_t lr = 0; lr < deal[h].size(); lr++) {
            CHECK(rk.wide[lr] == wide[deal[h][lr]]);
            CHECK(rk.src_off[lr + 1] - rk.src_off[lr] == one.src_off[deal[h][lr] + 1] - one.src_off[deal[h][lr]]);
        }
    }
    {   // a rank whose rows are all unmixed keeps no counts
        lig::NarrowPlan rk;
        CHECK(lig::plan_narrow_rows(eb.data(), rows, draw, L, K, {1, 6}, rk, wide.data()) == nullptr);
        CHECK(rk.packed && rk.wide.empty() && rk.mixed_rows.empty());
    }
    // ---- refusals, by every rank, whoever holds the row
    {
        lig::NarrowPlan pl;
        auto refused_everywhere = [&](const uint8_t* e, const std::vector<uint32_t>& w) {
            return lig::plan_narrow_rows(e, rows, draw, L, K, all, pl, w.data()) != nullptr && lig::plan_narrow_rows(e, rows, draw, L, K, deal[0], pl, w.data()) != nullptr &&
                   lig::plan_narrow_rows(e, rows, draw, L, K, deal[1], pl, w.data()) != nullptr;
        };
        std::vector<uint32_t> w = wide;
        w[6] = 1;                                        // on a full-width row (elem_bytes 32)
        CHECK(refused_everywhere(eb.data(), w));
        std::vector<uint8_t> e = eb;
        e[6] = 0;                                        // ... written as 0
        CHECK(refused_everywhere(e.data(), w));
        w = wide; w[5] = 1;                              // on a derived row
        CHECK(refused_everywhere(eb.data(), w));
        w = wide; w[0] = L + 1;                          // more records than data slots
        CHECK(refused_everywhere(eb.data(), w));
        w = wide; w[0] = L;                              // as many: accepted
        CHECK(lig::plan_narrow_rows(eb.data(), rows, draw, L, K, all, pl, w.data()) == nullptr);
        CHECK(refused_everywhere(nullptr, wide));        // without elem_bytes every row is full width
        const std::vector<uint32_t> zero(R, 0);
        CHECK(lig::plan_narrow_rows(nullptr, rows, draw, L, K, all, pl, zero.data()) == nullptr && !pl.packed);
        // the rules of the narrow row itself are unchanged under records: no flag, no narrow row
        std::vector<uint8_t> k2 = kinds;
        k2[0] = 0;
        lig_rows_job j2 = {};
        j2.rows = R; j2.kinds = k2.data();
        std::vector<RowDesc> r2; std::vector<uint8_t> d2; std::vector<uint64_t> p2;
        CHECK(lig::parse_row_kinds(j2, L, K, true, r2, d2, p2) == nullptr);
        CHECK(lig::plan_narrow_rows(eb.data(), r2, d2, L, K, all, pl, wide.data()) != nullptr);
    }
    // ---- the records of host rows: columns < l, strictly ascending
    {
        std::vector<uint8_t> packed(one.src_off.back(), 0xEE);
        auto put = [&](size_t row, std::vector<uint32_t> cols) {
            uint8_t* rec = packed.data() + one.src_off[row + 1] - 36 * cols.size();
            for (size_t j = 0; j < cols.size(); j++) std::memcpy(rec + 36 * j, &cols[j], 4);
        };
        std::vector<uint32_t> every(L);
        for (uint32_t i = 0; i < L; i++) every[i] = i;
        auto good = [&] { put(0, {0, 5, L - 1}); put(2, {L - 1}); put(3, {7, 8}); put(4, every); put(8, {0, 1, 2, 3, 316}); };
        auto why = [&] { return lig::wide_records_refusal(packed.data(), one.src_off, one.mixed_rows, one.wide, L); };
        good(); CHECK(why() == nullptr);
        put(2, {L}); CHECK(why() != nullptr);                       // a column == l
        good(); put(0, {0, 5, 0xFFFFFFFFu}); CHECK(why() != nullptr);
        good(); put(3, {8, 7}); CHECK(why() != nullptr);            // descending
        good(); put(3, {7, 7}); CHECK(why() != nullptr);            // twice the same
        good(); put(8, {0, 1, 2, 3, 3}); CHECK(why() != nullptr);
        good(); CHECK(why() == nullptr);
        // only the records of the rows the plan calls mixed are read: garbage anywhere else is not looked at
        lig::NarrowPlan rk;
        CHECK(lig::plan_narrow_rows(eb.data(), rows, draw, L, K, deal[0], rk, wide.data()) == nullptr);
        std::vector<uint8_t> local(rk.src_off.back(), 0xEE);
        const uint32_t cols[3] = {1, 2, 3};
        for (int j = 0; j < 3; j++) std::memcpy(local.data() + rk.src_off[1] - 108 + 36 * j, &cols[j], 4);
        CHECK(lig::wide_records_refusal(local.data(), rk.src_off, rk.mixed_rows, rk.wide, L) == nullptr);
    }
    // ---- the member is read only from a struct that says it has it: a caller built before it existed passes a struct that ends at
    // elem_bytes with reserved = 0 -- whatever lies behind it is not looked at
    {
        lig_rows_job old_style = {};
        old_style.wide_per_row = reinterpret_cast<const uint32_t*>(uintptr_t(0x10));          // never dereferenced
        CHECK(lig::job_wide_per_row(old_style) == nullptr);
        old_style.reserved = LIG_ROWS_JOB_WIDE;
        old_style.wide_per_row = wide.data();
        CHECK(lig::job_wide_per_row(old_style) == wide.data());
        old_style.reserved = 2;                                                               // some other bit
        CHECK(lig::job_wide_per_row(old_style) == nullptr);
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("mixed plan ok\n");
    return 0;
}
