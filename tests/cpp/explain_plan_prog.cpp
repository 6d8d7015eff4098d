// explain_plan_prog.cpp -- the host-side rules of lig_rows_explain (ligero-prover_amd/csrc/explain_plan.hpp) as a stand-alone host
// program: no GPU, no library.  tests/test_explain_plan.py builds it with AddressSanitizer and UBSan and runs it.  Checked here:
//   explain_asked_ok   accepts strictly ascending lists below n_constraints (the empty list with a NULL pointer too), refuses duplicates,
//                      descents, an entry = n_constraints, 0xFFFFFFFF, a NULL list with a count
//   explain_slots_ok   the bound is rows * l in 64 bits
//   explain_order      the order is (ask, slot, coefficient index as an unsigned number): the specials last; equal items stay equal and
//                      adjacent; first[] are the prefix sums of the per-constraint counts, empty constraints included; whatever order the
//                      items arrive in, the result is the same bytes; an item with an ask index outside the list is refused
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../ligero-prover_amd/csrc/explain_plan.hpp"

#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main() {
    using lig::ExplainItem;
    {
        const uint32_t up[] = {0, 1, 5, 9}, dup[] = {0, 5, 5}, down[] = {3, 2}, top[] = {0xFFFFFFFFu};
        CHECK(lig::explain_asked_ok(up, 4, 10));
        CHECK(!lig::explain_asked_ok(up, 4, 9));
        CHECK(lig::explain_asked_ok(up, 3, 6));
        CHECK(!lig::explain_asked_ok(dup, 3, 10));
        CHECK(!lig::explain_asked_ok(down, 2, 10));
        CHECK(!lig::explain_asked_ok(top, 1, 0xFFFFFFFFull));
        CHECK(lig::explain_asked_ok(top, 1, 0x100000000ull));
        CHECK(lig::explain_asked_ok(nullptr, 0, 0));
        CHECK(!lig::explain_asked_ok(nullptr, 1, 10));
        CHECK(!lig::explain_asked_ok(up, 1, 0));
    }
    {
        const uint32_t s[] = {0, 3839, 3840}, big[] = {0xFFFFFFFFu};
        CHECK(lig::explain_slots_ok(s, 2, 12, 320));
        CHECK(!lig::explain_slots_ok(s, 3, 12, 320));
        CHECK(lig::explain_slots_ok(nullptr, 0, 12, 320));
        CHECK(!lig::explain_slots_ok(nullptr, 1, 12, 320));
        CHECK(!lig::explain_slots_ok(s, 1, 0, 320));
        CHECK(lig::explain_slots_ok(big, 1, 1ull << 31, 8));          // rows * l = 2^34: no 32-bit wrap
        CHECK(lig::explain_slots_ok(big, 1, 1ull << 29, 8));          // rows * l = 2^32: the last 32-bit slot is in range
        CHECK(!lig::explain_slots_ok(big, 1, (1ull << 29) - 1, 8));   // rows * l = 2^32 - 8
    }
    {
        // four asked constraints: 0 has a slot three times, 1 is empty, 2 has the specials, 3 one term
        const std::vector<ExplainItem> want = {{0, 9, LIG_COEF_ONE}, {0, 700, 4}, {0, 700, 4}, {0, 700, 7}, {0, 700, LIG_COEF_NEG_ONE},
                                               {2, 5, 0}, {2, 5, LIG_COEF_NEG_ONE}, {2, 5, LIG_COEF_ONE}, {2, 6, 0}, {3, 0, 1}};
        const std::vector<uint64_t> want_first = {0, 5, 5, 9, 10};
        std::mt19937 rng(7);
        for (int round = 0; round < 50; round++) {
            std::vector<ExplainItem> items = want;
            std::shuffle(items.begin(), items.end(), rng);
            std::vector<uint64_t> first;
            CHECK(lig::explain_order(items, 4, first));
            CHECK(first == want_first);
            CHECK(!std::memcmp(items.data(), want.data(), want.size() * sizeof(ExplainItem)));
        }
        std::vector<ExplainItem> none;
        std::vector<uint64_t> first;
        CHECK(lig::explain_order(none, 3, first) && first == std::vector<uint64_t>({0, 0, 0, 0}));
        CHECK(lig::explain_order(none, 0, first) && first == std::vector<uint64_t>({0}));
        std::vector<ExplainItem> stray = {{0, 1, 2}, {4, 1, 2}};
        CHECK(!lig::explain_order(stray, 4, first));
        CHECK(stray[0].ask == 0 && stray[1].ask == 4);
    }
    std::printf("explain plan ok\n");
    return 0;
}
