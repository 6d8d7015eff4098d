// shard_explain_plan_prog.cpp -- the host-only pieces of lig_shard_rows_explain / lig_shard_rows_read_slots
// (ligero-prover_amd/csrc/explain_plan.hpp) as a stand-alone host program: no GPU, no library.  tests/test_shard_explain_plan.py builds
// it with AddressSanitizer and UBSan and runs it.  Checked here:
//   explain_items_of    the items of the asked constraints straight from a lig_linear_system, ordered by explain_order: a system with an
//                       empty constraint, a term held twice and the two special coefficient indices; asked lists that skip constraints,
//                       the empty list; ask = the position in the asked list, not the constraint number.  The ordered items are printed
//                       (one "items" line per list) and tests/test_shard_explain_plan.py restates the expected order.
//   explain_rhs_of      the right-hand side of every asked constraint by one forward walk over two ascending lists: against the plain
//                       search, for dense and sparse asked lists, lists in front of the first and behind the last right-hand side, no
//                       right-hand sides at all
//   the piece schedule  explain_piece_size / _count / _len: the sizes sum to m, every piece but the last has P entries, the last 1 .. P,
//                       m = 0 gives no piece, m = P and P +- 1, a slice of 0 counts as 1
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ligero-prover_amd/csrc/explain_plan.hpp"

#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static int schedule_ok(uint64_t m, uint64_t slice) {
    const uint64_t P = lig::explain_piece_size(m, slice), np = lig::explain_piece_count(m, P);
    CHECK(P <= m && (m == 0 || P >= 1) && P <= (slice ? slice : 1));
    CHECK((m == 0) == (np == 0));
    uint64_t sum = 0;
    for (uint64_t j = 0; j < np; j++) {
        const uint64_t len = lig::explain_piece_len(m, P, j);
        CHECK(len >= 1 && len <= P);
        CHECK(j + 1 == np || len == P);
        CHECK(j * P == sum);                             // piece j begins where the pieces before it end
        sum += len;
    }
    CHECK(sum == m);
    return 0;
}

int main() {
    using lig::ExplainItem;
    {
        // five constraints: 0 holds slot 700 twice with the same coefficient and the specials, 1 is empty, 2 one term, 3 the specials on
        // one slot in descending order, 4 two terms
        const std::vector<lig_lin_term> terms = {{700, 4}, {9, LIG_COEF_ONE}, {700, LIG_COEF_NEG_ONE}, {700, 4}, {700, 7},
                                                 {12, 0},
                                                 {5, LIG_COEF_ONE}, {5, LIG_COEF_NEG_ONE}, {5, 0}, {6, 0},
                                                 {1, 2}, {0, 1}};
        const std::vector<uint32_t> term_begin = {0, 5, 5, 6, 10, 12};
        lig_linear_system sys;
        std::memset(&sys, 0, sizeof sys);
        sys.struct_bytes = sizeof sys;
        sys.n_constraints = 5; sys.n_terms = terms.size();
        sys.term_begin = term_begin.data(); sys.terms = terms.data();
        const std::vector<std::vector<uint32_t>> lists = {{0, 1, 2, 3, 4}, {1, 3}, {0, 4}, {1}, {}};
        for (const auto& asked : lists) {
            std::vector<ExplainItem> items = {{9, 9, 9}};           // (cleared by the call)
            std::vector<uint64_t> first;
            const uint64_t m = lig::explain_items_of(sys, asked.data(), asked.size(), items);
            CHECK(lig::explain_asked_ok(asked.data(), asked.size(), sys.n_constraints));
            CHECK(m == items.size());
            uint64_t want_m = 0;
            for (uint32_t c : asked) want_m += term_begin[c + 1] - term_begin[c];
            CHECK(m == want_m);
            CHECK(lig::explain_order(items, asked.size(), first));
            CHECK(first.size() == asked.size() + 1 && first.back() == m);
            for (size_t a = 0; a < asked.size(); a++) {
                CHECK(first[a + 1] - first[a] == term_begin[asked[a] + 1] - term_begin[asked[a]]);
                for (uint64_t i = first[a]; i < first[a + 1]; i++) CHECK(items[i].ask == a);
            }
            for (size_t i = 1; i < items.size(); i++) CHECK(!lig::explain_item_less(items[i], items[i - 1]));
            std::printf("items");
            for (const ExplainItem& it : items) std::printf(" %u:%u:%u", it.ask, it.slot, it.coef);
            std::printf("\n");
        }
    }
    {
        // right-hand sides on the constraints 3 i + 1 (coefficient index 7 i), looked up for asked lists dense, sparse, in front of the
        // first, behind the last, and with no right-hand side at all: against the plain search
        const uint32_t NR = 5000, NC = 3 * NR + 50;
        std::vector<uint32_t> rhs_c(NR), rhs_b(NR);
        for (uint32_t i = 0; i < NR; i++) { rhs_c[i] = 3 * i + 1; rhs_b[i] = 7 * i; }
        lig_linear_system sys;
        std::memset(&sys, 0, sizeof sys);
        sys.struct_bytes = sizeof sys;
        sys.n_constraints = NC; sys.n_rhs = NR;
        sys.rhs_constraint = rhs_c.data(); sys.rhs_coef = rhs_b.data();
        std::vector<std::vector<uint32_t>> lists = {{0}, {1}, {0, 1, 2, 3, 4}, {3 * NR - 2}, {3 * NR - 1, 3 * NR, NC - 1}, {1, 3 * NR - 2}, {0, 700, 701, 702, 9000, NC - 1}, {}};
        std::vector<uint32_t> all(NC), third;
        for (uint32_t c = 0; c < NC; c++) { all[c] = c; if (c % 3 == 1) third.push_back(c); }
        lists.push_back(all);
        lists.push_back(third);
        for (int without = 0; without < 2; without++) {
            if (without) sys.n_rhs = 0;
            for (const auto& asked : lists) {
                std::vector<uint32_t> ri = {5}, rc = {5};
                lig::explain_rhs_of(sys, asked.data(), asked.size(), ri, rc);
                CHECK(ri.size() == asked.size() && rc.size() == asked.size());
                for (size_t a = 0; a < asked.size(); a++) {
                    const bool has = !without && asked[a] % 3 == 1 && asked[a] / 3 < NR;
                    CHECK(ri[a] == (has ? a + 1 : 0));
                    CHECK(rc[a] == (has ? 7 * (asked[a] / 3) : 0));
                }
            }
        }
    }
    {
        const uint64_t slices[] = {0, 1, 2, 7, 8, 64, 1ull << 22};
        for (uint64_t slice : slices) {
            const uint64_t P = slice ? slice : 1;
            const uint64_t ms[] = {0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P + P / 2, 193, 4201};
            for (uint64_t m : ms)
                if (schedule_ok(m, slice)) { std::printf("FAILED for m = %llu, slice = %llu\n", (unsigned long long)m, (unsigned long long)slice); return 1; }
        }
        CHECK(lig::explain_piece_size(193, 64) == 64 && lig::explain_piece_count(193, 64) == 4 && lig::explain_piece_len(193, 64, 3) == 1);
        CHECK(lig::explain_piece_size(64, 64) == 64 && lig::explain_piece_count(64, 64) == 1 && lig::explain_piece_len(64, 64, 0) == 64);
        CHECK(lig::explain_piece_size(63, 64) == 63 && lig::explain_piece_count(63, 63) == 1);
        CHECK(lig::explain_piece_size(65, 64) == 64 && lig::explain_piece_count(65, 64) == 2 && lig::explain_piece_len(65, 64, 1) == 1);
        CHECK(lig::explain_piece_size(0, 64) == 0 && lig::explain_piece_count(0, 0) == 0);
        CHECK(lig::explain_piece_size(5, 0) == 1 && lig::explain_piece_count(5, 1) == 5);
    }
    std::printf("shard explain plan ok\n");
    return 0;
}
