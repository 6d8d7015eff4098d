// shard_slots_plan_prog.cpp -- the host-only pieces of lig_shard_rows_explain_slots* / lig_shard_rows_untouched_slots*
// (ligero-prover_amd/csrc/explain_plan.hpp) as a stand-alone host program: no GPU, no library.  tests/test_shard_explain_slots_plan.py
// builds it with AddressSanitizer and UBSan and runs it.  A small world is simulated: a deal of rows to ranks, a statement as (slot,
// constraint, coef) terms; every rank's header block and padded item blocks are laid out as the rank would send them.
//   the holder     slot_asked_here: the asked indices a rank holds and their local slots; every asked slot has exactly one holder
//   the header     slot_header_words / slot_header_at, slot_header_merge: m_r, holder, n_terms and value of every slot -- a committed zero on
//                  a held slot is a value, not absence
//   the schedule   explain_record_schedule over the m_r: a rank with no items, m_r exactly P, a ragged last piece
//   the walk       slot_items_walk + explain_order: the output order and first[] against a direct restatement
//   the refusals   a slot with two holders, with none, a count without presence, an m_r that is not the sum of its counts, a non-zero
//                  reserved word; a valid item beyond m_r, an invalid one before it, ask >= n_asked, an item from a rank that does not hold
//                  the slot, counts that do not add up
//   the merge      untouched_header_merge + untouched_merge: W ascending lists -> the first cap of all; one rank contributes all cap
//                  records; cap = 0; a list that is not ascending, a slot listed by two ranks, a kept count that is not min(cap, selected)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <tuple>
#include <vector>

#include "../../ligero-prover_amd/csrc/explain_plan.hpp"

#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

using lig::ExplainItem;
using lig::SlotItem;
static constexpr uint32_t NOT_LOCAL = 0xFFFFFFFFu;
static constexpr uint32_t L = 10;

struct Term { uint32_t slot, constraint, coef; };
static uint32_t value_of(uint32_t slot, int w) { return slot % 7 == 0 ? 0u : 1000003u * slot + 17u * (uint32_t)w; }      // some committed zeros

// what one rank would send: its header block and its items in local collection order
struct Sent { std::vector<uint32_t> header; std::vector<SlotItem> items; };
static Sent rank_sends(const std::vector<Term>& statement, const std::vector<uint32_t>& local_of, const std::vector<uint32_t>& asked) {
    Sent s;
    std::vector<uint32_t> mine, local;
    lig::slot_asked_here(asked.data(), asked.size(), L, local_of, NOT_LOCAL, mine, local);
    s.header.assign(lig::slot_header_words(asked.size()), 0);
    for (size_t i = 0; i < mine.size(); i++) {
        uint32_t* h = s.header.data() + lig::slot_header_at(mine[i]);
        h[0] = 1;
        for (const Term& t : statement)
            if (t.slot == asked[mine[i]]) { s.items.push_back(SlotItem{mine[i], t.constraint, t.coef, 1}); h[1]++; }
        for (int w = 0; w < 8; w++) h[4 + w] = value_of(asked[mine[i]], w);
    }
    s.header[0] = (uint32_t)s.items.size();
    return s;
}
static std::vector<uint32_t> gather_headers(const std::vector<Sent>& sent) {
    std::vector<uint32_t> all;
    for (const Sent& s : sent) all.insert(all.end(), s.header.begin(), s.header.end());
    return all;
}
static std::vector<SlotItem> gather_items(const std::vector<Sent>& sent, const lig::ExplainRecordSchedule& x) {
    const size_t W = sent.size();
    std::vector<SlotItem> recv(x.pieces * W * x.P, SlotItem{0, 0, 0, 0});
    for (uint64_t j = 0; j < x.pieces; j++)
        for (size_t g = 0; g < W; g++)
            for (uint64_t r = 0; r < x.P; r++)
                if (j * x.P + r < sent[g].items.size()) recv[(j * W + g) * x.P + r] = sent[g].items[j * x.P + r];
    return recv;
}

struct World {
    std::vector<std::vector<uint32_t>> local_of;      // per rank: global row -> local row
    std::vector<Term> statement;
};
// 0: ok; 1: refused by the header merge; 2: by the walk; 3: by the order
static int run(const World& w, const std::vector<uint32_t>& asked, uint64_t slice, std::vector<ExplainItem>& items, std::vector<uint64_t>& first,
               std::vector<uint32_t>& holder, std::vector<uint32_t>& n_terms, std::vector<uint32_t>& value, lig::ExplainRecordSchedule& x,
               void (*tamper_header)(std::vector<uint32_t>&, uint64_t) = nullptr, void (*tamper_items)(std::vector<SlotItem>&, const lig::ExplainRecordSchedule&) = nullptr) {
    const uint32_t W = (uint32_t)w.local_of.size();
    std::vector<Sent> sent;
    for (uint32_t g = 0; g < W; g++) sent.push_back(rank_sends(w.statement, w.local_of[g], asked));
    std::vector<uint32_t> headers = gather_headers(sent);
    if (tamper_header) tamper_header(headers, lig::slot_header_words(asked.size()));
    std::vector<uint64_t> m;
    if (!lig::slot_header_merge(headers.data(), W, asked.size(), m, holder, n_terms, value)) return 1;
    x = lig::explain_record_schedule(m, slice);
    std::vector<SlotItem> recv = gather_items(sent, x);
    if (tamper_items) tamper_items(recv, x);
    if (!lig::slot_items_walk(recv.data(), W, x, m, asked.size(), holder, n_terms, items)) return 2;
    if (!lig::explain_order(items, asked.size(), first)) return 3;
    return 0;
}

static lig_slot_value sv(uint32_t slot) {
    lig_slot_value v;
    std::memset(&v, 0, sizeof v);
    v.slot = slot; v.row_kind = slot % 4; v.value[0] = (uint8_t)(slot * 3 + 1);
    return v;
}
// the untouched lists of the ranks -> headers and record pieces as sent; 0 ok, 1 refused by the header, 2 by the merge
static int run_untouched(const std::vector<std::vector<uint32_t>>& lists, uint64_t cap, uint64_t slice, std::vector<lig_slot_value>& out, uint64_t& un, uint64_t& nz,
                         lig::ExplainRecordSchedule& x, int tamper = 0) {
    const uint32_t W = (uint32_t)lists.size();
    std::vector<uint64_t> headers(W * lig::UNTOUCHED_HEADER_WORDS, 0), kept;
    for (uint32_t g = 0; g < W; g++) {
        uint64_t* h = headers.data() + g * lig::UNTOUCHED_HEADER_WORDS;
        h[0] = lists[g].size(); h[1] = lists[g].size() / 2; h[2] = std::min<uint64_t>(cap, lists[g].size());
    }
    if (tamper == 1) headers[2] += 1;                                  // kept != min(cap, selected)
    if (tamper == 2) headers[3] = 1;                                   // a reserved word
    if (tamper == 3) headers[1] = headers[0] + 1;                      // more non-zero than untouched
    if (!lig::untouched_header_merge(headers.data(), W, false, cap, un, nz, kept)) return 1;
    x = lig::explain_record_schedule(kept, slice);
    std::vector<lig_slot_value> recv(x.pieces * W * x.P);
    if (!recv.empty()) std::memset(recv.data(), 0, recv.size() * sizeof(lig_slot_value));
    for (uint64_t j = 0; j < x.pieces; j++)
        for (uint32_t g = 0; g < W; g++)
            for (uint64_t r = 0; r < x.P; r++)
                if (j * x.P + r < kept[g]) recv[(j * W + g) * x.P + r] = sv(lists[g][j * x.P + r]);
    return lig::untouched_merge(recv.data(), W, x, kept, cap, out) ? 0 : 2;
}

int main() {
    // ---- the layout
    CHECK(lig::slot_header_words(0) == 4 && lig::slot_header_words(3) == 40 && lig::slot_header_at(0) == 4 && lig::slot_header_at(2) == 28);
    CHECK(lig::slot_header_words(5) % 4 == 0 && lig::slot_header_at(5) % 4 == 0);      // 16-byte aligned blocks and entries
    CHECK(sizeof(SlotItem) == 16 && sizeof(lig_slot_value) == 40);

    // ---- a world of three ranks over 6 rows of L = 10 slots: rows 0, 3 -> rank 0; 1, 4, 5 -> rank 1; 2 -> rank 2
    World w;
    w.local_of = {{0, NOT_LOCAL, NOT_LOCAL, 1, NOT_LOCAL, NOT_LOCAL}, {NOT_LOCAL, 0, NOT_LOCAL, NOT_LOCAL, 1, 2}, {NOT_LOCAL, NOT_LOCAL, 0, NOT_LOCAL, NOT_LOCAL, NOT_LOCAL}};
    const uint32_t ONE = LIG_COEF_ONE, NEG = LIG_COEF_NEG_ONE;
    w.statement = {{3, 9, 2}, {3, 4, ONE}, {3, 4, 1}, {3, 4, 1}, {12, 9, 0}, {35, 1, NEG}, {35, 0, 5}, {41, 9, 2}, {59, 7, 3}, {59, 2, 3}, {21, 4, 0}};
    for (uint32_t c = 0; c < 70; c++) w.statement.push_back(Term{14, 100 + c % 9, c % 3});      // slot 14 (rank 1, a zero value: 14 % 7 == 0): 70 terms
    {
        // the holder of a slot
        const std::vector<uint32_t> asked = {3, 12, 14, 21, 30, 35, 41, 59};
        std::vector<uint32_t> mine, local;
        lig::slot_asked_here(asked.data(), asked.size(), L, w.local_of[0], NOT_LOCAL, mine, local);
        CHECK((mine == std::vector<uint32_t>{0, 4, 5}) && (local == std::vector<uint32_t>{3, 10, 15}));
        lig::slot_asked_here(asked.data(), asked.size(), L, w.local_of[1], NOT_LOCAL, mine, local);
        CHECK((mine == std::vector<uint32_t>{1, 2, 6, 7}) && (local == std::vector<uint32_t>{2, 4, 11, 29}));
        lig::slot_asked_here(asked.data(), asked.size(), L, w.local_of[2], NOT_LOCAL, mine, local);
        CHECK((mine == std::vector<uint32_t>{3}) && (local == std::vector<uint32_t>{1}));
        CHECK(std::is_sorted(local.begin(), local.end()));

        // the whole host side at several slices: the same items, first[], holders, counts and values whatever the pieces are
        std::vector<ExplainItem> want;
        for (size_t a = 0; a < asked.size(); a++) for (const Term& t : w.statement) if (t.slot == asked[a]) want.push_back(ExplainItem{(uint32_t)a, t.constraint, t.coef});
        std::sort(want.begin(), want.end(), lig::explain_item_less);
        // m_r = {4 + 2, 1 + 70 + 1 + 2, 1} = {6, 74, 1}
        struct Sched { uint64_t slice, P, pieces; };
        for (const Sched& sc : {Sched{1 << 20, 74, 1}, Sched{74, 74, 1}, Sched{37, 37, 2}, Sched{32, 32, 3}, Sched{1, 1, 74}, Sched{0, 1, 74}}) {
            std::vector<ExplainItem> items;
            std::vector<uint64_t> first;
            std::vector<uint32_t> holder, n_terms, value;
            lig::ExplainRecordSchedule x;
            CHECK(run(w, asked, sc.slice, items, first, holder, n_terms, value, x) == 0);
            std::printf("schedule slice %llu -> M %llu P %llu pieces %llu terms %llu\n", (unsigned long long)sc.slice, (unsigned long long)x.M, (unsigned long long)x.P,
                        (unsigned long long)x.pieces, (unsigned long long)x.off[3]);
            CHECK(x.M == 74 && x.P == sc.P && x.pieces == sc.pieces && x.off[3] == 81);
            CHECK(items.size() == want.size());
            for (size_t i = 0; i < want.size(); i++) CHECK(items[i].ask == want[i].ask && items[i].slot == want[i].slot && items[i].coef == want[i].coef);
            CHECK((holder == std::vector<uint32_t>{0, 1, 1, 2, 0, 0, 1, 1}));
            CHECK((n_terms == std::vector<uint32_t>{4, 1, 70, 1, 0, 2, 1, 2}));
            CHECK((first == std::vector<uint64_t>{0, 4, 5, 75, 76, 76, 78, 79, 81}));
            for (size_t a = 0; a < asked.size(); a++) for (int k = 0; k < 8; k++) CHECK(value[8 * a + k] == value_of(asked[a], k));
            CHECK(value[8 * 2] == 0 && value[8 * 2 + 7] == 0 && holder[2] == 1);      // a held slot whose committed value is zero
            if (sc.slice == 32) {
                std::printf("items");
                for (const ExplainItem& it : items) if (it.ask != 2) std::printf(" %u:%u:%u", it.ask, it.slot, it.coef);
                std::printf("\nfirst");
                for (uint64_t f : first) std::printf(" %llu", (unsigned long long)f);
                std::printf("\n");
            }
        }
        // a repeated term is kept twice, in place
        CHECK(want[0].slot == 4 && want[0].coef == 1 && want[1].slot == 4 && want[1].coef == 1 && want[2].slot == 4 && want[2].coef == ONE && want[3].slot == 9);

        // ---- the refusals of the header
        std::vector<ExplainItem> items;
        std::vector<uint64_t> first;
        std::vector<uint32_t> holder, n_terms, value;
        lig::ExplainRecordSchedule x;
        // two holders: rank 2's block claims slot index 0 as well (with no terms, so its m_r still adds up)
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x, [](std::vector<uint32_t>& h, uint64_t words) { h[2 * words + lig::slot_header_at(0)] = 1; }) == 1);
        // no holder: rank 2 drops its only slot (and its one item)
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x, [](std::vector<uint32_t>& h, uint64_t words) {
                  for (int k = 0; k < 12; k++) h[2 * words + lig::slot_header_at(3) + k] = 0;
                  h[2 * words] = 0;
              }) == 1);
        // a count without presence; a value without presence
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x, [](std::vector<uint32_t>& h, uint64_t words) { h[2 * words + lig::slot_header_at(0) + 1] = 1; }) == 1);
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x, [](std::vector<uint32_t>& h, uint64_t words) { h[2 * words + lig::slot_header_at(0) + 11] = 5; }) == 1);
        // m_r is not the sum of the counts the rank reports
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x, [](std::vector<uint32_t>& h, uint64_t) { h[0] += 1; }) == 1);
        // held = 2; a reserved word of the block; a reserved word of an entry
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x, [](std::vector<uint32_t>& h, uint64_t) { h[lig::slot_header_at(0)] = 2; }) == 1);
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x, [](std::vector<uint32_t>& h, uint64_t) { h[2] = 1; }) == 1);
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x, [](std::vector<uint32_t>& h, uint64_t) { h[lig::slot_header_at(0) + 3] = 1; }) == 1);
        // ---- the refusals of the walk (pieces of 32: rank 0 has 6 items, rank 2 one, rank 1 fills two pieces and ten entries of the third)
        // a valid item beyond m_r (rank 0, entry 6 of piece 0)
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x, nullptr, [](std::vector<SlotItem>& r, const lig::ExplainRecordSchedule& s) { r[(0 * 3 + 0) * s.P + 6] = SlotItem{0, 4, 1, 1}; }) == 2);
        // ... and in a later piece, where rank 0 has nothing at all
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x, nullptr, [](std::vector<SlotItem>& r, const lig::ExplainRecordSchedule& s) { r[(2 * 3 + 0) * s.P + 0] = SlotItem{0, 4, 1, 1}; }) == 2);
        // an item before m_r that is not valid; valid = 2
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x, nullptr, [](std::vector<SlotItem>& r, const lig::ExplainRecordSchedule&) { r[0].valid = 0; }) == 2);
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x, nullptr, [](std::vector<SlotItem>& r, const lig::ExplainRecordSchedule&) { r[0].valid = 2; }) == 2);
        // ask >= n_asked
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x, nullptr, [](std::vector<SlotItem>& r, const lig::ExplainRecordSchedule&) { r[0].ask = 8; }) == 2);
        // an item for a slot another rank holds (rank 0 sends one for asked index 1, which rank 1 holds)
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x, nullptr, [](std::vector<SlotItem>& r, const lig::ExplainRecordSchedule&) { r[0].ask = 1; }) == 2);
        // counts that do not add up: rank 0 sends an item of asked index 0 under index 5 (it holds both)
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x, nullptr, [](std::vector<SlotItem>& r, const lig::ExplainRecordSchedule&) { r[0].ask = 5; }) == 2);
        // untampered once more
        CHECK(run(w, asked, 32, items, first, holder, n_terms, value, x) == 0 && items.size() == 81);
    }
    {
        // a rank with no items; no items at all (no piece); m_r exactly P
        std::vector<ExplainItem> items;
        std::vector<uint64_t> first;
        std::vector<uint32_t> holder, n_terms, value;
        lig::ExplainRecordSchedule x;
        CHECK(run(w, {3, 35, 59}, 6, items, first, holder, n_terms, value, x) == 0);          // m_r = {6, 2, 0}: rank 0 fills the one piece exactly
        std::printf("schedule slice 6 -> M %llu P %llu pieces %llu terms %llu\n", (unsigned long long)x.M, (unsigned long long)x.P, (unsigned long long)x.pieces, (unsigned long long)x.off[3]);
        CHECK(x.M == 6 && x.P == 6 && x.pieces == 1 && x.off[3] == 8 && (first == std::vector<uint64_t>{0, 4, 6, 8}));
        CHECK(run(w, {3, 35, 59}, 3, items, first, holder, n_terms, value, x) == 0 && x.P == 3 && x.pieces == 2 && items.size() == 8);      // M an exact multiple of P
        CHECK(run(w, {22, 30, 31}, 64, items, first, holder, n_terms, value, x) == 0);
        std::printf("schedule slice 64 -> M %llu P %llu pieces %llu terms %llu\n", (unsigned long long)x.M, (unsigned long long)x.P, (unsigned long long)x.pieces, (unsigned long long)x.off[3]);
        CHECK(x.M == 0 && x.P == 0 && x.pieces == 0 && items.empty() && (first == std::vector<uint64_t>{0, 0, 0, 0}) && (holder == std::vector<uint32_t>{2, 0, 0}));
        CHECK(run(w, {}, 64, items, first, holder, n_terms, value, x) == 0 && x.pieces == 0 && first.size() == 1);
        // a slot beyond the deal's rows has no holder
        CHECK(run(w, {3, 60}, 64, items, first, holder, n_terms, value, x) == 1);
    }

    // ---- the W-way merge of untouched lists
    {
        std::vector<lig_slot_value> out;
        uint64_t un = 0, nz = 0;
        lig::ExplainRecordSchedule x;
        const std::vector<std::vector<uint32_t>> lists = {{5, 6, 7, 30, 31, 90}, {}, {1, 2, 8, 9, 40, 41, 42, 43, 44}, {3, 100}};
        std::vector<uint32_t> all;
        for (const auto& li : lists) all.insert(all.end(), li.begin(), li.end());
        std::sort(all.begin(), all.end());
        for (uint64_t cap : {0ull, 1ull, 4ull, 9ull, 16ull, 17ull, 22ull}) {
            for (uint64_t slice : {1ull << 20, 4ull, 3ull, 1ull}) {
                CHECK(run_untouched(lists, cap, slice, out, un, nz, x) == 0);
                CHECK(un == 17 && nz == 3 + 0 + 4 + 1);
                const uint64_t M = std::min<uint64_t>(cap, 9), P = std::min<uint64_t>(M, slice);
                CHECK(x.M == M && x.P == P && x.pieces == (M ? (M + P - 1) / P : 0));
                CHECK(out.size() == std::min<uint64_t>(cap, 17));
                for (size_t i = 0; i < out.size(); i++) { const lig_slot_value v = sv(all[i]); CHECK(!std::memcmp(&out[i], &v, sizeof v)); }
            }
            std::printf("merge cap %llu -> %zu", (unsigned long long)cap, out.size());
            for (const lig_slot_value& v : out) std::printf(" %u", v.slot);
            std::printf("\n");
        }
        // one rank contributes all cap records: the others' first slots come later
        const std::vector<std::vector<uint32_t>> one = {{50, 51}, {1, 2, 3, 4, 5, 6}, {60}};
        CHECK(run_untouched(one, 4, 3, out, un, nz, x) == 0 && un == 9 && out.size() == 4 && x.M == 4 && x.P == 3 && x.pieces == 2);
        CHECK(out[0].slot == 1 && out[3].slot == 4);
        // cap = 0: the counts alone, no piece
        CHECK(run_untouched(one, 0, 3, out, un, nz, x) == 0 && un == 9 && out.empty() && x.pieces == 0);
        // refusals
        CHECK(run_untouched(one, 4, 3, out, un, nz, x, 1) == 1 && run_untouched(one, 4, 3, out, un, nz, x, 2) == 1 && run_untouched(one, 4, 3, out, un, nz, x, 3) == 1);
        CHECK(run_untouched({{5, 4}, {1}}, 8, 3, out, un, nz, x) == 2);                   // a list that is not ascending
        CHECK(run_untouched({{4, 4}, {1}}, 8, 3, out, un, nz, x) == 2);                   // ... or repeats a slot
        CHECK(run_untouched({{4, 9}, {1, 9}}, 8, 3, out, un, nz, x) == 2);                // a slot two ranks list
    }
    std::printf("shard slots plan ok\n");
    return 0;
}
