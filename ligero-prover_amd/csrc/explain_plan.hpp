// explain_plan.hpp -- the host-side rules of lig_rows_explain / lig_rows_explain_attached (lig_hip.h): which asked lists are accepted,
// the order of the term records, and where every asked constraint's records begin in that order; and of lig_shard_rows_explain /
// lig_shard_rows_read_slots: the items and right-hand sides of the asked constraints from the caller's term list, the piece schedule of
// the value exchange; and of lig_shard_rows_explain_attached: the header block of a rank, the schedule of the record all-gathers, the
// walk over the received records and their merge into the output order; and of lig_shard_rows_explain_slots* /
// lig_shard_rows_untouched_slots*: which asked slots a rank holds, its header block, the walk over the received items, the merge of the
// ranks' untouched lists.
// Host only: nothing but lig_hip.h and the standard library, so that a plain host compiler builds it (tests/cpp/explain_plan_prog.cpp,
// tests/cpp/shard_explain_plan_prog.cpp, tests/cpp/shard_explain_attached_plan_prog.cpp, tests/cpp/shard_slots_plan_prog.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/lig_hip.h"

namespace lig {
// one term of an asked constraint before it is filled in: ask = the index of its constraint in the asked list
struct ExplainItem { uint32_t ask, slot, coef; };
static_assert(sizeof(ExplainItem) == 12, "the kernels of diagnose.hip write these 12 bytes");

// strictly ascending, every entry < n_constraints (n == 0: nothing to check, the list may be NULL)
inline bool explain_asked_ok(const uint32_t* asked, uint64_t n, uint64_t n_constraints) {
    if (n && !asked) return false;
    for (uint64_t i = 0; i < n; i++) {
        if (asked[i] >= n_constraints) return false;
        if (i && asked[i] <= asked[i - 1]) return false;
    }
    return true;
}
// every slot < rows * l (compared in 64 bits: rows * l may exceed 2^32 on a trace without a linear system)
inline bool explain_slots_ok(const uint32_t* slots, uint64_t n, uint64_t rows, uint32_t l) {
    if (n && !slots) return false;
    const uint64_t end = rows * (uint64_t)l;
    for (uint64_t i = 0; i < n; i++) if (slots[i] >= end) return false;
    return true;
}
// the output order: asked constraint, slot, coefficient index as an unsigned number (LIG_COEF_NEG_ONE, LIG_COEF_ONE last).  A total
// order on the 12 bytes: two items that compare equal ARE equal, so no sort, stable or not, can tell them apart.
inline bool explain_item_less(const ExplainItem& a, const ExplainItem& b) {
    if (a.ask != b.ask) return a.ask < b.ask;
    if (a.slot != b.slot) return a.slot < b.slot;
    return a.coef < b.coef;
}
// items (any order, every ask < n_asked) -> the output order; first[i] = the index of the first item of asked constraint i,
// first[n_asked] = items.size(): constraint i owns [first[i], first[i + 1]) -- empty for a constraint without terms.
// false: an item names an ask index outside the list (nothing is reordered then).
inline bool explain_order(std::vector<ExplainItem>& items, uint64_t n_asked, std::vector<uint64_t>& first) {
    first.assign(n_asked + 1, 0);
    for (const ExplainItem& it : items) {
        if (it.ask >= n_asked) return false;
        first[(size_t)it.ask + 1]++;
    }
    for (uint64_t i = 0; i < n_asked; i++) first[i + 1] += first[i];
    std::sort(items.begin(), items.end(), explain_item_less);
    return true;
}

// ---- lig_shard_rows_explain / lig_shard_rows_read_slots: the two host-only pieces of the sharded entries.
// The items of the asked constraints straight from the caller's term list (asked has passed explain_asked_ok against sys.n_constraints,
// sys has passed lig_linear_check): what k_explain_gather writes on the one-GPU entry, without a device.  Any order of the result will do:
// explain_order sorts it.  -> m, the number of items.
inline uint64_t explain_items_of(const lig_linear_system& sys, const uint32_t* asked, uint64_t n_asked, std::vector<ExplainItem>& items) {
    uint64_t m = 0;
    for (uint64_t a = 0; a < n_asked; a++) m += sys.term_begin[asked[a] + 1] - sys.term_begin[asked[a]];
    items.clear();
    items.reserve(m);
    for (uint64_t a = 0; a < n_asked; a++)
        for (uint32_t t = sys.term_begin[asked[a]]; t < sys.term_begin[asked[a] + 1]; t++) items.push_back(ExplainItem{(uint32_t)a, sys.terms[t].slot, sys.terms[t].coef});
    return m;
}
// b_c of the asked constraints without the system's n_constraints-entry index: rhs_index[a] = a + 1 and rhs_coef[a] = the coefficient index
// of b_c when asked constraint a is in sys.rhs_constraint, rhs_index[a] = 0 (b_c = 0) when it is not -- what k_explain_finish reads per
// asked constraint.  Both lists are strictly ascending: one forward walk, galloping from the previous position (a short asked list over
// a long right-hand-side list costs the logarithm of the gaps, not a binary search over the whole list per constraint).
inline void explain_rhs_of(const lig_linear_system& sys, const uint32_t* asked, uint64_t n_asked, std::vector<uint32_t>& rhs_index, std::vector<uint32_t>& rhs_coef) {
    rhs_index.assign(n_asked, 0);
    rhs_coef.assign(n_asked, 0);
    const uint64_t NR = sys.n_rhs;
    uint64_t at = 0;                                      // every entry before `at` is below asked[a]
    for (uint64_t a = 0; a < n_asked && at < NR; a++) {
        uint64_t step = 1, hi = at;
        while (hi < NR && sys.rhs_constraint[hi] < asked[a]) { at = hi + 1; hi += step; step *= 2; }
        at = std::lower_bound(sys.rhs_constraint + at, sys.rhs_constraint + std::min(hi, NR), asked[a]) - sys.rhs_constraint;
        if (at < NR && sys.rhs_constraint[at] == asked[a]) { rhs_index[a] = (uint32_t)a + 1; rhs_coef[a] = sys.rhs_coef[at]; }
    }
}
// The values of m terms (or slots) cross the ranks in pieces of P = min(m, slice) (slice = LIG_DIAG_SLICE, at least 1): piece j covers
// [j * P, j * P + explain_piece_len(m, P, j)), every piece but the last has P entries, the last 1 .. P; m = 0: no piece.  Every piece is
// SENT at the fixed size P (the tail of the last one zeroed), so the schedule depends on m and the slice alone.
inline uint64_t explain_piece_size(uint64_t m, uint64_t slice) { return std::min<uint64_t>(m, std::max<uint64_t>(slice, 1)); }
inline uint64_t explain_piece_count(uint64_t m, uint64_t P) { return m ? (m + P - 1) / P : 0; }
inline uint64_t explain_piece_len(uint64_t m, uint64_t P, uint64_t j) { return std::min<uint64_t>(P, m - j * P); }

// ---- lig_shard_rows_explain_attached: a rank selects the asked terms of its OWN share on its device and every rank receives all of them.
// One collected term, as it crosses the ranks: the item, valid = 1 (a zeroed record, valid = 0, pads a rank's block), the canonical
// committed w of the slot.  `slot` is a slot of the WHOLE trace.
struct ExplainRecord { uint32_t ask, slot, coef, valid; uint32_t value[8]; };
static_assert(sizeof(ExplainRecord) == 48, "k_explain_collect_values writes these 48 bytes with three 16-byte stores");
// The header block of one rank, in 32-bit words (a multiple of four: 16-byte aligned blocks): word 0 = m_r, the terms the rank collected;
// words 1 .. 3 zero; then per asked constraint a the pair {held, coef}: held = 1 when the rank's slice of the right-hand sides holds b_c
// of that constraint, coef = its coefficient index then (LIG_COEF_ONE is 0xFFFFFFFF: presence cannot be folded into the index).
inline uint64_t explain_header_words(uint64_t n_asked) { return 4 + 2 * ((n_asked + 1) & ~(uint64_t)1); }
inline uint64_t explain_header_held(uint64_t a) { return 4 + 2 * a; }
// The W gathered header blocks (block g from rank g) -> m[g]; rhs_index / rhs_coef as explain_rhs_of makes them; holder[a] = the rank that
// holds b_c of asked constraint a, W when no rank does.  false, a malformed block: a non-zero reserved word, held not 0 / 1, a coefficient
// index without held, two holders of one right-hand side, sum m_r >= 2^32.
inline bool explain_header_merge(const uint32_t* blocks, uint32_t W, uint64_t n_asked, std::vector<uint64_t>& m, std::vector<uint32_t>& rhs_index,
                                 std::vector<uint32_t>& rhs_coef, std::vector<uint32_t>& holder) {
    const uint64_t words = explain_header_words(n_asked);
    m.assign(W, 0);
    rhs_index.assign(n_asked, 0);
    rhs_coef.assign(n_asked, 0);
    holder.assign(n_asked, W);
    uint64_t total = 0;
    for (uint32_t g = 0; g < W; g++) {
        const uint32_t* b = blocks + (size_t)g * words;
        if (b[1] | b[2] | b[3]) return false;
        m[g] = b[0];
        total += b[0];
        for (uint64_t a = 0; a < n_asked; a++) {
            const uint32_t held = b[explain_header_held(a)], coef = b[explain_header_held(a) + 1];
            if (held > 1 || (!held && coef)) return false;
            if (!held) continue;
            if (holder[a] != W) return false;
            holder[a] = g; rhs_index[a] = (uint32_t)a + 1; rhs_coef[a] = coef;
        }
        for (uint64_t w = explain_header_held(n_asked); w < words; w++) if (b[w]) return false;
    }
    return total < (1ull << 32);
}
// The record all-gathers: with M = max m_r and P = explain_piece_size(M, slice) there are explain_piece_count(M, P) of them, each of P
// records per rank, whatever a rank holds itself (a rank pads with zeroed records).  off[g] = the records of the ranks before g,
// off[W] = sum m_r: record i of rank g (piece i / P, entry i % P of its block) is term off[g] + i of the unordered list.
struct ExplainRecordSchedule { uint64_t M = 0, P = 0, pieces = 0; std::vector<uint64_t> off; };
inline ExplainRecordSchedule explain_record_schedule(const std::vector<uint64_t>& m, uint64_t slice) {
    ExplainRecordSchedule x;
    x.off.assign(m.size() + 1, 0);
    for (size_t g = 0; g < m.size(); g++) { x.M = std::max(x.M, m[g]); x.off[g + 1] = x.off[g] + m[g]; }
    x.P = explain_piece_size(x.M, slice);
    x.pieces = explain_piece_count(x.M, x.P);
    return x;
}
// The walk over the received records: heads = the first 16 bytes {ask, slot, coef, valid} of every record, pieces x W x P of them, piece
// major, then rank, then entry.  -> items[off[g] + i] = record i of rank g: the invalid tails are dropped.  false, a malformed block:
// a record before m_r that is not valid or names no asked constraint, a valid record past m_r.
inline bool explain_records_walk(const uint32_t* heads, uint32_t W, const ExplainRecordSchedule& x, const std::vector<uint64_t>& m, uint64_t n_asked,
                                 std::vector<ExplainItem>& items) {
    items.assign((size_t)x.off[W], ExplainItem{0, 0, 0});
    for (uint64_t j = 0; j < x.pieces; j++)
        for (uint32_t g = 0; g < W; g++)
            for (uint64_t r = 0; r < x.P; r++) {
                const uint32_t* h = heads + ((j * W + g) * x.P + r) * 4;
                const uint64_t i = j * x.P + r;
                if (i >= m[g]) { if (h[3]) return false; continue; }
                if (h[3] != 1 || h[0] >= n_asked) return false;
                items[(size_t)(x.off[g] + i)] = ExplainItem{h[0], h[1], h[2]};
            }
    return true;
}
// items (the unordered list of the walk) -> the output order (explain_order) and perm: the term at position i of the output order is term
// perm[i] of the unordered list -- where its value lies on the device.  Items that compare equal are the same term held twice: the same
// slot, hence the same value, whichever of them perm names.
inline bool explain_merge(std::vector<ExplainItem>& items, uint64_t n_asked, std::vector<uint64_t>& first, std::vector<uint32_t>& perm) {
    const std::vector<ExplainItem> src = items;
    if (!explain_order(items, n_asked, first)) return false;
    perm.resize(src.size());
    for (size_t i = 0; i < src.size(); i++) perm[i] = (uint32_t)i;
    std::sort(perm.begin(), perm.end(), [&src](uint32_t a, uint32_t b) {
        if (explain_item_less(src[a], src[b])) return true;
        if (explain_item_less(src[b], src[a])) return false;
        return a < b;
    });
    return true;
}

// ---- lig_shard_rows_explain_slots*: the terms through a slot lie in the share of the ONE rank that was dealt its row; that rank collects
// them from its own slot-major index and every rank receives all of them.
// The asked slots (of the WHOLE trace, strictly ascending, every one < rows_global * l: the entry has checked them) a rank holds:
// mine[i] = the index in the asked list, local[i] = the slot in the rank's own rows x l numbering, through local_of (global row -> local
// row, not_local for a row of another rank).  Local rows are in commit order, so local[] is strictly ascending as well.
inline void slot_asked_here(const uint32_t* slots, uint64_t n_asked, uint32_t l, const std::vector<uint32_t>& local_of, uint32_t not_local,
                            std::vector<uint32_t>& mine, std::vector<uint32_t>& local) {
    mine.clear();
    local.clear();
    for (uint64_t a = 0; a < n_asked; a++) {
        const uint32_t row = slots[a] / l, lr = row < local_of.size() ? local_of[row] : not_local;
        if (lr == not_local) continue;
        mine.push_back((uint32_t)a);
        local.push_back(lr * l + (slots[a] - row * l));
    }
}
// One collected term, as it crosses the ranks: ask = the index of its slot in the asked list, the constraint OF THE WHOLE TRACE, the
// coefficient index, valid = 1 (a zeroed item, valid = 0, pads a rank's block).
struct SlotItem { uint32_t ask, constraint, coef, valid; };
static_assert(sizeof(SlotItem) == 16, "k_slot_collect_shard writes these 16 bytes with one store");
// The header block of one rank, in 32-bit words: word 0 = m_r, the items the rank collected; words 1 .. 3 zero; then 12 words per asked
// slot a: {held, n_terms, 0, 0, value[8]} -- held = 1 when the rank was dealt the row of the slot, n_terms = the length of its segment
// and value = the canonical committed w then, all zero otherwise.  Presence is a field of its own: a committed zero is a value.
// (constexpr: k_slot_header of diagnose.hip addresses its block with slot_header_at)
constexpr uint64_t slot_header_words(uint64_t n_asked) { return 4 + 12 * n_asked; }
constexpr uint64_t slot_header_at(uint64_t a) { return 4 + 12 * a; }
// The W gathered header blocks (block g from rank g) -> m[g]; holder[a] = the one rank that holds asked slot a, n_terms[a] and
// value[8 a .. 8 a + 8) as that rank reported them.  false, a malformed block: a non-zero reserved word, held not 0 / 1, a count or a
// value without held, a slot with two holders or with none, an m_r that is not the sum of the n_terms the rank reported, sum m_r >= 2^32.
inline bool slot_header_merge(const uint32_t* blocks, uint32_t W, uint64_t n_asked, std::vector<uint64_t>& m, std::vector<uint32_t>& holder,
                              std::vector<uint32_t>& n_terms, std::vector<uint32_t>& value) {
    const uint64_t words = slot_header_words(n_asked);
    m.assign(W, 0);
    holder.assign(n_asked, W);
    n_terms.assign(n_asked, 0);
    value.assign(8 * n_asked, 0);
    uint64_t total = 0;
    for (uint32_t g = 0; g < W; g++) {
        const uint32_t* b = blocks + (size_t)g * words;
        if (b[1] | b[2] | b[3]) return false;
        m[g] = b[0];
        total += b[0];
        uint64_t sum = 0;
        for (uint64_t a = 0; a < n_asked; a++) {
            const uint32_t* h = b + slot_header_at(a);
            if (h[0] > 1 || h[2] || h[3]) return false;
            if (!h[0]) {
                for (int w = 1; w < 12; w++) if (h[w]) return false;
                continue;
            }
            if (holder[a] != W) return false;
            holder[a] = g; n_terms[a] = h[1];
            for (int w = 0; w < 8; w++) value[8 * a + w] = h[4 + w];
            sum += h[1];
        }
        if (sum != b[0]) return false;
    }
    for (uint64_t a = 0; a < n_asked; a++) if (holder[a] == W) return false;
    return total < (1ull << 32);
}
// The walk over the received items: pieces x W x P of them (the schedule of explain_record_schedule over the m_r: piece major, then rank,
// then entry).  -> items[off[g] + i] = item i of rank g as an ExplainItem whose `slot` field carries the constraint (explain_order then
// gives the output order: asked slot, constraint, coefficient index); the invalid tails are dropped.  false, a malformed block: an item
// before m_r that is not valid, a valid item past m_r, ask >= n_asked, an item for a slot another rank holds, a slot whose items do not
// add up to the n_terms its holder reported.
inline bool slot_items_walk(const SlotItem* recv, uint32_t W, const ExplainRecordSchedule& x, const std::vector<uint64_t>& m, uint64_t n_asked,
                            const std::vector<uint32_t>& holder, const std::vector<uint32_t>& n_terms, std::vector<ExplainItem>& items) {
    items.assign((size_t)x.off[W], ExplainItem{0, 0, 0});
    std::vector<uint64_t> seen(n_asked, 0);
    for (uint64_t j = 0; j < x.pieces; j++)
        for (uint32_t g = 0; g < W; g++)
            for (uint64_t r = 0; r < x.P; r++) {
                const SlotItem& h = recv[(j * W + g) * x.P + r];
                const uint64_t i = j * x.P + r;
                if (i >= m[g]) { if (h.valid) return false; continue; }
                if (h.valid != 1 || h.ask >= n_asked || holder[h.ask] != g) return false;
                seen[h.ask]++;
                items[(size_t)(x.off[g] + i)] = ExplainItem{h.ask, h.constraint, h.coef};
            }
    for (uint64_t a = 0; a < n_asked; a++) if (seen[a] != n_terms[a]) return false;
    return true;
}

// ---- lig_shard_rows_untouched_slots*: every rank lists the untouched slots of its own rows (slots of the WHOLE trace, ascending) and keeps
// its first min(cap, selected) records; the global first `cap` are among them, so merging the W lists and cutting at `cap` is exact.
// The header block of one rank: {n_untouched, n_untouched_nonzero, kept, 0} as 64-bit words.
static constexpr uint64_t UNTOUCHED_HEADER_WORDS = 4;
// The W gathered header blocks -> the two sums and kept[g].  false, a malformed block: a non-zero reserved word, more non-zero than
// untouched slots, kept != min(cap, the selected count of the rank).
inline bool untouched_header_merge(const uint64_t* blocks, uint32_t W, bool nonzero_only, uint64_t cap, uint64_t& n_untouched, uint64_t& n_nonzero,
                                   std::vector<uint64_t>& kept) {
    kept.assign(W, 0);
    n_untouched = n_nonzero = 0;
    for (uint32_t g = 0; g < W; g++) {
        const uint64_t* b = blocks + (size_t)g * UNTOUCHED_HEADER_WORDS;
        if (b[3] || b[1] > b[0] || b[0] >= (1ull << 32)) return false;
        if (b[2] != std::min<uint64_t>(cap, nonzero_only ? b[1] : b[0])) return false;
        n_untouched += b[0]; n_nonzero += b[1];
        kept[g] = b[2];
    }
    return true;
}
// The received records: pieces x W x P of them (explain_record_schedule over kept[]), record i of rank g in piece i / P, entry i % P of
// its block.  -> the first `cap` of all of them in ascending slot order.  false: a rank's list is not strictly ascending, or two ranks
// list one slot (a row has one owner).
inline bool untouched_merge(const lig_slot_value* recv, uint32_t W, const ExplainRecordSchedule& x, const std::vector<uint64_t>& kept, uint64_t cap,
                            std::vector<lig_slot_value>& out) {
    out.clear();
    const auto at = [&](uint32_t g, uint64_t i) -> const lig_slot_value& { return recv[((i / x.P) * W + g) * x.P + i % x.P]; };
    for (uint32_t g = 0; g < W; g++)
        for (uint64_t i = 1; i < kept[g]; i++) if (at(g, i).slot <= at(g, i - 1).slot) return false;
    std::vector<uint64_t> next(W, 0);
    uint64_t last = ~0ull;
    while (out.size() < cap) {
        uint32_t best = W;
        for (uint32_t g = 0; g < W; g++)
            if (next[g] < kept[g] && (best == W || at(g, next[g]).slot < at(best, next[best]).slot)) best = g;
        if (best == W) break;
        const lig_slot_value& r = at(best, next[best]++);
        if (last != ~0ull && r.slot <= last) return false;
        last = r.slot;
        out.push_back(r);
    }
    return true;
}
}  // namespace lig
