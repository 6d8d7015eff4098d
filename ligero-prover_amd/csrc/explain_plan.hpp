// explain_plan.hpp -- the host-side rules of lig_rows_explain / lig_rows_explain_attached (lig_hip.h): which asked lists are accepted,
// the order of the term records, and where every asked constraint's records begin in that order; and of lig_shard_rows_explain /
// lig_shard_rows_read_slots: the items and right-hand sides of the asked constraints from the caller's term list, the piece schedule of
// the value exchange.
// Host only: nothing but lig_hip.h and the standard library, so that a plain host compiler builds it (tests/cpp/explain_plan_prog.cpp,
// tests/cpp/shard_explain_plan_prog.cpp).
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
}  // namespace lig
