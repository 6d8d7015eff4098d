// explain_plan.hpp -- the host-side rules of lig_rows_explain / lig_rows_explain_attached (lig_hip.h): which asked lists are accepted,
// the order of the term records, and where every asked constraint's records begin in that order.
// Host only: nothing but lig_hip.h and the standard library, so that a plain host compiler builds it (tests/cpp/explain_plan_prog.cpp).
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
}  // namespace lig
