// derive_plan.hpp -- the host-side rules of derived slots (lig_hip.h: lig_derived_check, lig_rows_set_derived): which lists are accepted,
// the wave of every listed slot, and the compact constraint-major program the kernels of derive.hip walk -- per wave the targets (slot,
// sign, right-hand-side index, term range) and their OTHER terms as (slot, coefficient index) -- next to a copy of the coefficient table.
// The system has passed lig_linear_check against the same kinds: every term's slot lies on a LINEAR / QX / QY / QZ row below `rows`,
// every coefficient index is one of the two specials or < n_coefs, rows * l < 2^32.
// Host only: nothing but lig_hip.h and the standard library, so that a plain host compiler builds it (tests/cpp/derive_plan_prog.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/lig_hip.h"

namespace lig {
// A target with at most this many other terms is one lane's work (2 to 4 terms for an eval of a few witnesses, 33 for a machine word
// recomposed from bits); one with more is summed by a whole workgroup of k_derive_wave, as k_diag_lin_heavy sums a long constraint.
static constexpr uint32_t DERIVE_LANE_MAX = 64;
static constexpr uint32_t DERIVE_RHS_ZERO = 0xFFFFFFFDu;      // DeriveTarget.rhs: b_c = 0 (a coefficient index is < n_coefs <= 0xFFFFFFFD or a special)

// one derived slot of the program: w[slot] = b - sum (negate == 0: the slot has coefficient +1 in its constraint) or sum - b (negate == 1:
// coefficient -1), sum = the sum of a * w over terms [begin, end) of the program's term list, b = the table entry `rhs` (or a special)
struct DeriveTarget { uint32_t slot, negate, rhs, begin, end; };
static_assert(sizeof(DeriveTarget) == 20, "the kernel of derive.hip reads these 20 bytes");

struct DerivePlan {
    uint32_t n_waves = 0;
    std::vector<uint32_t> wave_of;        // per entry of the caller's list: 1 .. n_waves
    // wave w (0-based) owns targets [wave_begin[w], wave_begin[w + 1]): first its wave_light[w] targets with at most DERIVE_LANE_MAX other
    // terms, then the heavy ones; within each class in the order of the caller's list
    std::vector<uint32_t> wave_begin, wave_light;
    std::vector<DeriveTarget> targets;
    std::vector<lig_lin_term> terms;      // the other terms of every target, in the order of its constraint
    std::vector<uint8_t> coefs;           // sys.coefs as passed: n_coefs x 32 bytes, canonical
};

// nullptr = accepted (out is the program), else why not (out is unspecified).  d may be in any order; n == 0 is the empty program.
// elem_bytes: one per row as in lig_rows_job, or NULL (no row is derived).
inline const char* plan_derived(const lig_linear_system& sys, const uint8_t* kinds, uint64_t rows, uint32_t l, const uint8_t* elem_bytes,
                                const lig_derived_slot* d, uint64_t n, DerivePlan& out) {
    out = DerivePlan{};
    out.wave_begin.assign(1, 0);
    if (!n) return nullptr;
    if (!d) return "null list";
    if (n >= (1ull << 32)) return "too many derived slots";
    std::unordered_map<uint32_t, uint32_t> index;      // derived slot -> its entry in d
    index.reserve((size_t)n * 2);
    for (uint64_t i = 0; i < n; i++)
        if (!index.emplace(d[i].slot, (uint32_t)i).second) return "a slot is listed twice";
    std::vector<uint32_t> at(n);                        // the term of the defining constraint that is the target
    for (uint64_t i = 0; i < n; i++) {
        if (d[i].constraint >= sys.n_constraints) return "a defining constraint is not a constraint of the system";
        const uint32_t b = sys.term_begin[d[i].constraint], e = sys.term_begin[d[i].constraint + 1];
        uint32_t hits = 0;
        for (uint32_t t = b; t < e; t++)
            if (sys.terms[t].slot == d[i].slot) { hits++; at[i] = t; }
        if (hits != 1) return hits ? "a target occurs more than once in its defining constraint" : "a target does not occur in its defining constraint";
        const uint32_t coef = sys.terms[at[i]].coef;
        if (coef != LIG_COEF_ONE && coef != LIG_COEF_NEG_ONE) return "the coefficient of a target must be LIG_COEF_ONE or LIG_COEF_NEG_ONE";
        const uint64_t row = d[i].slot / l;             // < rows: the slot is a term of a checked system
        if (row >= rows) return "a target beyond the rows";
        if (elem_bytes) {
            if (elem_bytes[row] == LIG_ELEM_PRODUCT) return "a target on a LIG_ELEM_PRODUCT row";
            // the operands of a derived product are read from their packed sources: a value derived here would not reach the product
            const uint8_t kd = kinds[row] & 0x7f;
            if (kd == LIG_ROW_QX && row + 2 < rows && elem_bytes[row + 2] == LIG_ELEM_PRODUCT) return "a target is an operand slot of a LIG_ELEM_PRODUCT row";
            if (kd == LIG_ROW_QY && row + 1 < rows && elem_bytes[row + 1] == LIG_ELEM_PRODUCT) return "a target is an operand slot of a LIG_ELEM_PRODUCT row";
        }
    }
    // waves: 1 + the largest wave among the derived slots a target reads (0 for a slot that is not derived); depth-first with an explicit
    // stack, a slot met again while it is still open closes a cycle
    out.wave_of.assign(n, 0);
    std::vector<uint8_t> state(n, 0);                   // 0 untouched, 1 open, 2 done
    std::vector<std::pair<uint32_t, uint32_t>> stack;   // (entry, next term to look at)
    for (uint64_t root = 0; root < n; root++) {
        if (state[root]) continue;
        state[root] = 1;
        stack.emplace_back((uint32_t)root, sys.term_begin[d[root].constraint]);
        while (!stack.empty()) {
            const uint32_t i = stack.back().first, e = sys.term_begin[d[i].constraint + 1];
            uint32_t& t = stack.back().second;
            bool descended = false;
            for (; t < e; t++) {
                if (t == at[i]) continue;
                const auto it = index.find(sys.terms[t].slot);
                if (it == index.end()) continue;
                const uint32_t j = it->second;
                if (state[j] == 1) return "the derived slots form a cycle";
                if (state[j] == 0) { state[j] = 1; stack.emplace_back(j, sys.term_begin[d[j].constraint]); descended = true; break; }      // (t stays: looked at again when j is done)
                out.wave_of[i] = std::max(out.wave_of[i], out.wave_of[j]);
            }
            if (descended) continue;
            out.wave_of[i] += 1;
            if (out.wave_of[i] > LIG_DERIVE_MAX_WAVES) return "more than LIG_DERIVE_MAX_WAVES waves";
            state[i] = 2;
            stack.pop_back();
        }
    }
    for (uint64_t i = 0; i < n; i++) out.n_waves = std::max(out.n_waves, out.wave_of[i]);
    // the program: wave-major, light targets in front of the heavy ones
    auto others = [&](uint64_t i) { return sys.term_begin[d[i].constraint + 1] - sys.term_begin[d[i].constraint] - 1; };
    out.wave_begin.assign((size_t)out.n_waves + 1, 0);
    out.wave_light.assign(out.n_waves, 0);
    for (uint64_t i = 0; i < n; i++) {
        out.wave_begin[out.wave_of[i]]++;
        if (others(i) <= DERIVE_LANE_MAX) out.wave_light[out.wave_of[i] - 1]++;
    }
    for (uint32_t w = 0; w < out.n_waves; w++) out.wave_begin[w + 1] += out.wave_begin[w];
    std::vector<uint32_t> light_at(out.n_waves), heavy_at(out.n_waves);
    for (uint32_t w = 0; w < out.n_waves; w++) { light_at[w] = out.wave_begin[w]; heavy_at[w] = out.wave_begin[w] + out.wave_light[w]; }
    out.targets.resize(n);
    std::vector<uint32_t> entry_of(n);                  // program position -> entry of d
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t w = out.wave_of[i] - 1;
        entry_of[others(i) <= DERIVE_LANE_MAX ? light_at[w]++ : heavy_at[w]++] = (uint32_t)i;
    }
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; i++) total += others(i);
    out.terms.reserve(total);
    for (uint64_t p = 0; p < n; p++) {
        const uint32_t i = entry_of[p], c = d[i].constraint;
        DeriveTarget tg;
        tg.slot = d[i].slot;
        tg.negate = sys.terms[at[i]].coef == LIG_COEF_NEG_ONE ? 1u : 0u;
        tg.rhs = DERIVE_RHS_ZERO;
        if (sys.n_rhs) {
            const uint32_t* const rend = sys.rhs_constraint + sys.n_rhs;
            const uint32_t* rc = std::lower_bound(sys.rhs_constraint, rend, c);      // strictly ascending (lig_linear_check)
            if (rc != rend && *rc == c) tg.rhs = sys.rhs_coef[rc - sys.rhs_constraint];
        }
        tg.begin = (uint32_t)out.terms.size();
        for (uint32_t t = sys.term_begin[c]; t < sys.term_begin[c + 1]; t++)
            if (t != at[i]) out.terms.push_back(sys.terms[t]);
        tg.end = (uint32_t)out.terms.size();
        out.targets[p] = tg;
    }
    if (sys.n_coefs) out.coefs.assign(sys.coefs, sys.coefs + sys.n_coefs * 32);
    return nullptr;
}
}  // namespace lig
