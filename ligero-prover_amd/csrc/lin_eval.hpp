// lin_eval.hpp -- sum_j a_j * w[slot_j] over a constraint-major term list, evaluated on the expanded message matrix: the device code the
// linear pass of diagnose.hip (the residual of every constraint) and the waves of derive.hip (the value of a derived slot) share.
#pragma once
#include "../../include/lig_hip.h"
#include "lin_common.hpp"

namespace lig {
// n / d for n < 2^32 and the launch-uniform d >= 1: m = floor(2^64 / d) + 1 (host: lin_reciprocal), exact because n * (m d - 2^64) < 2^64
static __device__ __forceinline__ uint32_t diag_div(uint32_t n, uint64_t m) { return (uint32_t)__umul64hi((uint64_t)n, m); }
inline uint64_t lin_reciprocal(uint32_t d) { return d <= 1 ? ~0ull : ~0ull / d + 1; }       // floor(2^64 / d) + 1 (d = 1 is never used: l >= 2)

static __device__ __forceinline__ fr diag_one() {
    fr o = fr_zero();
    o.v[0] = 1;
    return o;
}
// where the row a term names lies in `msgs`: the whole matrix (one GPU), or a rank's share through its global -> local row table
// (LIN_NOT_LOCAL: another rank holds that row)
struct DiagAllRows { __device__ __forceinline__ uint32_t operator()(uint32_t row) const { return row; } };
struct DiagLocalRows { const uint32_t* __restrict__ local_of; __device__ __forceinline__ uint32_t operator()(uint32_t row) const { return local_of[row]; } };
// acc (canonical) += a * w for the coefficient index `coef` and the canonical witness value w
static __device__ __forceinline__ fr diag_apply(const fr& acc, uint32_t coef, const fr& w, const fr* __restrict__ coef_mont) {
    if (coef == LIG_COEF_ONE) return fr_add(acc, w);
    if (coef == LIG_COEF_NEG_ONE) return fr_sub(acc, w);
    return fr_add(acc, fr_montmul(w, fr_load(coef_mont + coef)));         // w * (a R) / R = a * w, canonical
}
// acc (canonical) += coef * w[slot] for one term (unchanged for a term whose row is not in `msgs`)
template <class Rows>
static __device__ __forceinline__ fr diag_accumulate(const fr& acc, const lig_lin_term tm, const fr* __restrict__ msgs, uint32_t l, uint32_t k, uint64_t l_recip,
                                                     const fr* __restrict__ coef_mont, const Rows rows) {
    const uint32_t grow = diag_div(tm.slot, l_recip), col = tm.slot - grow * l, row = rows(grow);
    if (row == LIN_NOT_LOCAL) return acc;
    return diag_apply(acc, tm.coef, fr_load(msgs + (size_t)row * k + col), coef_mont);
}
// a term list whose `slot` is already an element of `msgs` -- a rank's import buffer on a rows shard (derive.hip): no row, no division
struct DiagFlat {};
static __device__ __forceinline__ fr diag_accumulate(const fr& acc, const lig_lin_term tm, const fr* __restrict__ msgs, uint32_t, uint32_t, uint64_t,
                                                     const fr* __restrict__ coef_mont, const DiagFlat) {
    return diag_apply(acc, tm.coef, fr_load(msgs + tm.slot), coef_mont);
}
// the canonical value a coefficient index stands for
static __device__ __forceinline__ fr diag_coef_value(uint32_t coef, const fr* __restrict__ coef_mont) {
    if (coef == LIG_COEF_ONE) return diag_one();
    if (coef == LIG_COEF_NEG_ONE) return fr_neg(diag_one());
    return fr_montmul(fr_load(coef_mont + coef), diag_one());             // (a R) * 1 / R = a
}
// the one walk over terms of a constraint: acc += the terms b, b + step, ... below e, read through `rows` from `msgs`.  A sum over two
// sources (a rank's matrix and its import buffer, derive.hip) is two calls, the second continuing the first's acc.
template <class Rows>
static __device__ __forceinline__ fr diag_walk(fr acc, uint32_t b, uint32_t e, uint32_t step, const lig_lin_term* __restrict__ terms, const fr* __restrict__ msgs,
                                               uint32_t l, uint32_t k, uint64_t l_recip, const fr* __restrict__ coef_mont, const Rows rows) {
    for (uint32_t t = b; t < e; t += step) acc = diag_accumulate(acc, terms[t], msgs, l, k, l_recip, coef_mont, rows);
    return acc;
}
// its two uses over the terms [b, e) of one constraint: one lane; or the lanes of a workgroup striding the segment, then the fixed tree
// (valid in thread 0; reached by all lanes of the workgroup)
template <class Rows>
static __device__ __forceinline__ fr diag_sum_lane(uint32_t b, uint32_t e, const lig_lin_term* __restrict__ terms, const fr* __restrict__ msgs, uint32_t l, uint32_t k,
                                                   uint64_t l_recip, const fr* __restrict__ coef_mont, const Rows rows) {
    return diag_walk(fr_zero(), b, e, 1, terms, msgs, l, k, l_recip, coef_mont, rows);
}
template <class Rows>
static __device__ __forceinline__ fr diag_sum_block(uint32_t b, uint32_t e, const lig_lin_term* __restrict__ terms, const fr* __restrict__ msgs, uint32_t l, uint32_t k,
                                                    uint64_t l_recip, const fr* __restrict__ coef_mont, const Rows rows, fr* sh) {
    return lin_block_sum(diag_walk(fr_zero(), b + threadIdx.x, e, LIN_WG, terms, msgs, l, k, l_recip, coef_mont, rows), sh);
}
}  // namespace lig
