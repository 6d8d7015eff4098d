// diagnose.hip -- which constraints of a rows job does the committed witness violate?  (lig_rows_diagnose, include/lig_hip.h)
//
// The prover's self-check answers with one bit per test (valid_linear, valid_quad), computed from a random combination.  This pass
// evaluates the statement itself on the committed witness matrix, exactly and without randomness, and returns the violated constraints:
//   k_diag_lin         one lane per linear constraint with at most HEAVY_MIN terms: walks a constraint-major term list, gathers w[slot]
//                      (32 bytes, random), adds / subtracts it or multiplies it by a table coefficient first (table in Montgomery
//                      form: one product per such term), subtracts b_c
//   k_diag_lin_heavy   one workgroup per constraint with more terms: lanes stride the segment, fixed LDS tree (lin_block_sum)
//   k_diag_quad        one lane per (quadratic term, column < l): x * y - z, b * b - b for a bit row, x - z for an equality pair
// and, for one rank of a sharded rows job (lig_shard_rows_diagnose: the rank holds only the rows it was dealt, a constraint may span ranks):
//   k_diag_lin_part, k_diag_lin_part_heavy   the same two walks over a slice of the constraints, through the rank's global -> local row
//                      table: a * w of the terms whose row the rank holds, the others skipped; a canonical PARTIAL per constraint, no b_c, no flag
//   k_diag_reduce      the owner of a sub-block of the slice adds the W partials it received, subtracts b_c, writes residual and flag
// (exact arithmetic mod p: no result depends on an order).  lig_shard_rows_diagnose_attached takes the partials from the rank's share
// ATTACHED to the shard instead (k_diag_att_bounds, k_diag_att_part*: their header below) and lets the one holder of a right-hand side
// subtract it there; the owner then only adds (k_diag_reduce<false>).
// lig_rows_explain* / lig_rows_read_slots and their sharded counterparts (k_explain_*, k_read_slots) have a header of their own below, and so
// have lig_rows_explain_slots* / lig_rows_untouched_slots* (k_slot_*, k_untouched_*), which read the slot-major program as it stands, and
// their sharded counterparts (k_slot_header, k_slot_collect_shard*: the owner of a slot's row collects, every rank receives).
// Where the constraint-major list comes from is the only difference between the two one-GPU entries:
//   lig_rows_diagnose            the caller's lig_linear_system, uploaded, with a scratch copy of its table in Montgomery form
//   lig_rows_diagnose_attached   the statement ATTACHED to the trace.  Its program keeps the terms slot-major (linear.hip: begin[], ent[] =
//                      (constraint, coefficient index)); per-constraint sums straight over that would need 256-bit atomics, so it is
//                      regrouped first -- the prepare of linear.hip run the other way:
//     k_diag_att_count    one lane per entry: a 32-bit atomic on the counter of its constraint
//     (rocPRIM exclusive scan of the counters -> cbegin; k_diag_att_classify: the constraints with more than HEAVY_MIN terms, sorted on the host)
//     k_diag_att_scatter  one lane per entry: its slot by binary search over begin[] (a slot with a very long segment does not serialise
//                      on one lane), lig_lin_term{slot, coef} to cbegin[c] + atomicAdd(cursor + c, 1)
//                      The atomics only decide WHERE a term lands inside its constraint's segment; the sum over a segment is exact, so no
//                      output byte depends on them.  One constraint with very many terms sends that many atomics to one address in the
//                      scatter: correct, slow, and off the proving path -- left as it is.
//                      rhs_coef and the Montgomery table in force for the attachment are read where they are: no copy, no conversion.
// Every lane writes its canonical residual and a 32-bit flag; the flags go through an exclusive scan (rocPRIM) and the first `cap`
// violated items are scattered into a record array in ascending order -- no atomic decides an order or a count, the output is the same
// bytes on every run.  The quadratic items (terms x l) are processed in slices of a fixed scratch budget; the running count and the
// output offset are carried on the host.  Like the form pass of linear.hip these passes are bound by the 32-byte gathers, not by VALU:
// canonical 8 x u32 arithmetic (fr.hpp).
// Everything is allocated inside the call and freed before it returns (off the proving path); all work is ENQUEUED on the context's
// main stream only -- the side stream, the uploader and the copy stream may be carrying the prefetch of the next trace.  Freeing the
// scratch (hipFree) waits for the whole device, though: with a prefetch in flight the call returns after that transfer (lig_hip.h says so).
// Host side: every entry works through one DiagFrame (scratch, typed allocation and copies, the two launch shapes, the scan, the wait);
// an entry of a sharded rows job through a DiagShardFrame, which adds the collectives, the LIG_TRACE phases and the one end of call.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "explain_plan.hpp"
#include "lin_common.hpp"
#include "lin_eval.hpp"
#include "prover_common.hpp"

namespace lig {
static constexpr uint32_t DIAG_MAX_BLOCKS = COEFS_MAX_BLOCKS;      // grid-stride passes: at most this many workgroups of LIN_WG lanes
static constexpr uint64_t DIAG_QUAD_ITEMS = 1ull << 20;            // scratch budget of the quadratic pass: (term, column) items per slice (40 bytes each)
static constexpr uint64_t DIAG_UNTOUCHED_ITEMS = 1ull << 22;       // scratch budget of the untouched pass: slots per slice (16 bytes each)

// (the walk over the terms of a constraint -- diag_div, diag_apply, diag_accumulate, diag_coef_value, diag_sum_lane, diag_sum_block -- is in
// lin_eval.hpp: derive.hip evaluates the same sums)
// acc - b_c -> residual and flag of constraint c, stored at index `at`; rhs_index[c] = 1 + the position of c in the right-hand-side list, 0: b_c = 0
static __device__ __forceinline__ void diag_finish(uint32_t c, uint32_t at, fr acc, const uint32_t* __restrict__ rhs_index, const uint32_t* __restrict__ rhs_coef,
                                                   const fr* __restrict__ coef_mont, fr* __restrict__ res, uint32_t* __restrict__ flag) {
    const uint32_t ri = rhs_index[c];
    if (ri) acc = fr_sub(acc, diag_coef_value(rhs_coef[ri - 1], coef_mont));
    fr_store(res + at, acc);
    flag[at] = fr_is_zero(acc) ? 0u : 1u;
}

// ---- the statement attached to the trace -> constraint-major (file header).  ent[e].x < n_constraints for every entry, the segments of
// begin[] tile [0, n_terms): the prepare built both from a system lig_linear_check accepted.
// slot of entry e: the s with begin[s] <= e < begin[s + 1] (slots may be empty); e < n_terms = begin[n_slots]
static __device__ __forceinline__ uint32_t diag_slot_of(const uint32_t* __restrict__ begin, uint32_t n_slots, uint32_t e) {
    uint32_t lo = 0, hi = n_slots;                // first index in (0, n_slots] whose entry is > e, minus one (lin_constraint_of, linear.hip)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (begin[mid + 1] > e) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// One rank's share of a sharded trace numbers its constraints compactly (linear.hip: ent[].x, rhs_c[] < n_need, need[i] = the constraint of
// the whole trace).  `need` != NULL regroups such a share by the numbers of the whole trace (one rank that holds every row: the one-GPU pass);
// NULL takes the numbers as they are -- a trace's own program, or the compact segments of lig_shard_rows_diagnose_attached.
static __device__ __forceinline__ uint32_t diag_number(const uint32_t* __restrict__ need, uint32_t c) { return need ? need[c] : c; }
__global__ void __launch_bounds__(LIN_WG) k_diag_att_count(const uint2* __restrict__ ent, uint32_t n_terms, const uint32_t* __restrict__ need,
                                                           uint32_t* __restrict__ count) {
    for (uint64_t e = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; e < n_terms; e += (uint64_t)gridDim.x * LIN_WG) atomicAdd(count + diag_number(need, ent[e].x), 1u);
}
// constraints with more than HEAVY_MIN terms, appended in any order: the host sorts the list
__global__ void __launch_bounds__(LIN_WG) k_diag_att_classify(const uint32_t* __restrict__ count, uint32_t n_constraints, uint32_t* __restrict__ heavy,
                                                              uint32_t heavy_cap, uint32_t* __restrict__ n_heavy) {
    for (uint64_t c = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; c < n_constraints; c += (uint64_t)gridDim.x * LIN_WG) {
        if (count[c] <= HEAVY_MIN) continue;
        const uint32_t i = atomicAdd(n_heavy, 1u);
        if (i < heavy_cap) heavy[i] = (uint32_t)c;
    }
}
// cursor[c] counts up to the number of terms of c (the counts cbegin was scanned from): every position lies inside the segment of c
__global__ void __launch_bounds__(LIN_WG) k_diag_att_scatter(const uint2* __restrict__ ent, uint32_t n_terms, const uint32_t* __restrict__ begin, uint32_t n_slots,
                                                             const uint32_t* __restrict__ need, const uint32_t* __restrict__ cbegin,
                                                             uint32_t* __restrict__ cursor, lig_lin_term* __restrict__ terms) {
    for (uint64_t e = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; e < n_terms; e += (uint64_t)gridDim.x * LIN_WG) {
        const uint2 en = ent[e];
        const uint32_t cn = diag_number(need, en.x);
        lig_lin_term tm;
        tm.slot = diag_slot_of(begin, n_slots, (uint32_t)e); tm.coef = en.y;
        terms[cbegin[cn] + atomicAdd(cursor + cn, 1u)] = tm;
    }
}

// rhs_constraint is strictly ascending: every entry of rhs_index is written at most once
__global__ void __launch_bounds__(LIN_WG) k_diag_rhs_index(const uint32_t* __restrict__ rhs_c, uint32_t n_rhs, const uint32_t* __restrict__ need,
                                                           uint32_t* __restrict__ rhs_index) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n_rhs; i += (uint64_t)gridDim.x * LIN_WG) rhs_index[diag_number(need, rhs_c[i])] = (uint32_t)i + 1;
}
__global__ void __launch_bounds__(LIN_WG) k_diag_lin(const uint32_t* __restrict__ term_begin, const lig_lin_term* __restrict__ terms, uint32_t n_constraints,
                                                     const fr* __restrict__ msgs, uint32_t l, uint32_t k, uint64_t l_recip, const fr* __restrict__ coef_mont,
                                                     const uint32_t* __restrict__ rhs_index, const uint32_t* __restrict__ rhs_coef, fr* __restrict__ res,
                                                     uint32_t* __restrict__ flag) {
    for (uint64_t c = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; c < n_constraints; c += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t b = term_begin[c], e = term_begin[c + 1];
        if (e - b > HEAVY_MIN) continue;                                  // k_diag_lin_heavy
        diag_finish((uint32_t)c, (uint32_t)c, diag_sum_lane(b, e, terms, msgs, l, k, l_recip, coef_mont, DiagAllRows{}), rhs_index, rhs_coef, coef_mont, res, flag);
    }
}
// workgroup -> heavy constraint heavy[blockIdx.x + i * gridDim.x]
__global__ void __launch_bounds__(LIN_WG) k_diag_lin_heavy(const uint32_t* __restrict__ heavy, uint32_t n_heavy, const uint32_t* __restrict__ term_begin,
                                                           const lig_lin_term* __restrict__ terms, const fr* __restrict__ msgs, uint32_t l, uint32_t k, uint64_t l_recip,
                                                           const fr* __restrict__ coef_mont, const uint32_t* __restrict__ rhs_index,
                                                           const uint32_t* __restrict__ rhs_coef, fr* __restrict__ res, uint32_t* __restrict__ flag) {
    __shared__ fr sh[LIN_WG];
    for (uint32_t h = blockIdx.x; h < n_heavy; h += gridDim.x) {          // (uniform over the workgroup: the barriers of lin_block_sum are reached by all lanes)
        const uint32_t c = heavy[h], b = term_begin[c], e = term_begin[c + 1];
        const fr acc = diag_sum_block(b, e, terms, msgs, l, k, l_recip, coef_mont, DiagAllRows{}, sh);
        if (threadIdx.x == 0) diag_finish(c, c, acc, rhs_index, rhs_coef, coef_mont, res, flag);
        __syncthreads();                                                  // sh is reused by the next constraint
    }
}
// One rank of a sharded rows job, constraints [c0, c0 + n) of the system of the WHOLE trace: part[c - c0] = the sum of a * w over the terms whose
// row this rank holds (local_of: global row -> local row of `msgs`, LIN_NOT_LOCAL for the rows of other ranks) -- zero for a constraint
// none of whose terms is here, and for every constraint on a rank without rows.  No b_c, no flag: k_diag_reduce on the owner.
__global__ void __launch_bounds__(LIN_WG) k_diag_lin_part(const uint32_t* __restrict__ term_begin, const lig_lin_term* __restrict__ terms, uint32_t c0, uint32_t n,
                                                          const fr* __restrict__ msgs, uint32_t l, uint32_t k, uint64_t l_recip, const fr* __restrict__ coef_mont,
                                                          const uint32_t* __restrict__ local_of, fr* __restrict__ part) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t b = term_begin[c0 + i], e = term_begin[c0 + i + 1];
        if (e - b > HEAVY_MIN) continue;                                  // k_diag_lin_part_heavy
        fr_store(part + i, diag_sum_lane(b, e, terms, msgs, l, k, l_recip, coef_mont, DiagLocalRows{local_of}));
    }
}
// workgroup -> heavy constraint heavy[blockIdx.x + i * gridDim.x]; heavy[0 .. n_heavy) are the heavy constraints of the slice, all >= c0
__global__ void __launch_bounds__(LIN_WG) k_diag_lin_part_heavy(const uint32_t* __restrict__ heavy, uint32_t n_heavy, const uint32_t* __restrict__ term_begin,
                                                                const lig_lin_term* __restrict__ terms, uint32_t c0, const fr* __restrict__ msgs, uint32_t l, uint32_t k,
                                                                uint64_t l_recip, const fr* __restrict__ coef_mont, const uint32_t* __restrict__ local_of,
                                                                fr* __restrict__ part) {
    __shared__ fr sh[LIN_WG];
    for (uint32_t h = blockIdx.x; h < n_heavy; h += gridDim.x) {          // (uniform over the workgroup, as in k_diag_lin_heavy)
        const uint32_t c = heavy[h], b = term_begin[c], e = term_begin[c + 1];
        const fr acc = diag_sum_block(b, e, terms, msgs, l, k, l_recip, coef_mont, DiagLocalRows{local_of}, sh);
        if (threadIdx.x == 0) fr_store(part + (c - c0), acc);
        __syncthreads();
    }
}
// ---- one rank of a sharded rows job, the share ATTACHED to it (lig_shard_rows_diagnose_attached): the regrouped list has one segment per
// COMPACT constraint i < n_need, its terms carry LOCAL slots (every one lies in the rank's own rows x k matrix), need[] is ascending.
//   k_diag_att_bounds        bound[j] = the first i with need[i] >= min(j * per, n_constraints), j = 0 .. n_slices: slice j of the constraints of
//                            the whole trace is the contiguous compact range [bound[j], bound[j + 1])
//   k_diag_att_heavy_global  the numbers of the whole trace of the (few) compact constraints with more than HEAVY_MIN local terms: the host
//                            cuts the sorted list at the slice boundaries
//   k_diag_att_part, k_diag_att_part_heavy   part[need[i] - c0] = the sum of a * w over the local terms of compact constraint i, MINUS b_c when
//                            this rank holds the right-hand side of it (rhs_index[i], over the compact numbers): a right-hand side has
//                            exactly one holder, so the W partials add up to the residual.  The send buffer was zeroed first: a
//                            constraint this rank does not need contributes zero.
static __device__ __forceinline__ uint32_t diag_lower_bound(const uint32_t* __restrict__ a, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__global__ void __launch_bounds__(LIN_WG) k_diag_att_bounds(const uint32_t* __restrict__ need, uint32_t n_need, uint64_t per, uint32_t n_slices,
                                                            uint64_t n_constraints, uint32_t* __restrict__ bound) {
    for (uint64_t j = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; j <= n_slices; j += (uint64_t)gridDim.x * LIN_WG) {
        const uint64_t c = j * per;
        bound[j] = diag_lower_bound(need, n_need, c < n_constraints ? c : n_constraints);
    }
}
__global__ void __launch_bounds__(LIN_WG) k_diag_att_heavy_global(const uint32_t* __restrict__ heavy, uint32_t n_heavy, const uint32_t* __restrict__ need,
                                                                  uint32_t* __restrict__ out) {
    for (uint64_t h = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; h < n_heavy; h += (uint64_t)gridDim.x * LIN_WG) out[h] = need[heavy[h]];
}
// acc - b_c (when this rank holds it) -> the partial of compact constraint i; the range came from k_diag_att_bounds, so need[i] - c0 < n
// (checked all the same: nothing is ever stored outside the n entries of the slice)
static __device__ __forceinline__ void diag_part_store(uint32_t i, fr acc, const uint32_t* __restrict__ need, uint32_t c0, uint32_t n,
                                                       const uint32_t* __restrict__ rhs_index, const uint32_t* __restrict__ rhs_coef,
                                                       const fr* __restrict__ coef_mont, fr* __restrict__ part) {
    const uint32_t at = need[i] - c0;
    if (at >= n) return;
    const uint32_t ri = rhs_index[i];
    if (ri) acc = fr_sub(acc, diag_coef_value(rhs_coef[ri - 1], coef_mont));
    fr_store(part + at, acc);
}
// range[0], range[1] = the compact range of the slice [c0, c0 + n)
__global__ void __launch_bounds__(LIN_WG) k_diag_att_part(const uint32_t* __restrict__ range, const uint32_t* __restrict__ term_begin,
                                                          const lig_lin_term* __restrict__ terms, const uint32_t* __restrict__ need, uint32_t c0, uint32_t n,
                                                          const fr* __restrict__ msgs, uint32_t l, uint32_t k, uint64_t l_recip, const fr* __restrict__ coef_mont,
                                                          const uint32_t* __restrict__ rhs_index, const uint32_t* __restrict__ rhs_coef, fr* __restrict__ part) {
    const uint32_t i0 = range[0], i1 = range[1];
    for (uint64_t i = (uint64_t)i0 + (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < i1; i += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t b = term_begin[i], e = term_begin[i + 1];
        if (e - b > HEAVY_MIN) continue;                                  // k_diag_att_part_heavy
        diag_part_store((uint32_t)i, diag_sum_lane(b, e, terms, msgs, l, k, l_recip, coef_mont, DiagAllRows{}), need, c0, n, rhs_index, rhs_coef, coef_mont, part);
    }
}
// workgroup -> heavy compact constraint heavy[blockIdx.x + i * gridDim.x]; heavy[0 .. n_heavy) are those of the slice
__global__ void __launch_bounds__(LIN_WG) k_diag_att_part_heavy(const uint32_t* __restrict__ heavy, uint32_t n_heavy, const uint32_t* __restrict__ term_begin,
                                                                const lig_lin_term* __restrict__ terms, const uint32_t* __restrict__ need, uint32_t c0, uint32_t n,
                                                                const fr* __restrict__ msgs, uint32_t l, uint32_t k, uint64_t l_recip, const fr* __restrict__ coef_mont,
                                                                const uint32_t* __restrict__ rhs_index, const uint32_t* __restrict__ rhs_coef, fr* __restrict__ part) {
    __shared__ fr sh[LIN_WG];
    for (uint32_t h = blockIdx.x; h < n_heavy; h += gridDim.x) {          // (uniform over the workgroup, as in k_diag_lin_heavy)
        const uint32_t i = heavy[h], b = term_begin[i], e = term_begin[i + 1];
        const fr acc = diag_sum_block(b, e, terms, msgs, l, k, l_recip, coef_mont, DiagAllRows{}, sh);
        if (threadIdx.x == 0) diag_part_store(i, acc, need, c0, n, rhs_index, rhs_coef, coef_mont, part);
        __syncthreads();
    }
}
// The owner of constraints [first, first + n_valid): recv = W blocks of B partials, block g from rank g, entry i of every block = constraint
// first + i.  res[i] = their sum - b_c, flag[i]; entries [n_valid, B) (beyond the end of the system) get flag 0.  RHS = false: the holder of
// b_c has subtracted it in its partial (k_diag_att_part*), the sum is the residual and rhs_index / rhs_coef / coef_mont are not read.
template <bool RHS>
__global__ void __launch_bounds__(LIN_WG) k_diag_reduce(const fr* __restrict__ recv, uint32_t W, uint32_t B, uint32_t n_valid, uint32_t first,
                                                        const uint32_t* __restrict__ rhs_index, const uint32_t* __restrict__ rhs_coef, const fr* __restrict__ coef_mont,
                                                        fr* __restrict__ res, uint32_t* __restrict__ flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < B; i += (uint64_t)gridDim.x * LIN_WG) {
        if (i >= n_valid) { flag[i] = 0u; continue; }
        fr acc = fr_load(recv + i);
        for (uint32_t g = 1; g < W; g++) acc = fr_add(acc, fr_load(recv + (size_t)g * B + i));
        if (RHS) { diag_finish(first + (uint32_t)i, (uint32_t)i, acc, rhs_index, rhs_coef, coef_mont, res, flag); continue; }
        fr_store(res + i, acc);
        flag[i] = fr_is_zero(acc) ? 0u : 1u;
    }
}
// item i of the slice = (term first_term + i / l, column i % l); tri = (x, y, z) rows per term, y = 0xFFFFFFFF: the equality term x - z
__global__ void __launch_bounds__(LIN_WG) k_diag_quad(const uint32_t* __restrict__ tri, uint32_t first_term, uint32_t n_items, const fr* __restrict__ msgs, uint32_t l,
                                                      uint32_t k, uint64_t l_recip, fr* __restrict__ res, uint32_t* __restrict__ flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n_items; i += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t t = diag_div((uint32_t)i, l_recip), col = (uint32_t)i - t * l;
        const uint32_t* q = tri + 3 * (size_t)(first_term + t);
        const uint32_t rx = q[0], ry = q[1], rz = q[2];
        const fr x = fr_load(msgs + (size_t)rx * k + col), z = fr_load(msgs + (size_t)rz * k + col);
        const fr r = ry == 0xFFFFFFFFu ? fr_sub(x, z) : fr_sub(fr_mul(x, fr_load(msgs + (size_t)ry * k + col)), z);
        fr_store(res + i, r);
        flag[i] = fr_is_zero(r) ? 0u : 1u;
    }
}
// the violated items with a position below `cap` -> records, in ascending order (pos = exclusive scan of flag); item c = constraint first + c
__global__ void __launch_bounds__(LIN_WG) k_diag_scatter_lin(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, const fr* __restrict__ res,
                                                             uint32_t n, uint32_t first, uint32_t cap, lig_diag_linear* __restrict__ out) {
    for (uint64_t c = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; c < n; c += (uint64_t)gridDim.x * LIN_WG) {
        if (!flag[c] || pos[c] >= cap) continue;
        lig_diag_linear rec;
        rec.constraint = first + (uint32_t)c; rec.reserved = 0;
        const fr r = fr_load(res + c);
        for (int w = 0; w < 8; w++) for (int b = 0; b < 4; b++) rec.residual[4 * w + b] = (uint8_t)(r.v[w] >> (8 * b));
        out[pos[c]] = rec;
    }
}
// grow (NULL: the rows of `tri` are the job's): local -> global row of a rank's share; ord / ord_out (NULL: none): the global ordinal of every
// local term, written next to its records
__global__ void __launch_bounds__(LIN_WG) k_diag_scatter_quad(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, const fr* __restrict__ res,
                                                              const uint32_t* __restrict__ tri, uint32_t first_term, uint32_t n_items, uint32_t l, uint64_t l_recip,
                                                              uint32_t cap, lig_diag_quad* __restrict__ out, const uint32_t* __restrict__ grow,
                                                              const uint32_t* __restrict__ ord, uint32_t* __restrict__ ord_out) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n_items; i += (uint64_t)gridDim.x * LIN_WG) {
        if (!flag[i] || pos[i] >= cap) continue;
        const uint32_t t = diag_div((uint32_t)i, l_recip);
        const uint32_t* q = tri + 3 * (size_t)(first_term + t);
        lig_diag_quad rec;
        rec.row_x = q[0]; rec.row_y = q[1]; rec.row_z = q[2]; rec.column = (uint32_t)i - t * l;
        if (grow) { rec.row_x = grow[rec.row_x]; if (rec.row_y != 0xFFFFFFFFu) rec.row_y = grow[rec.row_y]; rec.row_z = grow[rec.row_z]; }
        if (ord_out) ord_out[pos[i]] = ord[first_term + t];
        const fr r = fr_load(res + i);
        for (int w = 0; w < 8; w++) for (int b = 0; b < 4; b++) rec.residual[4 * w + b] = (uint8_t)(r.v[w] >> (8 * b));
        out[pos[i]] = rec;
    }
}

// ---- lig_rows_explain / lig_rows_explain_attached: the asked constraints as the library holds them (terms, coefficient values, committed
// witness values, b_c, residual), and lig_rows_read_slots.  A term before it is filled in is a 12-byte lig::ExplainItem {index in the
// asked list, slot, coefficient index} (explain_plan.hpp).  Where the items come from is the only difference between the two entries:
//   k_explain_mark     (attached) one lane per entry of the program: mark[e] = 1 + the position of its constraint in the asked list (binary
//                      search over the ascending device copy), 0 when it is not asked
//   (rocPRIM exclusive scan of mark != 0 -> pos, the total m)
//   k_explain_collect  (attached) a marked entry writes its item at pos[e]; its slot by binary search over begin[] (diag_slot_of).  No atomic.
//   k_explain_gather   (term list) one lane per output term: the asked segments of the uploaded constraint-major list, addressed through the
//                      prefix sums of their lengths (host)
// The host puts the m items into the output order (explain_order: a total order on the 12 bytes, so the bytes depend neither on the order
// of the entries inside a slot's segment -- which prepare made the program -- nor on the sort) and uploads them again; then
//   k_explain_fill     one lane per reported record: coefficient value (diag_coef_value), the 32-byte gather of w[slot], 16-byte stores
//   k_explain_finish   one workgroup per asked constraint over its segment of the ordered items: the lanes stride it, the fixed tree, b_c as in
//                      diag_finish; writes the whole 88-byte record
//   k_read_slots       one lane per slot: gather, store
// On a rank of a sharded rows job (lig_shard_rows_explain / lig_shard_rows_read_slots) the items are formed and ordered on the host from the
// caller's term list (explain_items_of), the values cross the ranks in pieces (k_explain_part, one all-gather, k_explain_sum), and the same
// fill and finish run over the value list instead of the matrix (their witness source is a template parameter).
// lig_shard_rows_explain_attached selects the items from the rank's own share with k_explain_mark and gathers whole records (its kernels
// have a header of their own below).
// position of c in the ascending list asked[0 .. n), n when it is not there
static __device__ __forceinline__ uint32_t explain_find(const uint32_t* __restrict__ asked, uint32_t n, uint32_t c) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (asked[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo < n && asked[lo] == c ? lo : n;
}
struct ExplainMarked { __host__ __device__ uint32_t operator()(uint32_t mark) const { return mark ? 1u : 0u; } };
// need: NULL, or the need list of a rank's share (diag_number): the asked list always holds numbers of the whole trace
__global__ void __launch_bounds__(LIN_WG) k_explain_mark(const uint2* __restrict__ ent, uint32_t n_terms, const uint32_t* __restrict__ need,
                                                         const uint32_t* __restrict__ asked, uint32_t n_asked, uint32_t* __restrict__ mark) {
    for (uint64_t e = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; e < n_terms; e += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t a = explain_find(asked, n_asked, diag_number(need, ent[e].x));
        mark[e] = a < n_asked ? a + 1 : 0u;
    }
}
// pos = the exclusive scan of mark != 0: the marked entries get the positions 0 .. m - 1 in entry order, items has m entries
__global__ void __launch_bounds__(LIN_WG) k_explain_collect(const uint2* __restrict__ ent, uint32_t n_terms, const uint32_t* __restrict__ begin, uint32_t n_slots,
                                                            const uint32_t* __restrict__ mark, const uint32_t* __restrict__ pos, ExplainItem* __restrict__ items) {
    for (uint64_t e = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; e < n_terms; e += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t mk = mark[e];
        if (!mk) continue;
        ExplainItem it;
        it.ask = mk - 1; it.slot = diag_slot_of(begin, n_slots, (uint32_t)e); it.coef = ent[e].y;
        items[pos[e]] = it;
    }
}
// pre[0 .. n_asked]: prefix sums of the asked constraints' term counts, pre[n_asked] = m; item i belongs to the a with pre[a] <= i < pre[a + 1]
__global__ void __launch_bounds__(LIN_WG) k_explain_gather(const uint32_t* __restrict__ term_begin, const lig_lin_term* __restrict__ terms,
                                                           const uint32_t* __restrict__ asked, uint32_t n_asked, const uint32_t* __restrict__ pre, uint32_t m,
                                                           ExplainItem* __restrict__ items) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < m; i += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t a = diag_slot_of(pre, n_asked, (uint32_t)i);
        const lig_lin_term tm = terms[term_begin[asked[a]] + ((uint32_t)i - pre[a])];
        ExplainItem it;
        it.ask = a; it.slot = tm.slot; it.coef = tm.coef;
        items[i] = it;
    }
}
static __device__ __forceinline__ fr diag_witness(uint32_t slot, const fr* __restrict__ msgs, uint32_t l, uint32_t k, uint64_t l_recip) {
    const uint32_t row = diag_div(slot, l_recip);
    return fr_load(msgs + (size_t)row * k + (slot - row * l));
}
// Where k_explain_fill / k_explain_finish take the committed w of the term at position t of the ordered list from, and how they find b_c:
//   ExplainFromMatrix   the rows x k matrix (one GPU): w[slot]; rhs_index is indexed by the constraint number (k_diag_rhs_index)
//   ExplainFromValues   vals[t], the values the ranks of a shard exchanged (k_explain_part, k_explain_sum: no rank holds every row);
//                       rhs_index is indexed by the position in the asked list (made on the host: only the asked constraints are uploaded)
struct ExplainFromMatrix {
    static constexpr bool rhs_by_asked = false;
    const fr* __restrict__ msgs; uint32_t l, k; uint64_t l_recip;
    __device__ __forceinline__ fr operator()(uint32_t, uint32_t slot) const { return diag_witness(slot, msgs, l, k, l_recip); }
};
struct ExplainFromValues {
    static constexpr bool rhs_by_asked = true;
    const fr* __restrict__ vals;
    __device__ __forceinline__ fr operator()(uint32_t t, uint32_t) const { return fr_load(vals + t); }
};
// record i = the i-th item of the output order: terms[i] with ask[i]; out is 16-byte aligned and a record has 80 bytes
template <class Wit>
__global__ void __launch_bounds__(LIN_WG) k_explain_fill(const lig_lin_term* __restrict__ terms, const uint32_t* __restrict__ ask, uint32_t n,
                                                         const uint32_t* __restrict__ asked, const Wit wit, const fr* __restrict__ coef_mont,
                                                         lig_explain_term* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LIN_WG) {
        const lig_lin_term tm = terms[i];
        uint4* o = reinterpret_cast<uint4*>(out + i);
        o[0] = make_uint4(asked[ask[i]], tm.slot, tm.coef, 0u);
        fr_store(reinterpret_cast<fr*>(o + 1), diag_coef_value(tm.coef, coef_mont));
        fr_store(reinterpret_cast<fr*>(o + 3), wit((uint32_t)i, tm.slot));
    }
}
// workgroup -> asked constraint blockIdx.x + i * gridDim.x; first[0 .. n_asked]: its items are terms[first[a] .. first[a + 1]): the lanes stride
// the segment, then the fixed tree (as diag_sum_block).  A record has 88 bytes: 8-byte stores.
template <class Wit>
__global__ void __launch_bounds__(LIN_WG) k_explain_finish(const uint32_t* __restrict__ first, const lig_lin_term* __restrict__ terms, const uint32_t* __restrict__ asked,
                                                           uint32_t n_asked, const Wit wit, const fr* __restrict__ coef_mont, const uint32_t* __restrict__ rhs_index,
                                                           const uint32_t* __restrict__ rhs_coef, lig_explain_constraint* __restrict__ out) {
    __shared__ fr sh[LIN_WG];
    for (uint32_t a = blockIdx.x; a < n_asked; a += gridDim.x) {          // (uniform over the workgroup, as in k_diag_lin_heavy)
        const uint32_t b = first[a], e = first[a + 1];
        fr acc = fr_zero();
        for (uint32_t t = b + threadIdx.x; t < e; t += LIN_WG) {
            const lig_lin_term tm = terms[t];
            acc = diag_apply(acc, tm.coef, wit(t, tm.slot), coef_mont);
        }
        acc = lin_block_sum(acc, sh);
        if (threadIdx.x == 0) {
            const uint32_t cn = asked[a], ri = rhs_index[Wit::rhs_by_asked ? a : cn];
            const fr rhs = ri ? diag_coef_value(rhs_coef[ri - 1], coef_mont) : fr_zero();
            const fr res = fr_sub(acc, rhs);
            uint2* o = reinterpret_cast<uint2*>(out + a);
            o[0] = make_uint2(cn, 0u);
            o[1] = make_uint2(e - b, 0u);
            o[2] = make_uint2(b, 0u);
            for (int w = 0; w < 4; w++) { o[3 + w] = make_uint2(rhs.v[2 * w], rhs.v[2 * w + 1]); o[7 + w] = make_uint2(res.v[2 * w], res.v[2 * w + 1]); }
        }
        __syncthreads();                                                  // sh is reused by the next constraint
    }
}
// ---- one rank of a sharded rows job (lig_shard_rows_explain, lig_shard_rows_read_slots): the value of a slot exists on the rank that was
// dealt its row, and nowhere else.
//   k_explain_part   one lane per entry of a piece: send[i] = the canonical w of slot[i * stride] when this rank holds its row (local_of, as
//                    k_diag_lin_part), zero when it does not.  stride = 2: the slots of a lig_lin_term list; 1: a plain slot list.
//                    Every slot is < rows_global * l (the host checked it): the row indexes local_of inside its rows_global entries.
//   k_explain_sum    one lane per entry: vals[i] = the sum of the W received values (recv = W blocks of P entries, block g from rank g).
//                    A row has one owner, so exactly one summand is non-zero: the sum is the value, no owner table, no dependence on order.
__global__ void __launch_bounds__(LIN_WG) k_explain_part(const uint32_t* __restrict__ slot, uint32_t stride, uint32_t n, const fr* __restrict__ msgs, uint32_t l,
                                                         uint32_t k, uint64_t l_recip, const uint32_t* __restrict__ local_of, fr* __restrict__ send) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t sl = slot[i * stride], grow = diag_div(sl, l_recip), row = local_of[grow];
        fr_store(send + i, row == LIN_NOT_LOCAL ? fr_zero() : fr_load(msgs + (size_t)row * k + (sl - grow * l)));
    }
}
__global__ void __launch_bounds__(LIN_WG) k_explain_sum(const fr* __restrict__ recv, uint32_t W, uint32_t P, uint32_t n, fr* __restrict__ vals) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LIN_WG) {
        fr acc = fr_load(recv + i);
        for (uint32_t g = 1; g < W; g++) acc = fr_add(acc, fr_load(recv + (size_t)g * P + i));
        fr_store(vals + i, acc);
    }
}
// ---- lig_shard_rows_explain_attached: a rank keeps exactly the terms whose row it was dealt, so it selects the asked ones from its own
// share (k_explain_mark through need[], the scan) and reads their values from its own matrix; the records cross the ranks whole.
//   k_explain_rhs_held        one lane per right-hand side of the rank's slice: held[a] = {1, coefficient index} when its constraint is
//                             asked constraint a (rhs_c is strictly ascending: every pair is written at most once); rhs_c[i] < n_need
//   k_explain_collect_values  a marked entry writes its 48-byte ExplainRecord at pos[e] (k_explain_collect): the LOCAL slot of the entry is
//                             below n_slots = rows_local * l (the host checked the product), its row indexes grow[0 .. rows_local) and the
//                             rows_local x k matrix; the slot written is the one of the whole trace, grow[row] * l + column < 2^32 (host)
//   k_explain_keep            piece j of the record all-gathers (recv = W blocks of P records): every head is copied for the host's walk,
//                             the value of record r of rank g goes to vals[off[g] + j * P + r] while j * P + r < m[g] (m, off: the host's
//                             schedule, off[g] + m[g] <= the length of vals)
//   k_explain_permute         out[i] = in[perm[i]], perm[i] < the length of in (explain_merge)
__global__ void __launch_bounds__(LIN_WG) k_explain_rhs_held(const uint32_t* __restrict__ rhs_c, const uint32_t* __restrict__ rhs_coef, uint32_t n_rhs,
                                                             const uint32_t* __restrict__ need, const uint32_t* __restrict__ asked, uint32_t n_asked,
                                                             uint2* __restrict__ held) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n_rhs; i += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t a = explain_find(asked, n_asked, diag_number(need, rhs_c[i]));
        if (a < n_asked) held[a] = make_uint2(1u, rhs_coef[i]);
    }
}
__global__ void __launch_bounds__(LIN_WG) k_explain_collect_values(const uint2* __restrict__ ent, uint32_t n_terms, const uint32_t* __restrict__ begin, uint32_t n_slots,
                                                                   const uint32_t* __restrict__ mark, const uint32_t* __restrict__ pos,
                                                                   const uint32_t* __restrict__ grow, const fr* __restrict__ msgs, uint32_t l, uint32_t k,
                                                                   uint64_t l_recip, ExplainRecord* __restrict__ rec) {
    for (uint64_t e = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; e < n_terms; e += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t mk = mark[e];
        if (!mk) continue;
        const uint32_t sl = diag_slot_of(begin, n_slots, (uint32_t)e), row = diag_div(sl, l_recip), col = sl - row * l;
        uint4* o = reinterpret_cast<uint4*>(rec + pos[e]);
        o[0] = make_uint4(mk - 1, grow[row] * l + col, ent[e].y, 1u);
        fr_store(reinterpret_cast<fr*>(o + 1), fr_load(msgs + (size_t)row * k + col));
    }
}
__global__ void __launch_bounds__(LIN_WG) k_explain_keep(const ExplainRecord* __restrict__ recv, uint32_t W, uint32_t P, uint64_t j, const uint32_t* __restrict__ m,
                                                         const uint32_t* __restrict__ off, uint4* __restrict__ heads, fr* __restrict__ vals) {
    const uint64_t n = (uint64_t)W * P;
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t g = (uint32_t)(i / P), r = (uint32_t)(i - (uint64_t)g * P);
        const uint4* in = reinterpret_cast<const uint4*>(recv + i);
        heads[i] = in[0];
        const uint64_t at = j * P + r;
        if (at < m[g]) fr_store(vals + (off[g] + at), fr_load(reinterpret_cast<const fr*>(in + 1)));
    }
}
__global__ void __launch_bounds__(LIN_WG) k_explain_permute(const fr* __restrict__ in, const uint32_t* __restrict__ perm, uint32_t n, fr* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LIN_WG) fr_store(out + i, fr_load(in + perm[i]));
}
__global__ void __launch_bounds__(LIN_WG) k_read_slots(const uint32_t* __restrict__ slots, uint32_t n, const fr* __restrict__ msgs, uint32_t l, uint32_t k,
                                                       uint64_t l_recip, fr* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LIN_WG)
        fr_store(out + i, diag_witness(slots[i], msgs, l, k, l_recip));
}

// ---- lig_rows_explain_slots*: the constraints through the asked slots.  The program is slot-major, so the terms of asked slot a are the
// segment ent[begin[slots[a]] .. begin[slots[a] + 1]) as it stands: nothing is marked, nothing regrouped.  An item is an ExplainItem whose
// `slot` field carries the CONSTRAINT: {index in the asked list, constraint, coefficient index}, so that explain_order is the output order.
//   k_slot_len            one lane per asked slot: len[a] = the length of its segment
//   (rocPRIM exclusive scan -> pre[0 .. n_asked], the total m; downloaded: the host needs n_terms / first_term and the heavy list)
//   k_slot_collect        one lane per item i < m: its asked slot by binary search over pre[] (diag_slot_of), the entry copied to items[i];
//                         the items of a slot with more than HEAVY_MIN terms are left to
//   k_slot_collect_heavy  one workgroup per such slot, the lanes striding its segment (one slot may carry 2^24 terms)
//   k_slot_fill           one lane per reported record, over the items the host has ordered: the coefficient value in force
//                         (diag_coef_value), size and residual of its constraint out of the record k_explain_finish wrote for it (con[cidx[i]]:
//                         the distinct constraints went through explain_rows), 16-byte stores
// No atomic.  Where an item lands inside items[pre[a] .. pre[a + 1]) follows the order inside the slot's segment, which the atomics of the
// prepare decided: the host's sort on the whole 12 bytes removes it.  Every slots[a] < n_slots = rows * l and begin[] tiles [0, n_terms)
// (the host has checked the asked list, and m <= n_terms before the collect is launched): every read of ent[] lies inside it.
__global__ void __launch_bounds__(LIN_WG) k_slot_len(const uint32_t* __restrict__ slots, uint32_t n_asked, const uint32_t* __restrict__ begin, uint32_t* __restrict__ len) {
    for (uint64_t a = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; a < n_asked; a += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t s = slots[a];
        len[a] = begin[s + 1] - begin[s];
    }
}
__global__ void __launch_bounds__(LIN_WG) k_slot_collect(const uint32_t* __restrict__ slots, uint32_t n_asked, const uint32_t* __restrict__ pre, uint32_t m,
                                                         const uint32_t* __restrict__ begin, const uint2* __restrict__ ent, ExplainItem* __restrict__ items) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < m; i += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t a = diag_slot_of(pre, n_asked, (uint32_t)i), b = pre[a];
        if (pre[a + 1] - b > HEAVY_MIN) continue;                             // k_slot_collect_heavy
        const uint2 en = ent[begin[slots[a]] + ((uint32_t)i - b)];
        ExplainItem it;
        it.ask = a; it.slot = en.x; it.coef = en.y;
        items[i] = it;
    }
}
// workgroup -> heavy asked slot heavy[blockIdx.x + i * gridDim.x] (indices into the asked list, ascending)
__global__ void __launch_bounds__(LIN_WG) k_slot_collect_heavy(const uint32_t* __restrict__ heavy, uint32_t n_heavy, const uint32_t* __restrict__ slots,
                                                               const uint32_t* __restrict__ pre, const uint32_t* __restrict__ begin, const uint2* __restrict__ ent,
                                                               ExplainItem* __restrict__ items) {
    for (uint32_t h = blockIdx.x; h < n_heavy; h += gridDim.x) {
        const uint32_t a = heavy[h], b = pre[a], n = pre[a + 1] - b, src = begin[slots[a]];
        for (uint32_t j = threadIdx.x; j < n; j += LIN_WG) {
            const uint2 en = ent[src + j];
            ExplainItem it;
            it.ask = a; it.slot = en.x; it.coef = en.y;
            items[b + j] = it;
        }
    }
}
// record i = the i-th item of the output order; out is 16-byte aligned and a record has 80 bytes; a constraint record has 88, its residual
// begins at byte 56: 8-byte loads
__global__ void __launch_bounds__(LIN_WG) k_slot_fill(const ExplainItem* __restrict__ items, const uint32_t* __restrict__ cidx, uint32_t n,
                                                      const uint32_t* __restrict__ slots, const lig_explain_constraint* __restrict__ con,
                                                      const fr* __restrict__ coef_mont, lig_slot_term* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LIN_WG) {
        const ExplainItem it = items[i];
        const uint2* cr = reinterpret_cast<const uint2*>(con + cidx[i]);      // {constraint, 0}, n_terms, first_term, rhs x 4, residual x 4
        uint4* o = reinterpret_cast<uint4*>(out + i);
        o[0] = make_uint4(slots[it.ask], it.slot, it.coef, cr[1].x);
        fr_store(reinterpret_cast<fr*>(o + 1), diag_coef_value(it.coef, coef_mont));
        const uint2 r0 = cr[7], r1 = cr[8], r2 = cr[9], r3 = cr[10];
        o[3] = make_uint4(r0.x, r0.y, r1.x, r1.y);
        o[4] = make_uint4(r2.x, r2.y, r3.x, r3.y);
    }
}
// ---- lig_shard_rows_explain_slots*: one rank of a sharded rows job.  Every term through a slot lies in the share of the rank that was dealt
// its row, so that rank runs k_slot_len / the scan / k_read_slots over the asked slots it holds, in its LOCAL numbering (lslots, ascending;
// mine[i] = the index of lslots[i] in the asked list of the whole call), and
//   k_slot_header               one lane per held slot: {held = 1, n_terms, 0, 0, value} into the rank's header block (slot_header_at,
//                               explain_plan.hpp; 48 bytes at a 16-byte boundary: three 16-byte stores).  The block was zeroed first.
//   k_slot_collect_shard        k_slot_collect into 16-byte SlotItems {index in the asked list, constraint OF THE WHOLE TRACE = need[ent.x],
//                               coefficient index, valid = 1}, one 16-byte store each
//   k_slot_collect_shard_heavy  k_slot_collect_heavy likewise: a hot slot's terms all lie on its owner
// No atomic.  Every lslots[i] < n_slots = rows_local * l, every mine[i] < n_asked (slot_asked_here made both on the host), ent[].x < n_need
// (the prepare), m <= n_terms checked before the collect is launched.
__global__ void __launch_bounds__(LIN_WG) k_slot_header(const uint32_t* __restrict__ mine, const uint32_t* __restrict__ len, const fr* __restrict__ val, uint32_t n_here,
                                                        uint32_t* __restrict__ hdr) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n_here; i += (uint64_t)gridDim.x * LIN_WG) {
        uint4* o = reinterpret_cast<uint4*>(hdr + slot_header_at(mine[i]));
        o[0] = make_uint4(1u, len[i], 0u, 0u);
        fr_store(reinterpret_cast<fr*>(o + 1), fr_load(val + i));
    }
}
static __device__ __forceinline__ void slot_item_store(SlotItem* __restrict__ at, uint32_t ask, const uint2 en, const uint32_t* __restrict__ need) {
    *reinterpret_cast<uint4*>(at) = make_uint4(ask, need[en.x], en.y, 1u);
}
__global__ void __launch_bounds__(LIN_WG) k_slot_collect_shard(const uint32_t* __restrict__ lslots, const uint32_t* __restrict__ mine, uint32_t n_here,
                                                               const uint32_t* __restrict__ pre, uint32_t m, const uint32_t* __restrict__ begin,
                                                               const uint2* __restrict__ ent, const uint32_t* __restrict__ need, SlotItem* __restrict__ items) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < m; i += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t a = diag_slot_of(pre, n_here, (uint32_t)i), b = pre[a];
        if (pre[a + 1] - b > HEAVY_MIN) continue;                             // k_slot_collect_shard_heavy
        slot_item_store(items + i, mine[a], ent[begin[lslots[a]] + ((uint32_t)i - b)], need);
    }
}
// workgroup -> heavy held slot heavy[blockIdx.x + i * gridDim.x] (indices into lslots, ascending)
__global__ void __launch_bounds__(LIN_WG) k_slot_collect_shard_heavy(const uint32_t* __restrict__ heavy, uint32_t n_heavy, const uint32_t* __restrict__ lslots,
                                                                     const uint32_t* __restrict__ mine, const uint32_t* __restrict__ pre,
                                                                     const uint32_t* __restrict__ begin, const uint2* __restrict__ ent,
                                                                     const uint32_t* __restrict__ need, SlotItem* __restrict__ items) {
    for (uint32_t h = blockIdx.x; h < n_heavy; h += gridDim.x) {
        const uint32_t a = heavy[h], b = pre[a], n = pre[a + 1] - b, src = begin[lslots[a]], ask = mine[a];
        for (uint32_t j = threadIdx.x; j < n; j += LIN_WG) slot_item_store(items + b + j, ask, ent[src + j], need);
    }
}
// ---- lig_rows_untouched_slots*: the slots of the LINEAR / QX / QY / QZ rows with an empty segment.  lrows = those rows ascending, {row, kind};
// item i of a slice = column i % l of row lrows[first + i / l].  On a rank of a sharded rows job (lig_shard_rows_untouched_slots*) lrows is
// {LOCAL row, kind, row of the WHOLE trace, 0}: the local row addresses begin[] and the matrix, the global one makes the record's slot.
//   k_untouched_flag     flag[i] = 1 when the segment of the slot is empty, + 2^32 when its committed element is not zero besides (fr_load:
//                        two 16-byte loads) -- one 64-bit exclusive scan (rocPRIM) carries both counts, no atomic
//   k_untouched_compact  the selected slots with a position below `cap` -> {slot, kind, value} in ascending order; a record has 40 bytes:
//                        8-byte stores
static __device__ __forceinline__ uint32_t untouched_trace_row(const uint2 lr) { return lr.x; }
static __device__ __forceinline__ uint32_t untouched_trace_row(const uint4 lr) { return lr.z; }
template <class LR>
__global__ void __launch_bounds__(LIN_WG) k_untouched_flag(const LR* __restrict__ lrows, uint32_t first, uint32_t n_items, const uint32_t* __restrict__ begin,
                                                           const fr* __restrict__ msgs, uint32_t l, uint32_t k, uint64_t l_recip, uint64_t* __restrict__ flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n_items; i += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t t = diag_div((uint32_t)i, l_recip), col = (uint32_t)i - t * l, row = lrows[first + t].x, s = row * l + col;
        uint64_t f = 0;
        if (begin[s + 1] == begin[s]) f = fr_is_zero(fr_load(msgs + (size_t)row * k + col)) ? 1ull : 1ull | (1ull << 32);
        flag[i] = f;
    }
}
template <class LR>
__global__ void __launch_bounds__(LIN_WG) k_untouched_compact(const uint64_t* __restrict__ flag, const uint64_t* __restrict__ pos, const LR* __restrict__ lrows,
                                                              uint32_t first, uint32_t n_items, const fr* __restrict__ msgs, uint32_t l, uint32_t k, uint64_t l_recip,
                                                              uint32_t nonzero_only, uint32_t cap, lig_slot_value* __restrict__ out) {
    const uint32_t shift = nonzero_only ? 32u : 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n_items; i += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t at = (uint32_t)(pos[i] >> shift);
        if (!(uint32_t)(flag[i] >> shift) || at >= cap) continue;
        const uint32_t t = diag_div((uint32_t)i, l_recip), col = (uint32_t)i - t * l;
        const LR lr = lrows[first + t];
        const fr w = fr_load(msgs + (size_t)lr.x * k + col);
        uint2* o = reinterpret_cast<uint2*>(out + at);
        o[0] = make_uint2(untouched_trace_row(lr) * l + col, lr.y);
        for (int j = 0; j < 4; j++) o[1 + j] = make_uint2(w.v[2 * j], w.v[2 * j + 1]);
    }
}
}  // namespace lig

namespace {
uint64_t diag_reciprocal(uint32_t d) { return lig::lin_reciprocal(d); }
uint32_t diag_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + lig::LIN_WG - 1) / lig::LIN_WG, 1), lig::DIAG_MAX_BLOCKS); }
using DiagWait = std::function<int()>;      // "the main stream has drained": the way a proof waits (one GPU), or the bounded poll of a shard

// device scratch of one call: freed (after the main stream has drained) when the call returns, whatever way.  hipFree waits for
// every stream of the device, a prefetch of the next trace included.
struct DiagScratch {
    lig_ctx* c;
    std::vector<void*> bufs;
    explicit DiagScratch(lig_ctx* c_) : c(c_) {}
    ~DiagScratch() {
        if (!bufs.empty()) (void)lig_internal_wait_stream(c->stream);
        for (void* p : bufs) (void)hipFree(p);
    }
    void abandon() { bufs.clear(); }       // a poisoned shard: kernels that never drained may still touch the buffers, they outlive the call
    int alloc(void** p, size_t bytes) {
        *p = nullptr;
        const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
        if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string("lig_rows_diagnose: scratch: ") + hipGetErrorString(e); return LIG_E_NOMEM; }
        bufs.push_back(*p);
        return LIG_OK;
    }
};

// What every entry of this file sets up: the context's main stream and shape, the scratch, the temp of the scans and the way the call
// waits -- as a proof does (one GPU), or the bounded poll of a shard (DiagShardFrame).  Sizes are in ELEMENTS.  A host buffer that is the
// source or the target of a queued copy is declared BEFORE the frame: the scratch drains the stream when the frame goes.
struct DiagFrame {
    lig_ctx* const c;
    const hipStream_t s;
    const uint32_t l, k;
    const uint64_t l_recip;
    const DiagWait wait;
    DiagScratch sc;
    void* scan_tmp = nullptr;
    size_t scan_cap = 0;
    explicit DiagFrame(lig_ctx* c_) : DiagFrame(c_, [c = c_, s = c_->stream]() -> int { HIP_TRY(c, lig_internal_wait_stream(s)); return LIG_OK; }) {}
    DiagFrame(lig_ctx* c_, DiagWait w) : c(c_), s(c_->stream), l(c_->l), k(c_->k), l_recip(diag_reciprocal(c_->l)), wait(std::move(w)), sc(c_) {}

    template <class T> int alloc(T*& p, size_t n) { return sc.alloc((void**)&p, n * sizeof(T)); }
    template <class T> int upload(T*& p, const T* host, size_t n) {
        TRY(alloc(p, n));
        if (n) HIP_TRY(c, hipMemcpyAsync(p, host, n * sizeof(T), hipMemcpyHostToDevice, s));
        return LIG_OK;
    }
    template <class T> int download(void* host, const T* dev, size_t n) {
        if (n) HIP_TRY(c, hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
        return LIG_OK;
    }
    template <class T> int fetch(void* host, const T* dev, size_t n) { TRY(download(host, dev, n)); return wait(); }      // ... and blocks until it is there
    template <class T> int zero(T* p, size_t n) { HIP_TRY(c, hipMemsetAsync(p, 0, n * sizeof(T), s)); return LIG_OK; }
    // grid-stride over `items`: diag_grid(items) workgroups of LIN_WG lanes
    template <class... P, class... A> int launch(void (*kernel)(P...), uint64_t items, A... a) {
        hipLaunchKernelGGL(kernel, dim3(diag_grid(items)), dim3(lig::LIN_WG), 0, s, a...);
        HIP_TRY(c, hipGetLastError());
        return LIG_OK;
    }
    // one workgroup per item (the heavy walks, k_explain_finish), at most DIAG_MAX_BLOCKS of them
    template <class... P, class... A> int launch_blocks(void (*kernel)(P...), uint32_t n, A... a) {
        hipLaunchKernelGGL(kernel, dim3(std::min(n, lig::DIAG_MAX_BLOCKS)), dim3(lig::LIN_WG), 0, s, a...);
        HIP_TRY(c, hipGetLastError());
        return LIG_OK;
    }
    // flag[0 .. n] (flag[n] = 0) -> pos[0 .. n] = exclusive scan, enqueued; the temp grows to what the largest scan of the call asks for.
    // Flags: const V*, or an iterator over them (the marks of k_explain_mark read as 0 / 1).  V: uint32_t, or two packed counts in 64 bits.
    template <class Flags, class V> int scan_enqueue(Flags flag, V* pos, size_t n) {
        size_t need = 0;
        HIP_TRY(c, rocprim::exclusive_scan(nullptr, need, flag, pos, V(0), n + 1, rocprim::plus<V>(), s));
        if (need > scan_cap || !scan_tmp) { TRY(sc.alloc(&scan_tmp, need)); scan_cap = need; }
        need = scan_cap;
        HIP_TRY(c, rocprim::exclusive_scan(scan_tmp, need, flag, pos, V(0), n + 1, rocprim::plus<V>(), s));
        return LIG_OK;
    }
    // ... and *count = pos[n] = the number of set flags.  Blocks until it is known.
    template <class Flags, class V> int scan(Flags flag, V* pos, size_t n, V* count) {
        TRY(scan_enqueue(flag, pos, n));
        TRY(download(count, pos + n, 1));
        return wait();
    }
};

// a system on the device, as the linear passes consume it: a constraint-major term list, rhs_index, the constraints with more than HEAVY_MIN
// terms (ascending), the right-hand-side coefficients and a table in Montgomery form.
//   diag_upload_system   the caller's system: the term list as passed, a scratch copy of its table (the table of an attached program is
//                        neither read nor written)
//   diag_regroup_system  the statement attached to the trace: the term list regrouped in scratch; rhs_coef and coef point INTO the program /
//                        the attachment, which nothing here writes
struct DiagSystem {
    uint32_t NC = 0;
    std::vector<uint32_t> heavy;
    uint32_t *tb = nullptr, *rhs_index = nullptr, *heavy_dev = nullptr;
    const uint32_t* rhs_coef = nullptr;
    lig_lin_term* terms = nullptr;
    const fr* coef = nullptr;
};
// the caller's coefficient table -> scratch, converted to Montgomery form there
int diag_upload_table(DiagFrame& f, const lig_linear_system* sys, fr*& d_coef) {
    TRY(f.upload(d_coef, reinterpret_cast<const fr*>(sys->coefs), sys->n_coefs));
    lig::launch_lin_coefs_mont(f.s, d_coef, sys->n_coefs);
    HIP_TRY(f.c, hipGetLastError());
    return LIG_OK;
}
int diag_upload_system(DiagFrame& f, const lig_linear_system* sys, DiagSystem& d) {
    const uint32_t NC = d.NC = (uint32_t)sys->n_constraints, NT = (uint32_t)sys->n_terms, NR = (uint32_t)sys->n_rhs;
    for (uint32_t cn = 0; cn < NC; cn++) if (sys->term_begin[cn + 1] - sys->term_begin[cn] > lig::HEAVY_MIN) d.heavy.push_back(cn);
    uint32_t *d_rhs_c = nullptr, *d_rhs_coef = nullptr; fr* d_coef = nullptr;
    TRY(f.upload(d.tb, sys->term_begin, (size_t)NC + 1));
    TRY(f.upload(d.terms, sys->terms, NT));
    TRY(f.upload(d_rhs_c, sys->rhs_constraint, NR));
    TRY(f.upload(d_rhs_coef, sys->rhs_coef, NR));
    TRY(f.alloc(d.rhs_index, NC));
    TRY(f.upload(d.heavy_dev, d.heavy.data(), d.heavy.size()));
    TRY(diag_upload_table(f, sys, d_coef));
    d.rhs_coef = d_rhs_coef; d.coef = d_coef;
    TRY(f.zero(d.rhs_index, NC));
    if (NR) TRY(f.launch(lig::k_diag_rhs_index, NR, d_rhs_c, NR, nullptr, d.rhs_index));
    return LIG_OK;
}
// The statement attached to the trace (v: prover_common.hpp) -> constraint-major, in scratch: count, scan, scatter (file header).
// Scratch: cbegin (n_constraints + 1) x 4, counters / cursor (n_constraints + 1) x 4, terms n_terms x 8, rhs_index, the short heavy list.
// Blocks once, for the scan's total and the number of heavy constraints.
// One rank's share of a sharded trace (v.sharded): compact = false numbers the segments as the whole trace does, through need[] -- for the
// rank that holds every row, whose local slots are the trace's; compact = true keeps the rank's own numbers: d.NC = n_need segments, d.tb,
// d.rhs_index and d.heavy all over i < n_need, local slots (lig_shard_rows_diagnose_attached).
int diag_regroup_system(DiagFrame& f, const lig_linear_view& v, bool compact, DiagSystem& d) {
    lig_ctx* c = f.c;
    hipStream_t s = f.s;
    const uint32_t NC = d.NC = (uint32_t)(compact ? v.n_need : v.n_constraints), NT = (uint32_t)v.n_terms, NR = (uint32_t)v.n_rhs;
    const uint32_t* number = v.sharded && !compact ? v.need : nullptr;
    const uint32_t heavy_cap = NT / (lig::HEAVY_MIN + 1) + 1;
    uint32_t *d_cursor = nullptr, *d_nheavy = nullptr;
    TRY(f.alloc(d.tb, (size_t)NC + 1));
    TRY(f.alloc(d_cursor, (size_t)NC + 1));
    TRY(f.alloc(d.terms, NT));
    TRY(f.alloc(d.rhs_index, NC));
    TRY(f.alloc(d.heavy_dev, heavy_cap));
    TRY(f.alloc(d_nheavy, 1));
    d.rhs_coef = v.rhs_coef; d.coef = v.coef;
    // values set on the side stream (lig_rows_set_linear_values): the passes below read the table once its conversion has finished
    if (v.coef_ready) HIP_TRY(c, hipStreamWaitEvent(s, v.coef_ready, 0));
    TRY(f.zero(d_cursor, (size_t)NC + 1));
    TRY(f.zero(d_nheavy, 1));
    if (NT) TRY(f.launch(lig::k_diag_att_count, NT, v.ent, NT, number, d_cursor));
    TRY(f.launch(lig::k_diag_att_classify, NC, d_cursor, NC, d.heavy_dev, heavy_cap, d_nheavy));
    uint32_t total = 0, n_heavy = 0;
    TRY(f.download(&n_heavy, d_nheavy, 1));
    const int rc = f.scan(d_cursor, d.tb, NC, &total);
    if (rc != LIG_OK) { (void)f.wait(); return rc; }      // (the copy into n_heavy may still be queued)
    if (total != NT || n_heavy > heavy_cap) FAIL(c, LIG_E_STATE, "lig_rows_diagnose_attached: the attached program's index does not add up to its term count");
    if (n_heavy) {      // ascending: the same launch geometry whatever order the atomics appended them in
        d.heavy.resize(n_heavy);
        TRY(f.fetch(d.heavy.data(), d.heavy_dev, n_heavy));
        std::sort(d.heavy.begin(), d.heavy.end());
        HIP_TRY(c, hipMemcpyAsync(d.heavy_dev, d.heavy.data(), (size_t)n_heavy * 4, hipMemcpyHostToDevice, s));
    }
    TRY(f.zero(d_cursor, (size_t)NC + 1));
    if (NT) TRY(f.launch(lig::k_diag_att_scatter, NT, v.ent, NT, v.begin, v.n_slots, number, d.tb, d_cursor, d.terms));
    TRY(f.zero(d.rhs_index, NC));
    if (NR) TRY(f.launch(lig::k_diag_rhs_index, NR, v.rhs_c, NR, number, d.rhs_index));
    return LIG_OK;
}

// The quadratic terms tri_dev[0 .. n_terms) over `msgs`, in slices of at most DIAG_QUAD_ITEMS items; the running count and the output offset
// are carried on the host.  The first `cap` records go to host_out slice by slice (one GPU), or -- host_out == NULL -- stay on the device in
// dev_out[0 .. cap) with the terms' ordinals in ord_out (a rank of a shard: rows through grow_dev, ordinals from ord_dev).
int diag_quad_pass(DiagFrame& f, const fr* msgs, const uint32_t* tri_dev, uint64_t n_terms, uint64_t cap, lig_diag_quad* host_out, lig_diag_quad* dev_out,
                   const uint32_t* grow_dev, const uint32_t* ord_dev, uint32_t* ord_out, uint64_t* bad_total_out, uint64_t* reported_out) {
    const uint32_t l = f.l;
    const uint64_t per = std::max<uint64_t>(lig::DIAG_QUAD_ITEMS / l, 1);        // terms per slice: per * l < 2^32 (l < 2^32, and per = 1 beyond the budget)
    const uint64_t slice_items = std::min(per, n_terms) * l;
    uint32_t *d_flag = nullptr, *d_pos = nullptr; fr* d_res = nullptr;
    TRY(f.alloc(d_res, slice_items));
    TRY(f.alloc(d_flag, (size_t)slice_items + 1));
    TRY(f.alloc(d_pos, (size_t)slice_items + 1));
    if (host_out || !dev_out) {
        const uint64_t out_cap = std::min<uint64_t>(cap, slice_items);
        if (out_cap) TRY(f.alloc(dev_out, out_cap));
    }
    uint64_t bad_total = 0, reported = 0;
    for (uint64_t t0 = 0; t0 < n_terms; t0 += per) {
        const uint32_t items = (uint32_t)(std::min(per, n_terms - t0) * l);
        TRY(f.zero(d_flag + items, 1));
        TRY(f.launch(lig::k_diag_quad, items, tri_dev, (uint32_t)t0, items, msgs, l, f.k, f.l_recip, d_res, d_flag));
        uint32_t bad = 0;
        TRY(f.scan(d_flag, d_pos, items, &bad));
        if (bad > items) FAIL(f.c, LIG_E_STATE, "lig_rows_diagnose: counted more violated items than the slice holds");
        bad_total += bad;
        const uint32_t rep = (uint32_t)std::min<uint64_t>(bad, cap - reported);
        if (rep) {
            const uint64_t at = host_out ? 0 : reported;
            TRY(f.launch(lig::k_diag_scatter_quad, items, d_flag, d_pos, d_res, tri_dev, (uint32_t)t0, items, l, f.l_recip, rep, dev_out + at, grow_dev, ord_dev,
                         ord_out ? ord_out + at : nullptr));
            if (host_out) TRY(f.fetch(host_out + reported, dev_out, rep));
            reported += rep;
        }
    }
    *bad_total_out = bad_total;
    *reported_out = reported;
    return LIG_OK;
}
}  // namespace

namespace {
// The two one-GPU entries.  msgs: the committed rows x k witness matrix; tri_dev / n_quad_terms: the quadratic terms of the trace (quad_terms(),
// rows_plan.hpp).  The linear statement is `sys` (it has passed lig_linear_check against the trace's kinds) or `att` (the view of the trace's
// attachment), at most one of them: where the DiagSystem comes from is all that differs.  Waits with lig_internal_wait_stream (prover.hip: bounded
// spin, then the blocking wait).
int diag_rows(lig_ctx* c, const fr* msgs, uint64_t rows, const uint32_t* tri_dev, uint64_t n_quad_terms, const lig_linear_system* sys, const lig_linear_view* att,
              lig_diag_linear* lin_out, uint64_t lin_cap, lig_diag_quad* quad_out, uint64_t quad_cap, lig_diag_info* info) {
    DiagFrame f(c);
    const uint32_t l = f.l, k = f.k;

    // ---------------------------------------------------------------- linear constraints
    if (sys ? sys->n_constraints : att ? att->n_constraints : 0) {
        DiagSystem d;
        if (sys) TRY(diag_upload_system(f, sys, d));
        else TRY(diag_regroup_system(f, *att, false, d));
        const uint32_t NC = d.NC, NH = (uint32_t)d.heavy.size();
        uint32_t *d_flag = nullptr, *d_pos = nullptr; fr* d_res = nullptr;
        TRY(f.alloc(d_res, NC));
        TRY(f.alloc(d_flag, (size_t)NC + 1));
        TRY(f.alloc(d_pos, (size_t)NC + 1));
        TRY(f.zero(d_flag, (size_t)NC + 1));
        TRY(f.launch(lig::k_diag_lin, NC, d.tb, d.terms, NC, msgs, l, k, f.l_recip, d.coef, d.rhs_index, d.rhs_coef, d_res, d_flag));
        if (NH) TRY(f.launch_blocks(lig::k_diag_lin_heavy, NH, d.heavy_dev, NH, d.tb, d.terms, msgs, l, k, f.l_recip, d.coef, d.rhs_index, d.rhs_coef, d_res, d_flag));
        uint32_t bad = 0;
        TRY(f.scan(d_flag, d_pos, NC, &bad));
        if (bad > NC) FAIL(c, LIG_E_STATE, "lig_rows_diagnose: counted more violated constraints than the system holds");
        info->n_linear_bad = bad;
        const uint32_t rep = (uint32_t)std::min<uint64_t>(bad, lin_cap);
        if (rep) {
            lig_diag_linear* d_out = nullptr;
            TRY(f.alloc(d_out, rep));
            TRY(f.launch(lig::k_diag_scatter_lin, NC, d_flag, d_pos, d_res, NC, 0u, rep, d_out));
            TRY(f.fetch(lin_out, d_out, rep));
        }
        info->n_linear_reported = rep;
    }

    // ---------------------------------------------------------------- quadratic terms
    if (n_quad_terms && rows)
        TRY(diag_quad_pass(f, msgs, tri_dev, n_quad_terms, quad_cap, quad_out, nullptr, nullptr, nullptr, nullptr, &info->n_quad_bad, &info->n_quad_reported));
    return LIG_OK;
}
}  // namespace

int lig_internal_rows_diagnose(lig_ctx* c, const fr* msgs, uint64_t rows, const uint32_t* tri_dev, uint64_t n_quad_terms, const lig_linear_system* sys,
                               lig_diag_linear* lin_out, uint64_t lin_cap, lig_diag_quad* quad_out, uint64_t quad_cap, lig_diag_info* info) {
    return diag_rows(c, msgs, rows, tri_dev, n_quad_terms, sys, nullptr, lin_out, lin_cap, quad_out, quad_cap, info);
}
int lig_internal_rows_diagnose_attached(lig_ctx* c, const fr* msgs, uint64_t rows, const uint32_t* tri_dev, uint64_t n_quad_terms, const lig_linear* att,
                                        lig_diag_linear* lin_out, uint64_t lin_cap, lig_diag_quad* quad_out, uint64_t quad_cap, lig_diag_info* info) {
    // (a sharded share: the caller is the ONE rank of its world and holds every row in commit order -- its local slots are the trace's, and
    // diag_regroup_system numbers the segments through need[])
    const lig_linear_view v = lig_internal_linear_view(att);
    return diag_rows(c, msgs, rows, tri_dev, n_quad_terms, nullptr, &v, lin_out, lin_cap, quad_out, quad_cap, info);
}

namespace {
// The tail every explain entry ends with: the items in output order (explain_order / explain_merge) -> the two record arrays.
//   explain_upload    the m ordered terms, the asked index of the first `rep` of them and first[0 .. NA] -> scratch.  o holds the sources of
//                     the queued uploads: it is declared before the frame.
//   explain_records   k_explain_fill / k_explain_finish over them with the witness source `wit`, both arrays to the host.  Blocks once.
//                     terms_out may be NULL when rep = 0 (lig_internal_rows_explain_slots asks for the constraint records alone).
// What lies between the two stays with the entry (the value exchange of a shard, which reads d_ordered).
struct ExplainOrdered {
    std::vector<lig_lin_term> ordered;
    std::vector<uint32_t> ask, first32;
    uint32_t m = 0, rep = 0, NA = 0;
    lig_lin_term* d_ordered = nullptr; uint32_t *d_ask = nullptr, *d_first = nullptr;
};
int explain_upload(DiagFrame& f, const std::vector<lig::ExplainItem>& items, const std::vector<uint64_t>& first, uint32_t NA, uint32_t rep, ExplainOrdered& o) {
    o.m = (uint32_t)items.size(); o.rep = rep; o.NA = NA;
    o.ordered.resize(o.m);
    o.ask.resize(rep);
    o.first32.assign(first.begin(), first.end());
    for (uint32_t i = 0; i < o.m; i++) { o.ordered[i].slot = items[i].slot; o.ordered[i].coef = items[i].coef; }
    for (uint32_t i = 0; i < rep; i++) o.ask[i] = items[i].ask;
    TRY(f.upload(o.d_ordered, o.ordered.data(), o.m));
    TRY(f.upload(o.d_ask, o.ask.data(), rep));
    return f.upload(o.d_first, o.first32.data(), (size_t)NA + 1);
}
template <class Wit>
int explain_records(DiagFrame& f, const ExplainOrdered& o, const uint32_t* d_asked, const Wit& wit, const fr* coef, const uint32_t* rhs_index, const uint32_t* rhs_coef,
                    lig_explain_constraint* con_out, lig_explain_term* terms_out) {
    lig_explain_constraint* d_con = nullptr; lig_explain_term* d_out = nullptr;
    TRY(f.alloc(d_con, o.NA));
    TRY(f.alloc(d_out, o.rep));
    if (o.rep) TRY(f.launch(lig::k_explain_fill<Wit>, o.rep, o.d_ordered, o.d_ask, o.rep, d_asked, wit, coef, d_out));
    TRY(f.launch_blocks(lig::k_explain_finish<Wit>, o.NA, o.d_first, o.d_ordered, d_asked, o.NA, wit, coef, rhs_index, rhs_coef, d_con));
    TRY(f.download(con_out, d_con, o.NA));
    TRY(f.download(terms_out, d_out, o.rep));
    return f.wait();
}

// The two explain entries (lig_hip.h).  The statement is `sys` (it has passed lig_linear_check against the trace's kinds) or `att` (the view of
// the trace's attachment, not sharded), exactly one of them; asked[0 .. n_asked) has passed explain_asked_ok against its constraint count and
// n_asked > 0.  Where the unordered items come from is all that differs (the kernels' header above).  Blocks twice: for the items (ordered on
// the host), and for the records.
int explain_rows(lig_ctx* c, const fr* msgs, const lig_linear_system* sys, const lig_linear_view* att, const uint32_t* asked, uint64_t n_asked,
                 lig_explain_constraint* con_out, lig_explain_term* terms_out, uint64_t term_cap, lig_explain_info* info) {
    const uint32_t NA = (uint32_t)n_asked;
    // (sources and targets of queued copies: declared before the frame, whose scratch drains the stream when it goes)
    std::vector<lig::ExplainItem> items;
    std::vector<uint64_t> first;
    std::vector<uint32_t> pre;
    ExplainOrdered o;
    DiagFrame f(c);

    uint32_t* d_asked = nullptr; lig::ExplainItem* d_items = nullptr;
    TRY(f.upload(d_asked, asked, NA));
    DiagSystem d;
    uint32_t m = 0;
    if (sys) {
        TRY(diag_upload_system(f, sys, d));
        pre.assign((size_t)NA + 1, 0);
        for (uint32_t a = 0; a < NA; a++) pre[a + 1] = pre[a] + (sys->term_begin[asked[a] + 1] - sys->term_begin[asked[a]]);      // <= n_terms < 2^32: the asked are distinct
        m = pre[NA];
        uint32_t* d_pre = nullptr;
        TRY(f.upload(d_pre, pre.data(), (size_t)NA + 1));
        TRY(f.alloc(d_items, m));
        if (m) TRY(f.launch(lig::k_explain_gather, m, d.tb, d.terms, d_asked, NA, d_pre, m, d_items));
    } else {
        const lig_linear_view& v = *att;
        const uint32_t NC = d.NC = (uint32_t)v.n_constraints, NT = (uint32_t)v.n_terms, NR = (uint32_t)v.n_rhs;
        uint32_t *d_mark = nullptr, *d_pos = nullptr;
        TRY(f.alloc(d_mark, (size_t)NT + 1));
        TRY(f.alloc(d_pos, (size_t)NT + 1));
        TRY(f.alloc(d.rhs_index, NC));
        d.rhs_coef = v.rhs_coef; d.coef = v.coef;
        // values set on the side stream (lig_rows_set_linear_values): the table is read once its conversion has finished
        if (v.coef_ready) HIP_TRY(c, hipStreamWaitEvent(f.s, v.coef_ready, 0));
        TRY(f.zero(d_mark + NT, 1));
        if (NT) TRY(f.launch(lig::k_explain_mark, NT, v.ent, NT, nullptr, d_asked, NA, d_mark));
        TRY(f.scan(rocprim::make_transform_iterator((const uint32_t*)d_mark, lig::ExplainMarked{}), d_pos, NT, &m));
        if (m > NT) FAIL(c, LIG_E_STATE, "lig_rows_explain_attached: counted more asked terms than the attached program holds");
        TRY(f.alloc(d_items, m));
        if (m) TRY(f.launch(lig::k_explain_collect, NT, v.ent, NT, v.begin, v.n_slots, d_mark, d_pos, d_items));
        TRY(f.zero(d.rhs_index, NC));
        if (NR) TRY(f.launch(lig::k_diag_rhs_index, NR, v.rhs_c, NR, nullptr, d.rhs_index));
    }
    // the m items -> the output order, on the host (explain_plan.hpp)
    items.resize(m);
    TRY(f.fetch(items.data(), d_items, m));
    if (!lig::explain_order(items, NA, first)) FAIL(c, LIG_E_STATE, "lig_rows_explain: a collected term names no asked constraint");
    const uint32_t rep = (uint32_t)std::min<uint64_t>(m, term_cap);
    TRY(explain_upload(f, items, first, NA, rep, o));
    TRY(explain_records(f, o, d_asked, lig::ExplainFromMatrix{msgs, f.l, f.k, f.l_recip}, d.coef, d.rhs_index, d.rhs_coef, con_out, terms_out));
    info->n_terms_total = m;
    info->n_terms_reported = rep;
    return LIG_OK;
}
}  // namespace

int lig_internal_rows_explain(lig_ctx* c, const fr* msgs, const lig_linear_system* sys, const uint32_t* asked, uint64_t n_asked, lig_explain_constraint* con_out,
                              lig_explain_term* terms_out, uint64_t term_cap, lig_explain_info* info) {
    if (!lig::explain_asked_ok(asked, n_asked, sys->n_constraints))
        FAIL(c, LIG_E_ARG, "lig_rows_explain: the asked constraints must be strictly ascending and below n_constraints");
    if (!n_asked) return LIG_OK;
    return explain_rows(c, msgs, sys, nullptr, asked, n_asked, con_out, terms_out, term_cap, info);
}
int lig_internal_rows_explain_attached(lig_ctx* c, const fr* msgs, const lig_linear* att, const uint32_t* asked, uint64_t n_asked, lig_explain_constraint* con_out,
                                       lig_explain_term* terms_out, uint64_t term_cap, lig_explain_info* info) {
    const lig_linear_view v = lig_internal_linear_view(att);
    if (v.sharded) FAIL(c, LIG_E_STATE, "lig_rows_explain_attached: the attached structure is one rank's share of a sharded trace");
    if (!lig::explain_asked_ok(asked, n_asked, v.n_constraints))
        FAIL(c, LIG_E_ARG, "lig_rows_explain_attached: the asked constraints must be strictly ascending and below n_constraints");
    if (!n_asked) return LIG_OK;
    return explain_rows(c, msgs, nullptr, &v, asked, n_asked, con_out, terms_out, term_cap, info);
}
// lig_rows_read_slots: values[i] = the canonical w[slots[i]] of the committed rows x k matrix; every slot < rows * l (checked here, before
// anything is launched).  In pieces of 2^24 slots.
int lig_internal_rows_read_slots(lig_ctx* c, const fr* msgs, uint64_t rows, const uint32_t* slots, uint64_t n_slots, uint8_t* values) {
    if (!lig::explain_slots_ok(slots, n_slots, rows, c->l)) FAIL(c, LIG_E_ARG, "lig_rows_read_slots: a slot is not below rows * l");
    if (!n_slots) return LIG_OK;
    const uint64_t piece = std::min<uint64_t>(n_slots, 1ull << 24);
    DiagFrame f(c);
    uint32_t* d_slots = nullptr; fr* d_val = nullptr;
    TRY(f.alloc(d_slots, piece));
    TRY(f.alloc(d_val, piece));
    for (uint64_t at = 0; at < n_slots; at += piece) {
        const uint32_t n = (uint32_t)std::min(piece, n_slots - at);
        HIP_TRY(c, hipMemcpyAsync(d_slots, slots + at, (size_t)n * 4, hipMemcpyHostToDevice, f.s));
        TRY(f.launch(lig::k_read_slots, n, d_slots, n, msgs, f.l, f.k, f.l_recip, d_val));
        TRY(f.fetch(values + at * 32, d_val, n));
    }
    return LIG_OK;
}

// lig_rows_explain_slots / lig_rows_explain_slots_attached (lig_hip.h; the kernels' header above).  v: the view of the trace's attachment, or
// of the temporary program the caller made from its term list -- not sharded, over the rows x l slots of this trace (checked here).  kinds:
// one per committed row.  Blocks for the prefix sums, for the items (ordered on the host), inside explain_rows for the distinct
// constraints, and for the records.
int lig_internal_rows_explain_slots(lig_ctx* c, const fr* msgs, const uint8_t* kinds, uint64_t rows, const lig_linear_view& v, const uint32_t* slots, uint64_t n_asked,
                                    lig_slot_record* slot_out, lig_slot_term* terms_out, uint64_t term_cap, lig_slot_info* info) {
    if (v.sharded) FAIL(c, LIG_E_STATE, "lig_rows_explain_slots: the attached structure is one rank's share of a sharded trace");
    if ((uint64_t)v.n_slots != rows * (uint64_t)c->l) FAIL(c, LIG_E_STATE, "lig_rows_explain_slots: the program does not cover the slots of this trace");
    if (!lig::explain_slots_ok(slots, n_asked, rows, c->l)) FAIL(c, LIG_E_ARG, "lig_rows_explain_slots: a slot is not below rows * l");
    for (uint64_t i = 1; i < n_asked; i++) if (slots[i] <= slots[i - 1]) FAIL(c, LIG_E_ARG, "lig_rows_explain_slots: the asked slots must be strictly ascending");
    if (!n_asked) return LIG_OK;
    const uint32_t l = c->l, NA = (uint32_t)n_asked, NT = (uint32_t)v.n_terms;
    // (sources and targets of queued copies: declared before the frame, whose scratch drains the stream when it goes)
    std::vector<uint32_t> pre((size_t)NA + 1), heavy, distinct, cidx;
    std::vector<lig::ExplainItem> items;
    std::vector<uint64_t> first;
    std::vector<lig_explain_constraint> con;
    std::vector<fr> vals(NA);
    DiagFrame f(c);

    uint32_t *d_slots = nullptr, *d_len = nullptr, *d_pre = nullptr; fr* d_val = nullptr;
    TRY(f.upload(d_slots, slots, NA));
    TRY(f.alloc(d_len, (size_t)NA + 1));
    TRY(f.alloc(d_pre, (size_t)NA + 1));
    TRY(f.alloc(d_val, NA));
    TRY(f.zero(d_len + NA, 1));
    TRY(f.launch(lig::k_slot_len, NA, d_slots, NA, v.begin, d_len));
    TRY(f.launch(lig::k_read_slots, NA, d_slots, NA, msgs, l, f.k, f.l_recip, d_val));
    TRY(f.download(vals.data(), d_val, NA));
    TRY(f.scan_enqueue(d_len, d_pre, NA));
    TRY(f.fetch(pre.data(), d_pre, (size_t)NA + 1));
    const uint32_t m = pre[NA];
    // distinct slots own disjoint segments: the lengths add up to at most n_terms, every prefix sum is exact in 32 bits
    if (m > NT || !std::is_sorted(pre.begin(), pre.end())) FAIL(c, LIG_E_STATE, "lig_rows_explain_slots: the program's index does not add up to its term count");
    for (uint32_t a = 0; a < NA; a++) if (pre[a + 1] - pre[a] > lig::HEAVY_MIN) heavy.push_back(a);

    lig::ExplainItem* d_items = nullptr;
    TRY(f.alloc(d_items, m));
    if (m) TRY(f.launch(lig::k_slot_collect, m, d_slots, NA, d_pre, m, v.begin, v.ent, d_items));
    if (!heavy.empty()) {
        uint32_t* d_heavy = nullptr;
        TRY(f.upload(d_heavy, heavy.data(), heavy.size()));
        TRY(f.launch_blocks(lig::k_slot_collect_heavy, (uint32_t)heavy.size(), d_heavy, (uint32_t)heavy.size(), d_slots, d_pre, v.begin, v.ent, d_items));
    }
    items.resize(m);
    TRY(f.fetch(items.data(), d_items, m));
    // the m items -> the output order (asked slot, constraint, coefficient index), on the host; the distinct constraints, ascending
    if (!lig::explain_order(items, NA, first)) FAIL(c, LIG_E_STATE, "lig_rows_explain_slots: a collected term names no asked slot");
    distinct.resize(m);
    for (uint32_t i = 0; i < m; i++) {
        if (items[i].slot >= v.n_constraints) FAIL(c, LIG_E_STATE, "lig_rows_explain_slots: an entry of the program names no constraint");
        distinct[i] = items[i].slot;
    }
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    const uint32_t ND = (uint32_t)distinct.size(), rep = (uint32_t)std::min<uint64_t>(m, term_cap);
    // their sizes and residuals: the attached selection pass itself, asked for the constraint records alone
    con.resize(ND);
    if (ND) {
        lig_explain_info einfo;
        std::memset(&einfo, 0, sizeof einfo);
        TRY(explain_rows(c, msgs, nullptr, &v, distinct.data(), ND, con.data(), nullptr, 0, &einfo));
    }
    if (rep) {
        cidx.resize(rep);
        for (uint32_t i = 0; i < rep; i++) cidx[i] = (uint32_t)(std::lower_bound(distinct.begin(), distinct.end(), items[i].slot) - distinct.begin());
        uint32_t* d_cidx = nullptr; lig_explain_constraint* d_con = nullptr; lig_slot_term* d_out = nullptr;
        HIP_TRY(c, hipMemcpyAsync(d_items, items.data(), (size_t)rep * sizeof(lig::ExplainItem), hipMemcpyHostToDevice, f.s));      // the ordered ones over the collected
        TRY(f.upload(d_cidx, cidx.data(), rep));
        TRY(f.upload(d_con, con.data(), ND));
        TRY(f.alloc(d_out, rep));
        // values set on the side stream (lig_rows_set_linear_values): the table is read once its conversion has finished
        if (v.coef_ready) HIP_TRY(c, hipStreamWaitEvent(f.s, v.coef_ready, 0));
        TRY(f.launch(lig::k_slot_fill, rep, d_items, d_cidx, rep, d_slots, d_con, v.coef, d_out));
        TRY(f.fetch(terms_out, d_out, rep));
    }
    for (uint32_t a = 0; a < NA; a++) {
        lig_slot_record& r = slot_out[a];
        std::memset(&r, 0, sizeof r);
        r.slot = slots[a]; r.row_kind = kinds[slots[a] / l] & 0x7fu;
        r.n_terms = pre[a + 1] - pre[a]; r.first_term = first[a];
        std::memcpy(r.value, vals[a].v, 32);
    }
    info->n_terms_total = m;
    info->n_terms_reported = rep;
    info->n_constraints_distinct = ND;
    return LIG_OK;
}

// lig_rows_untouched_slots / lig_rows_untouched_slots_attached (lig_hip.h; the kernels' header above): v and kinds as for
// lig_internal_rows_explain_slots.  The slots of the LINEAR .. QZ rows in slices of UNTOUCHED_ITEMS; blocks once per slice for the two
// counts, and once more for the records of a slice that reports some.
int lig_internal_rows_untouched_slots(lig_ctx* c, const fr* msgs, const uint8_t* kinds, uint64_t rows, const lig_linear_view& v, int nonzero_only, lig_slot_value* out,
                                      uint64_t cap, lig_untouched_info* info) {
    static constexpr uint64_t UNTOUCHED_ITEMS = lig::DIAG_UNTOUCHED_ITEMS;
    if (v.sharded) FAIL(c, LIG_E_STATE, "lig_rows_untouched_slots: the attached structure is one rank's share of a sharded trace");
    if ((uint64_t)v.n_slots != rows * (uint64_t)c->l) FAIL(c, LIG_E_STATE, "lig_rows_untouched_slots: the program does not cover the slots of this trace");
    const uint32_t l = c->l;
    std::vector<uint2> lrows;      // (source of a queued copy: declared before the frame)
    for (uint64_t r = 0; r < rows; r++) if ((kinds[r] & 0x7fu) <= LIG_ROW_QZ) lrows.push_back(make_uint2((uint32_t)r, kinds[r] & 0x7fu));
    const uint64_t NL = lrows.size();
    if (!NL) return LIG_OK;
    DiagFrame f(c);
    const uint64_t per = std::max<uint64_t>(UNTOUCHED_ITEMS / l, 1);      // rows per slice: per * l < 2^32 (rows * l < 2^32: lig_linear_check)
    const uint64_t slice_items = std::min(per, NL) * l, out_cap = std::min<uint64_t>(cap, slice_items);
    uint2* d_lrows = nullptr; uint64_t *d_flag = nullptr, *d_pos = nullptr; lig_slot_value* d_out = nullptr;
    TRY(f.upload(d_lrows, lrows.data(), NL));
    TRY(f.alloc(d_flag, (size_t)slice_items + 1));
    TRY(f.alloc(d_pos, (size_t)slice_items + 1));
    if (out_cap) TRY(f.alloc(d_out, out_cap));
    uint64_t n_untouched = 0, n_nonzero = 0, reported = 0;
    for (uint64_t r0 = 0; r0 < NL; r0 += per) {      // (the first slice is the largest: its scan sizes the temp for all of them)
        const uint32_t items = (uint32_t)(std::min(per, NL - r0) * l);
        TRY(f.zero(d_flag + items, 1));
        TRY(f.launch(lig::k_untouched_flag<uint2>, items, d_lrows, (uint32_t)r0, items, v.begin, msgs, l, f.k, f.l_recip, d_flag));
        uint64_t both = 0;      // the two counts of the slice, packed
        TRY(f.scan(d_flag, d_pos, items, &both));
        const uint32_t un = (uint32_t)both, nz = (uint32_t)(both >> 32);
        if (un > items || nz > un) FAIL(c, LIG_E_STATE, "lig_rows_untouched_slots: counted more slots than the slice holds");
        n_untouched += un; n_nonzero += nz;
        const uint32_t rep = (uint32_t)std::min<uint64_t>(nonzero_only ? nz : un, cap - reported);
        if (rep) {
            TRY(f.launch(lig::k_untouched_compact<uint2>, items, d_flag, d_pos, d_lrows, (uint32_t)r0, items, msgs, l, f.k, f.l_recip, nonzero_only ? 1u : 0u, rep, d_out));
            TRY(f.fetch(out + reported, d_out, rep));
            reported += rep;
        }
    }
    info->n_untouched = n_untouched;
    info->n_untouched_nonzero = n_nonzero;
    info->n_reported = reported;
    return LIG_OK;
}

namespace {
// The frame of one rank's call on a sharded rows job (v: prover_common.hpp): it waits with v.drain(who), the bounded poll, issues the
// collectives and holds the rule every such entry ends by -- run(): a poisoned shard abandons its scratch; otherwise the stream drains and
// v.forget runs BEFORE the frame goes and frees a send buffer (lig_comm.forget).  Every send buffer is an allocation of its own.
// LIG_TRACE: mark(p) closes phase p with a wait, a synchronised split of the call on stderr, one line per successful call:
//   [lig_trace] <name> rank <r>: <phase> <ms> ... ms
// alone (lig_shard_rows_explain_attached): the one rank of its world -- a device copy in place of every all-gather, no collective.
struct DiagShardFrame : DiagFrame {
    const lig_diag_shard& v;
    const char* const name;
    const std::vector<const char*> phases;
    const bool alone, trace_on = lig::knobs().trace;
    bool used_comm = false;
    std::vector<double> ph;
    clk::time_point t_mark = clk::now();
    DiagShardFrame(lig_ctx* c_, const lig_diag_shard& v_, const char* who, const char* name_, std::initializer_list<const char*> phases_, bool alone_ = false)
        : DiagFrame(c_, [&v_, who]() -> int { return v_.drain(who); }), v(v_), name(name_), phases(phases_), alone(alone_), ph(phases_.size(), 0.0) {}

    int mark(int p) {
        if (!trace_on) return LIG_OK;
        TRY(wait());
        ph[p] += ms_since(t_mark);
        t_mark = clk::now();
        return LIG_OK;
    }
    int all_to_all(const void* src, void* dst, size_t bytes, const char* what) {
        used_comm = true;
        return v.all_to_all(src, dst, bytes, what);
    }
    int all_gather(const void* src, void* dst, size_t bytes, const char* what) {
        if (alone) { HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s)); return LIG_OK; }
        used_comm = true;
        return v.all_gather(src, dst, bytes, what);
    }
    template <class Body> int run(Body body) {
        const int rc = body();
        if (rc != LIG_OK && v.settle_failed()) { sc.abandon(); return rc; }      // poisoned: the scratch outlives the call
        if (rc == LIG_OK) (void)wait();
        if (used_comm) v.forget();                                                // before any send buffer is freed
        if (trace_on && rc == LIG_OK) {
            char num[32];
            std::string line = std::string("[lig_trace] ") + name + " rank " + std::to_string(v.rank) + ":";
            for (size_t p = 0; p < phases.size(); p++) { std::snprintf(num, sizeof num, " %.3f", ph[p]); line += std::string(" ") + phases[p] + num; }
            std::fprintf(stderr, "%s ms\n", line.c_str());
        }
        return rc;
    }
};
// the rank's global -> local row table (LIN_NOT_LOCAL: another rank holds that row) -> scratch; local_of is the source of the queued upload
int diag_row_table(DiagFrame& f, const lig_diag_shard& v, std::vector<uint32_t>& local_of, uint32_t*& d_local) {
    local_of.assign(v.rows_global, lig::LIN_NOT_LOCAL);
    for (size_t lr = 0; lr < v.grow->size(); lr++) local_of[(*v.grow)[lr]] = (uint32_t)lr;
    return f.upload(d_local, local_of.data(), local_of.size());
}
}  // namespace

// One rank of a sharded rows job (lig_shard_rows_diagnose, lig_hip.h; v: prover_common.hpp).  Collective: whether a collective is issued,
// how many and of which size depends on sys' sizes, the caps, the world size and the slice knob alone -- never on what this rank holds.
//   linear     constraints in slices of W * B; sub-block h of a slice (B contiguous constraints) is owned by rank h.  Per slice: partials of
//              the whole slice (k_diag_lin_part*), ONE all-to-all of B x 32 bytes per pair, k_diag_reduce on the owner's sub-block, scan,
//              scatter behind the owner's earlier records (at most lin_cap of them are kept).  Then one all-gather of
//              [count, kept | lin_cap' records] and a merge into ascending constraint order on the host of every rank.
//   quadratic  every term is local to one rank: the one-GPU pass over the local terms, global rows through `grow`, at most quad_cap records
//              kept with the terms' global ordinals; one all-gather of [count, kept | records | ordinals], merged by (ordinal, column).
// Every send buffer is an allocation of its own; v.forget runs before any of them is freed.
// The linear statement is `sys` (the term list of the WHOLE trace; it has passed lig_linear_check) or `att` (the view of the rank's share
// attached to the shard), at most one of them.  Where the partials of a slice come from is all that differs:
//   sys   the uploaded list walked through the rank's global -> local row table (k_diag_lin_part*); the owner subtracts b_c (k_diag_reduce<true>)
//   att   the share regrouped by compact constraint (diag_regroup_system), the slice as a compact range (k_diag_att_bounds), the send buffer
//         zeroed, k_diag_att_part* with b_c subtracted by its one holder; the owner only adds (k_diag_reduce<false>).  No host pass over the
//         terms, no upload; the table in force is read in place behind its event.  Scratch instead of the uploaded system:
//         8 kept terms + 12 (n_need + 1) + 4 (slices + 1) and the short heavy lists.
namespace {
int shard_diagnose(const char* who, lig_ctx* c, const lig_diag_shard& v, const lig_linear_system* sys, const lig_linear_view* att, lig_diag_linear* lin_out,
                   uint64_t lin_cap, lig_diag_quad* quad_out, uint64_t quad_cap, lig_diag_info* info) {
    const uint32_t W = v.world;
    // (sources and targets of queued copies: declared before the frame, whose scratch drains the stream when it goes)
    std::vector<uint32_t> local_of, grow32, ord32, heavy_global;
    std::vector<uint8_t> gathered;
    uint64_t header[2] = {0, 0}, qheader[2] = {0, 0};
    enum { PH_PARTIAL, PH_EXCHANGE, PH_REDUCE, PH_RECORDS, PH_QUAD };
    DiagShardFrame f(c, v, who, att ? "shard_diagnose_attached" : "shard_diagnose", {"partial", "exchange", "reduce", "records", "quadratic"});
    hipStream_t s = f.s;
    const uint32_t l = f.l, k = f.k;
    const uint64_t l_recip = f.l_recip;

    return f.run([&]() -> int {
        // ---------------------------------------------------------------- linear constraints
        if (sys ? sys->n_constraints : att ? att->n_constraints : 0) {
            DiagSystem d;
            const uint32_t NC = (uint32_t)(sys ? sys->n_constraints : att->n_constraints);      // constraints of the WHOLE trace
            uint32_t *d_local = nullptr, *d_bound = nullptr;
            if (sys) {
                TRY(diag_upload_system(f, sys, d));
                TRY(diag_row_table(f, v, local_of, d_local));
            } else {
                if (att->rows_local != v.grow->size()) FAIL(c, LIG_E_STATE, std::string(who) + ": the attached share was made for another deal");
                TRY(diag_regroup_system(f, *att, true, d));
            }
            const uint64_t SL = std::max<uint64_t>(v.slice, 1);
            const uint32_t B = (uint32_t)(NC <= SL ? ((uint64_t)NC + W - 1) / W : std::max<uint64_t>(SL / W, 1));      // constraints per sub-block
            const uint64_t SE = (uint64_t)B * W, n_slices = (NC + SE - 1) / SE;                                         // constraints per slice, slices
            const uint64_t rec_cap = std::min<uint64_t>(lin_cap, n_slices * B);                                          // no owner has more to report
            const size_t blk = 16 + (size_t)rec_cap * sizeof(lig_diag_linear);
            fr *d_send = nullptr, *d_recv = nullptr, *d_res = nullptr; uint32_t *d_flag = nullptr, *d_pos = nullptr; uint8_t *d_gsend = nullptr, *d_grecv = nullptr;
            TRY(f.alloc(d_send, SE));
            TRY(f.alloc(d_recv, SE));
            TRY(f.alloc(d_res, B));
            TRY(f.alloc(d_flag, (size_t)B + 1));
            TRY(f.alloc(d_pos, (size_t)B + 1));
            TRY(f.alloc(d_gsend, blk));
            TRY(f.alloc(d_grecv, (size_t)W * blk));
            TRY(f.zero(d_flag, (size_t)B + 1));
            lig_diag_linear* d_rec = reinterpret_cast<lig_diag_linear*>(d_gsend + 16);
            uint64_t bad_mine = 0, rep_mine = 0;
            // the heavy constraints by their numbers of the whole trace, ascending: the uploaded list's own, or need[] of the compact ones
            const std::vector<uint32_t>* heavy_c = &d.heavy;
            if (att) {
                TRY(f.alloc(d_bound, (size_t)n_slices + 1));
                TRY(f.launch(lig::k_diag_att_bounds, n_slices + 1, att->need, d.NC, SE, (uint32_t)n_slices, (uint64_t)NC, d_bound));
                if (!d.heavy.empty()) {
                    const uint32_t NH = (uint32_t)d.heavy.size();
                    uint32_t* d_hg = nullptr;
                    TRY(f.alloc(d_hg, NH));
                    heavy_global.resize(NH);
                    TRY(f.launch(lig::k_diag_att_heavy_global, NH, d.heavy_dev, NH, att->need, d_hg));
                    TRY(f.fetch(heavy_global.data(), d_hg, NH));
                    if (!std::is_sorted(heavy_global.begin(), heavy_global.end())) FAIL(c, LIG_E_STATE, std::string(who) + ": the attached share's need list is not ascending");
                }
                heavy_c = &heavy_global;
            }
            TRY(f.mark(PH_RECORDS));      // (uploads, table conversion; regrouping)
            for (uint64_t j = 0; j < n_slices; j++) {
                const uint32_t c0 = (uint32_t)(j * SE), n = (uint32_t)std::min<uint64_t>(SE, NC - c0);
                const size_t h0 = std::lower_bound(heavy_c->begin(), heavy_c->end(), c0) - heavy_c->begin();
                const uint32_t nh = (uint32_t)(std::lower_bound(heavy_c->begin(), heavy_c->end(), c0 + n) - heavy_c->begin() - h0);
                if (sys) {
                    if (n < SE) TRY(f.zero(d_send + n, SE - n));       // beyond the end of the system: zero partials
                    TRY(f.launch(lig::k_diag_lin_part, n, d.tb, d.terms, c0, n, v.msgs, l, k, l_recip, d.coef, d_local, d_send));
                    if (nh) TRY(f.launch_blocks(lig::k_diag_lin_part_heavy, nh, d.heavy_dev + h0, nh, d.tb, d.terms, c0, v.msgs, l, k, l_recip, d.coef, d_local, d_send));
                } else {
                    TRY(f.zero(d_send, SE));      // the constraints this rank does not need, and those beyond the end
                    TRY(f.launch(lig::k_diag_att_part, std::min<uint64_t>(n, d.NC), d_bound + j, d.tb, d.terms, att->need, c0, n, v.msgs, l, k, l_recip, d.coef, d.rhs_index,
                                 d.rhs_coef, d_send));
                    if (nh) TRY(f.launch_blocks(lig::k_diag_att_part_heavy, nh, d.heavy_dev + h0, nh, d.tb, d.terms, att->need, c0, n, v.msgs, l, k, l_recip, d.coef, d.rhs_index,
                                                d.rhs_coef, d_send));
                }
                TRY(f.mark(PH_PARTIAL));
                TRY(f.all_to_all(d_send, d_recv, (size_t)B * 32, "all_to_all(partial constraint sums)"));
                TRY(f.mark(PH_EXCHANGE));
                const uint64_t first = (uint64_t)c0 + (uint64_t)v.rank * B;                             // my sub-block of this slice
                const uint32_t n_valid = first < NC ? (uint32_t)std::min<uint64_t>(B, NC - first) : 0u, first_c = (uint32_t)std::min<uint64_t>(first, NC);
                if (sys) TRY(f.launch(lig::k_diag_reduce<true>, B, d_recv, W, B, n_valid, first_c, d.rhs_index, d.rhs_coef, d.coef, d_res, d_flag));
                else TRY(f.launch(lig::k_diag_reduce<false>, B, d_recv, W, B, n_valid, first_c, nullptr, nullptr, nullptr, d_res, d_flag));
                TRY(f.mark(PH_REDUCE));
                uint32_t bad = 0;
                TRY(f.scan(d_flag, d_pos, B, &bad));
                if (bad > n_valid) FAIL(c, LIG_E_STATE, "lig_shard_rows_diagnose: counted more violated constraints than the sub-block holds");
                bad_mine += bad;
                const uint32_t rep = (uint32_t)std::min<uint64_t>(bad, rec_cap - rep_mine);
                if (rep) {
                    TRY(f.launch(lig::k_diag_scatter_lin, B, d_flag, d_pos, d_res, B, (uint32_t)first, rep, d_rec + rep_mine));
                    rep_mine += rep;
                }
                TRY(f.mark(PH_RECORDS));
            }
            header[0] = bad_mine; header[1] = rep_mine;
            HIP_TRY(c, hipMemcpyAsync(d_gsend, header, 16, hipMemcpyHostToDevice, s));
            TRY(f.all_gather(d_gsend, d_grecv, blk, "all_gather(violated constraints)"));
            gathered.resize((size_t)W * blk);
            TRY(f.fetch(gathered.data(), d_grecv, gathered.size()));
            // every rank: W ascending lists -> ascending constraint order, cut at lin_cap
            std::vector<lig_diag_linear> all;
            uint64_t bad_total = 0;
            for (uint32_t g = 0; g < W; g++) {
                uint64_t hd[2];
                std::memcpy(hd, gathered.data() + (size_t)g * blk, 16);
                if (hd[1] > rec_cap || hd[1] > hd[0] || hd[0] > n_slices * B) FAIL(c, LIG_E_STATE, "lig_shard_rows_diagnose: a rank's record block is malformed");
                bad_total += hd[0];
                const size_t at = all.size();
                all.resize(at + hd[1]);
                if (hd[1]) std::memcpy(all.data() + at, gathered.data() + (size_t)g * blk + 16, hd[1] * sizeof(lig_diag_linear));
            }
            std::stable_sort(all.begin(), all.end(), [](const lig_diag_linear& a, const lig_diag_linear& b) { return a.constraint < b.constraint; });
            const uint64_t rep = std::min<uint64_t>(all.size(), lin_cap);
            if (rep) std::memcpy(lin_out, all.data(), rep * sizeof(lig_diag_linear));
            info->n_linear_bad = bad_total;
            info->n_linear_reported = rep;
            TRY(f.mark(PH_RECORDS));
        }

        // ---------------------------------------------------------------- quadratic terms: every term is local to one rank
        if (v.n_terms_global) {
            const uint64_t NTl = v.triple_ord->size();
            const uint64_t rec_cap = std::min<uint64_t>(quad_cap, v.n_terms_global * l);
            const size_t blk = 16 + (size_t)rec_cap * (sizeof(lig_diag_quad) + 4);                     // [count, kept | records | ordinals]
            uint8_t *d_gsend = nullptr, *d_grecv = nullptr; uint32_t *d_grow = nullptr, *d_ord = nullptr;
            TRY(f.alloc(d_gsend, blk));
            TRY(f.alloc(d_grecv, (size_t)W * blk));
            lig_diag_quad* d_rec = reinterpret_cast<lig_diag_quad*>(d_gsend + 16);
            uint32_t* d_rec_ord = reinterpret_cast<uint32_t*>(d_gsend + 16 + (size_t)rec_cap * sizeof(lig_diag_quad));
            uint64_t bad_mine = 0, rep_mine = 0;
            if (NTl) {
                grow32.assign(v.grow->begin(), v.grow->end());
                ord32.assign(v.triple_ord->begin(), v.triple_ord->end());
                TRY(f.upload(d_grow, grow32.data(), grow32.size()));
                TRY(f.upload(d_ord, ord32.data(), ord32.size()));
                TRY(diag_quad_pass(f, v.msgs, v.tri_dev, NTl, rec_cap, nullptr, d_rec, d_grow, d_ord, d_rec_ord, &bad_mine, &rep_mine));
            }
            qheader[0] = bad_mine; qheader[1] = rep_mine;
            HIP_TRY(c, hipMemcpyAsync(d_gsend, qheader, 16, hipMemcpyHostToDevice, s));
            TRY(f.all_gather(d_gsend, d_grecv, blk, "all_gather(violated quadratic terms)"));
            gathered.resize((size_t)W * blk);
            TRY(f.fetch(gathered.data(), d_grecv, gathered.size()));
            struct Item { uint32_t ord; lig_diag_quad rec; };
            std::vector<Item> all;
            uint64_t bad_total = 0;
            for (uint32_t g = 0; g < W; g++) {
                const uint8_t* b = gathered.data() + (size_t)g * blk;
                uint64_t hd[2];
                std::memcpy(hd, b, 16);
                if (hd[1] > rec_cap || hd[1] > hd[0] || hd[0] > v.n_terms_global * l) FAIL(c, LIG_E_STATE, "lig_shard_rows_diagnose: a rank's record block is malformed");
                bad_total += hd[0];
                for (uint64_t i = 0; i < hd[1]; i++) {
                    Item it;
                    std::memcpy(&it.rec, b + 16 + i * sizeof(lig_diag_quad), sizeof(lig_diag_quad));
                    std::memcpy(&it.ord, b + 16 + (size_t)rec_cap * sizeof(lig_diag_quad) + i * 4, 4);
                    all.push_back(it);
                }
            }
            std::stable_sort(all.begin(), all.end(), [](const Item& a, const Item& b) { return a.ord != b.ord ? a.ord < b.ord : a.rec.column < b.rec.column; });
            const uint64_t rep = std::min<uint64_t>(all.size(), quad_cap);
            for (uint64_t i = 0; i < rep; i++) quad_out[i] = all[i].rec;
            info->n_quad_bad = bad_total;
            info->n_quad_reported = rep;
            TRY(f.mark(PH_QUAD));
        }
        return LIG_OK;
    });
}
}  // namespace
int lig_internal_shard_diagnose(lig_ctx* c, const lig_diag_shard& v, const lig_linear_system* sys, lig_diag_linear* lin_out, uint64_t lin_cap, lig_diag_quad* quad_out,
                                uint64_t quad_cap, lig_diag_info* info) {
    return shard_diagnose("lig_shard_rows_diagnose", c, v, sys, nullptr, lin_out, lin_cap, quad_out, quad_cap, info);
}
int lig_internal_shard_diagnose_attached(lig_ctx* c, const lig_diag_shard& v, const lig_linear* att, lig_diag_linear* lin_out, uint64_t lin_cap,
                                         lig_diag_quad* quad_out, uint64_t quad_cap, lig_diag_info* info) {
    const lig_linear_view view = lig_internal_linear_view(att);
    if (!view.sharded) FAIL(c, LIG_E_STATE, "lig_shard_rows_diagnose_attached: the attached structure is not a rank's share of a sharded trace");
    return shard_diagnose("lig_shard_rows_diagnose_attached", c, v, nullptr, &view, lin_out, lin_cap, quad_out, quad_cap, info);
}

namespace {
// What lig_shard_rows_explain and lig_shard_rows_read_slots share: the committed values of n_items slots, each held by one rank, on every
// rank.  d_slot: the slots on the device, `stride` 32-bit words apart (k_explain_part).  In pieces of P = explain_piece_size(n_items, slice)
// entries: part -> d_send (the ragged tail of the last piece zeroed, so that every piece is sent at the fixed size), ONE all-gather of
// P x 32 bytes per rank, sum -> the caller's buffer for the piece.  The schedule depends on n_items, W and the slice alone.
struct ExplainExchange {
    uint32_t* d_local = nullptr; fr *d_send = nullptr, *d_recv = nullptr;
    uint64_t P = 0;
};
enum { XPH_PART, XPH_EXCHANGE, XPH_SUM, XPH_RECORDS };
const std::initializer_list<const char*> XPH_NAMES = {"part", "exchange", "sum", "records"};
int explain_exchange_alloc(DiagShardFrame& f, std::vector<uint32_t>& local_of, uint64_t n_items, ExplainExchange& x) {
    x.P = lig::explain_piece_size(n_items, f.v.slice);
    TRY(diag_row_table(f, f.v, local_of, x.d_local));
    TRY(f.alloc(x.d_send, x.P));
    return f.alloc(x.d_recv, (size_t)f.v.world * x.P);
}
// piece j of the n_items entries: d_slot points at the first slot of the piece, the sums go to d_out[0 .. n)
int explain_exchange_piece(DiagShardFrame& f, const ExplainExchange& x, const uint32_t* d_slot, uint32_t stride, uint32_t n, fr* d_out, const char* what) {
    if (n < x.P) TRY(f.zero(x.d_send + n, x.P - n));
    TRY(f.launch(lig::k_explain_part, n, d_slot, stride, n, f.v.msgs, f.l, f.k, f.l_recip, x.d_local, x.d_send));
    TRY(f.mark(XPH_PART));
    TRY(f.all_gather(x.d_send, x.d_recv, (size_t)x.P * 32, what));
    TRY(f.mark(XPH_EXCHANGE));
    TRY(f.launch(lig::k_explain_sum, n, x.d_recv, f.v.world, (uint32_t)x.P, n, d_out));
    return f.mark(XPH_SUM);
}
}  // namespace

// One rank of a sharded rows job (lig_shard_rows_explain, lig_hip.h).  sys has passed lig_linear_check, asked explain_asked_ok, n_asked > 0.
// Collective: with m = the terms of the asked constraints (known on every host from sys->term_begin) and P = min(m, LIG_DIAG_SLICE) there are
// ceil(m / P) all-gathers of 32 P bytes per rank -- whatever this rank holds, whatever term_cap is (con_out needs every value).
// The items are formed and ordered on the host (explain_items_of, explain_order): no k_explain_gather, no copy back, and the system is not
// uploaded -- only the m ordered terms, first[], the asked list, one right-hand-side coefficient index per asked constraint and the table.
// Scratch: 32 P (send) + 32 W P (receive) + 32 m (values) + 8 m (terms) + 4 rows_global + 32 n_coefs + 12 n_asked + 4 (n_asked + 1), and
// the records: 88 n_asked + 84 min(m, term_cap).  Every send buffer is an allocation of its own; v.forget runs before any of them is freed.
int lig_internal_shard_explain(lig_ctx* c, const lig_diag_shard& v, const lig_linear_system* sys, const uint32_t* asked, uint64_t n_asked,
                               lig_explain_constraint* con_out, lig_explain_term* terms_out, uint64_t term_cap, lig_explain_info* info) {
    const uint32_t NA = (uint32_t)n_asked;
    // (sources of queued uploads: declared before the frame, whose scratch drains the stream when it goes)
    std::vector<lig::ExplainItem> items;
    std::vector<uint64_t> first;
    std::vector<uint32_t> rhs_index, rhs_coef, local_of;
    ExplainOrdered o;
    DiagShardFrame f(c, v, "lig_shard_rows_explain", "shard_explain", XPH_NAMES);
    uint32_t m = 0, rep = 0;

    TRY(f.run([&]() -> int {
        m = (uint32_t)lig::explain_items_of(*sys, asked, n_asked, items);       // <= n_terms < 2^32: the asked are distinct
        if (!lig::explain_order(items, NA, first)) FAIL(c, LIG_E_STATE, "lig_shard_rows_explain: a term names no asked constraint");
        rep = (uint32_t)std::min<uint64_t>(m, term_cap);
        // b_c of asked constraint a: rhs_coef[rhs_index[a] - 1], rhs_index[a] = a + 1 when it has one, else 0 (rhs_constraint is ascending)
        lig::explain_rhs_of(*sys, asked, n_asked, rhs_index, rhs_coef);
        uint32_t *d_asked = nullptr, *d_rhs_index = nullptr, *d_rhs_coef = nullptr; fr *d_coef = nullptr, *d_vals = nullptr;
        ExplainExchange x;
        if (m) TRY(explain_exchange_alloc(f, local_of, m, x));
        TRY(explain_upload(f, items, first, NA, rep, o));
        TRY(f.upload(d_asked, asked, NA));
        TRY(f.upload(d_rhs_index, rhs_index.data(), NA));
        TRY(f.upload(d_rhs_coef, rhs_coef.data(), NA));
        TRY(diag_upload_table(f, sys, d_coef));
        TRY(f.alloc(d_vals, m));
        TRY(f.mark(XPH_RECORDS));      // (uploads, table conversion)
        const uint64_t n_pieces = lig::explain_piece_count(m, x.P);
        for (uint64_t j = 0; j < n_pieces; j++) {
            const uint32_t n = (uint32_t)lig::explain_piece_len(m, x.P, j);
            TRY(explain_exchange_piece(f, x, &o.d_ordered[j * x.P].slot, 2, n, d_vals + j * x.P, "all_gather(witness values of the asked terms)"));
        }
        TRY(explain_records(f, o, d_asked, lig::ExplainFromValues{d_vals}, d_coef, d_rhs_index, d_rhs_coef, con_out, terms_out));
        return f.mark(XPH_RECORDS);
    }));
    info->n_terms_total = m;
    info->n_terms_reported = rep;
    return LIG_OK;
}

// One rank of a sharded rows job (lig_shard_rows_explain_attached, lig_hip.h).  att = the rank's share attached to the shard (sharded);
// asked has passed explain_asked_ok against the view's n_constraints (the global count), n_asked > 0.  alone: the one rank of its world
// without LIG_SHARD_FORCE_EXCHANGE -- the same passes, a device copy in place of every all-gather, no collective.
// Collective: ONE header all-gather of 4 explain_header_words(n_asked) bytes per rank (m_r, and who holds which b_c), then -- with
// M = max m_r, known on every rank from the headers -- explain_piece_count(M, P) all-gathers of 48 P bytes per rank,
// P = explain_piece_size(M, LIG_DIAG_SLICE).  The number of record all-gathers depends on what the ranks hold, but only through numbers every
// rank has received: every rank issues the same schedule.
// Scratch: 8 (n_terms + 1) marks and positions over the local terms, 48 m_r collected records, (W + 1) header blocks, 48 P (send) +
// 48 W P (receive), 16 W P per piece for the heads, 32 sum m_r unordered values + 4 sum m_r permutation, 44 sum m_r ordered terms, asked
// positions and values, 4 per local row, 8 W, 16 n_asked, and the records: 88 n_asked + 84 min(sum m_r, term_cap).  Every send buffer is an
// allocation of its own; v.forget runs before any of them is freed.
int lig_internal_shard_explain_attached(lig_ctx* c, const lig_diag_shard& v, const lig_linear* att, bool alone, const uint32_t* asked, uint64_t n_asked,
                                        lig_explain_constraint* con_out, lig_explain_term* terms_out, uint64_t term_cap, lig_explain_info* info) {
    const lig_linear_view a = lig_internal_linear_view(att);
    const uint32_t NA = (uint32_t)n_asked, W = v.world, l = c->l, k = c->k, NT = (uint32_t)a.n_terms, NR = (uint32_t)a.n_rhs;
    const uint64_t rows_local = v.grow->size();
    // what the kernels index with: the local slots tile the rank's rows, a slot of the whole trace fits 32 bits
    if (!a.sharded || a.rows_local != rows_local || (uint64_t)a.n_slots != rows_local * l || v.rows_global * (uint64_t)l > (1ull << 32) || a.n_terms >= (1ull << 32) ||
        (NT && !rows_local) || v.rank >= W || (alone && W != 1))
        FAIL(c, LIG_E_STATE, "lig_shard_rows_explain_attached: the attached structure is not this rank's share of the sharded trace");
    for (size_t lr = 0; lr < rows_local; lr++)
        if ((*v.grow)[lr] >= v.rows_global) FAIL(c, LIG_E_STATE, "lig_shard_rows_explain_attached: a local row lies outside the trace");
    // (sources and targets of queued copies: declared before the frame, whose scratch drains the stream when it goes)
    std::vector<uint32_t> grow32(v.grow->begin(), v.grow->end()), hdr_all, heads, m32, off32, rhs_index, rhs_coef, holder, perm;
    std::vector<uint64_t> m_of, first;
    std::vector<lig::ExplainItem> items;
    ExplainOrdered o;
    enum { APH_SELECT, APH_EXCHANGE, APH_MERGE, APH_RECORDS };
    DiagShardFrame f(c, v, "lig_shard_rows_explain_attached", "shard_explain_attached", {"select", "exchange", "merge", "records"}, alone);
    hipStream_t s = f.s;
    uint32_t total = 0, rep = 0;

    TRY(f.run([&]() -> int {
        // 1. select: mark, scan, the right-hand sides this rank holds, the header block
        const size_t hw = (size_t)lig::explain_header_words(NA);
        uint32_t *d_asked = nullptr, *d_mark = nullptr, *d_pos = nullptr, *d_grow = nullptr, *d_hdr = nullptr, *d_hdr_all = nullptr;
        TRY(f.upload(d_asked, asked, NA));
        TRY(f.upload(d_grow, grow32.data(), rows_local));
        TRY(f.alloc(d_mark, (size_t)NT + 1));
        TRY(f.alloc(d_pos, (size_t)NT + 1));
        TRY(f.alloc(d_hdr, hw));
        TRY(f.alloc(d_hdr_all, (size_t)W * hw));
        TRY(f.zero(d_mark + NT, 1));
        TRY(f.zero(d_hdr, hw));
        if (NT) TRY(f.launch(lig::k_explain_mark, NT, a.ent, NT, a.need, d_asked, NA, d_mark));
        if (NR) TRY(f.launch(lig::k_explain_rhs_held, NR, a.rhs_c, a.rhs_coef, NR, a.need, d_asked, NA, reinterpret_cast<uint2*>(d_hdr + lig::explain_header_held(0))));
        uint32_t m_own = 0;
        TRY(f.scan(rocprim::make_transform_iterator((const uint32_t*)d_mark, lig::ExplainMarked{}), d_pos, NT, &m_own));
        if (m_own > NT) FAIL(c, LIG_E_STATE, "lig_shard_rows_explain_attached: counted more asked terms than the rank's share holds");
        HIP_TRY(c, hipMemcpyAsync(d_hdr, d_pos + NT, 4, hipMemcpyDeviceToDevice, s));
        lig::ExplainRecord* d_rec = nullptr;
        TRY(f.alloc(d_rec, m_own));
        if (m_own) TRY(f.launch(lig::k_explain_collect_values, NT, a.ent, NT, a.begin, a.n_slots, d_mark, d_pos, d_grow, v.msgs, l, k, f.l_recip, d_rec));
        TRY(f.mark(APH_SELECT));
        // 2. the headers: every m_r, the holder of every b_c
        TRY(f.all_gather(d_hdr, d_hdr_all, hw * 4, "all_gather(counts and right-hand sides of the asked constraints)"));
        hdr_all.resize((size_t)W * hw);
        TRY(f.fetch(hdr_all.data(), d_hdr_all, (size_t)W * hw));
        if (!lig::explain_header_merge(hdr_all.data(), W, NA, m_of, rhs_index, rhs_coef, holder) || m_of[v.rank] != m_own)
            FAIL(c, LIG_E_STATE, "lig_shard_rows_explain_attached: a rank's header block is malformed");
        const lig::ExplainRecordSchedule x = lig::explain_record_schedule(m_of, v.slice);
        if ((uint64_t)W * x.P >= (1ull << 32)) FAIL(c, LIG_E_STATE, "lig_shard_rows_explain_attached: a piece of the record exchange exceeds 2^32 records");
        total = (uint32_t)x.off[W];
        rep = (uint32_t)std::min<uint64_t>(total, term_cap);
        TRY(f.mark(APH_EXCHANGE));
        // 3. the records, in pieces of P per rank; the values stay on the device, the heads go to the host
        const size_t WP = (size_t)W * x.P;
        lig::ExplainRecord *d_send = nullptr, *d_recv = nullptr; uint4* d_heads = nullptr; fr *d_vals_in = nullptr, *d_vals = nullptr; uint32_t *d_m = nullptr, *d_off = nullptr;
        TRY(f.alloc(d_send, x.P));
        TRY(f.alloc(d_recv, WP));
        TRY(f.alloc(d_heads, (size_t)x.pieces * WP));
        TRY(f.alloc(d_vals_in, total));
        TRY(f.alloc(d_vals, total));
        m32.assign(m_of.begin(), m_of.end());
        off32.assign(x.off.begin(), x.off.begin() + W);
        TRY(f.upload(d_m, m32.data(), W));
        TRY(f.upload(d_off, off32.data(), W));
        for (uint64_t j = 0; j < x.pieces; j++) {
            const uint64_t lo = std::min<uint64_t>(j * x.P, m_own), n = std::min<uint64_t>(x.P, m_own - lo);      // this rank's records of the piece
            if (n) HIP_TRY(c, hipMemcpyAsync(d_send, d_rec + lo, (size_t)n * sizeof(lig::ExplainRecord), hipMemcpyDeviceToDevice, s));
            if (n < x.P) TRY(f.zero(d_send + n, x.P - n));
            TRY(f.mark(APH_SELECT));
            TRY(f.all_gather(d_send, d_recv, (size_t)x.P * sizeof(lig::ExplainRecord), "all_gather(the asked terms of every rank)"));
            TRY(f.mark(APH_EXCHANGE));
            TRY(f.launch(lig::k_explain_keep, WP, d_recv, W, (uint32_t)x.P, j, d_m, d_off, d_heads + j * WP, d_vals_in));
            TRY(f.mark(APH_MERGE));
        }
        // 4. merge and order on the host, permute the values, the records
        heads.resize((size_t)x.pieces * WP * 4);
        TRY(f.fetch(heads.data(), d_heads, (size_t)x.pieces * WP));
        if (!lig::explain_records_walk(heads.data(), W, x, m_of, NA, items)) FAIL(c, LIG_E_STATE, "lig_shard_rows_explain_attached: a rank's record block is malformed");
        if (!lig::explain_merge(items, NA, first, perm)) FAIL(c, LIG_E_STATE, "lig_shard_rows_explain_attached: a term names no asked constraint");
        uint32_t *d_perm = nullptr, *d_rhs_index = nullptr, *d_rhs_coef = nullptr;
        TRY(explain_upload(f, items, first, NA, rep, o));
        TRY(f.upload(d_perm, perm.data(), total));
        TRY(f.upload(d_rhs_index, rhs_index.data(), NA));
        TRY(f.upload(d_rhs_coef, rhs_coef.data(), NA));
        if (total) TRY(f.launch(lig::k_explain_permute, total, d_vals_in, d_perm, total, d_vals));
        TRY(f.mark(APH_MERGE));
        // values set on the side stream (lig_shard_rows_set_linear_values): the table is read in place once its conversion has finished
        if (a.coef_ready) HIP_TRY(c, hipStreamWaitEvent(s, a.coef_ready, 0));
        TRY(explain_records(f, o, d_asked, lig::ExplainFromValues{d_vals}, a.coef, d_rhs_index, d_rhs_coef, con_out, terms_out));
        return f.mark(APH_RECORDS);
    }));
    info->n_terms_total = total;
    info->n_terms_reported = rep;
    return LIG_OK;
}

// lig_shard_rows_read_slots: the same part / all-gather / sum over the slot list (it has passed explain_slots_ok against the rows of the WHOLE
// trace, n_slots > 0) in pieces of P = min(n_slots, LIG_DIAG_SLICE); the summed piece is copied to `values`.  ceil(n_slots / P) all-gathers.
// Scratch: 4 P (slots) + 32 P (send) + 32 W P (receive) + 32 P (sums) + 4 rows_global.
int lig_internal_shard_read_slots(lig_ctx* c, const lig_diag_shard& v, const uint32_t* slots, uint64_t n_slots, uint8_t* values) {
    std::vector<uint32_t> local_of;      // (source of a queued upload: declared before the frame)
    DiagShardFrame f(c, v, "lig_shard_rows_read_slots", "shard_read_slots", XPH_NAMES);
    return f.run([&]() -> int {
        ExplainExchange x;
        uint32_t* d_slots = nullptr; fr* d_val = nullptr;
        TRY(explain_exchange_alloc(f, local_of, n_slots, x));
        TRY(f.alloc(d_slots, x.P));
        TRY(f.alloc(d_val, x.P));
        const uint64_t n_pieces = lig::explain_piece_count(n_slots, x.P);
        for (uint64_t j = 0; j < n_pieces; j++) {
            const uint32_t n = (uint32_t)lig::explain_piece_len(n_slots, x.P, j);
            HIP_TRY(c, hipMemcpyAsync(d_slots, slots + j * x.P, (size_t)n * 4, hipMemcpyHostToDevice, f.s));
            TRY(explain_exchange_piece(f, x, d_slots, 1, n, d_val, "all_gather(witness values of the slots)"));
            TRY(f.fetch(values + j * x.P * 32, d_val, n));
            TRY(f.mark(XPH_RECORDS));
        }
        return LIG_OK;
    });
}

// One rank of a sharded rows job (lig_shard_rows_explain_slots*, lig_hip.h).  att = the rank's share attached to the shard, or the temporary
// share the entry made from the caller's term list (sharded either way); kinds: one per committed row of the WHOLE trace; slots has passed
// explain_slots_ok against the rows of the whole trace and is strictly ascending, n_asked > 0.  alone: as lig_internal_shard_explain_attached.
// Collective: ONE header all-gather of 4 slot_header_words(n_asked) bytes per rank (m_r, and per asked slot {held, n_terms, value}), then --
// with M = max m_r, known on every rank from the headers -- explain_piece_count(M, P) all-gathers of 16 P bytes per rank,
// P = explain_piece_size(M, LIG_DIAG_SLICE); then, when any slot has a term, lig_internal_shard_explain_attached itself over the distinct
// constraints with term_cap = 0 (one evaluator; the list is the same on every rank, hence its schedule).  The fetch of the last piece has
// drained the stream before that call: no collective of this frame is in flight while the inner frame issues its own, and the inner frame's
// v.forget runs while this frame's send buffers are still allocated -- this frame's own runs again before they are freed.
// Scratch on top of the inner call: 12 n_here + 32 n_here + 8 (n_here + 1) for the held slots (local numbers, indices, values, lengths and
// prefix sums), 4 n_asked, (W + 1) header blocks, 16 m_r collected items, 16 P (send) + 16 W P (receive) + 16 J W P for the host's walk
// (J = ceil(M / P)), and the records: 88 distinct + 96 min(sum m_r, term_cap).
int lig_internal_shard_explain_slots(lig_ctx* c, const lig_diag_shard& v, const lig_linear* att, bool alone, const uint8_t* kinds, const uint32_t* slots, uint64_t n_asked,
                                     lig_slot_record* slot_out, lig_slot_term* terms_out, uint64_t term_cap, lig_slot_info* info) {
    static const char* const who = "lig_shard_rows_explain_slots";
    const lig_linear_view a = lig_internal_linear_view(att);
    const uint32_t NA = (uint32_t)n_asked, W = v.world, l = c->l, k = c->k, NT = (uint32_t)a.n_terms;
    const uint64_t rows_local = v.grow->size();
    // what the kernels index with: the local slots tile the rank's rows, a slot of the whole trace fits 32 bits
    if (!a.sharded || a.rows_local != rows_local || (uint64_t)a.n_slots != rows_local * l || v.rows_global * (uint64_t)l > (1ull << 32) || a.n_terms >= (1ull << 32) ||
        (NT && !rows_local) || v.rank >= W || (alone && W != 1))
        FAIL(c, LIG_E_STATE, std::string(who) + ": the linear structure is not this rank's share of the sharded trace");
    // (sources and targets of queued copies: declared before the frame, whose scratch drains the stream when it goes)
    std::vector<uint32_t> local_of(v.rows_global, lig::LIN_NOT_LOCAL), mine, lslots, pre, heavy, hdr_all, holder, n_terms, values, distinct, cidx;
    for (size_t lr = 0; lr < rows_local; lr++) {
        if ((*v.grow)[lr] >= v.rows_global) FAIL(c, LIG_E_STATE, std::string(who) + ": a local row lies outside the trace");
        local_of[(*v.grow)[lr]] = (uint32_t)lr;
    }
    lig::slot_asked_here(slots, n_asked, l, local_of, lig::LIN_NOT_LOCAL, mine, lslots);
    const uint32_t NM = (uint32_t)mine.size();
    std::vector<uint64_t> m_of, first;
    std::vector<lig::SlotItem> recv_all;
    std::vector<lig::ExplainItem> items;
    std::vector<lig_explain_constraint> con;
    enum { SPH_SELECT, SPH_EXCHANGE, SPH_MERGE, SPH_RESIDUALS, SPH_RECORDS };
    DiagShardFrame f(c, v, who, "shard_explain_slots", {"select", "exchange", "merge", "residuals", "records"}, alone);
    hipStream_t s = f.s;
    uint32_t total = 0, rep = 0, ND = 0;

    TRY(f.run([&]() -> int {
        // 1. the asked slots this rank holds: segment lengths, prefix sums, values, the header block, the items
        const size_t hw = (size_t)lig::slot_header_words(NA);
        uint32_t *d_slots = nullptr, *d_lslots = nullptr, *d_mine = nullptr, *d_len = nullptr, *d_pre = nullptr, *d_hdr = nullptr, *d_hdr_all = nullptr; fr* d_val = nullptr;
        TRY(f.upload(d_slots, slots, NA));
        TRY(f.upload(d_lslots, lslots.data(), NM));
        TRY(f.upload(d_mine, mine.data(), NM));
        TRY(f.alloc(d_len, (size_t)NM + 1));
        TRY(f.alloc(d_pre, (size_t)NM + 1));
        TRY(f.alloc(d_val, NM));
        TRY(f.alloc(d_hdr, hw));
        TRY(f.alloc(d_hdr_all, (size_t)W * hw));
        TRY(f.zero(d_hdr, hw));
        TRY(f.zero(d_len + NM, 1));
        if (NM) {
            TRY(f.launch(lig::k_slot_len, NM, d_lslots, NM, a.begin, d_len));
            TRY(f.launch(lig::k_read_slots, NM, d_lslots, NM, v.msgs, l, k, f.l_recip, d_val));
        }
        TRY(f.scan_enqueue(d_len, d_pre, NM));
        HIP_TRY(c, hipMemcpyAsync(d_hdr, d_pre + NM, 4, hipMemcpyDeviceToDevice, s));
        if (NM) TRY(f.launch(lig::k_slot_header, NM, d_mine, d_len, d_val, NM, d_hdr));
        pre.resize((size_t)NM + 1);
        TRY(f.fetch(pre.data(), d_pre, (size_t)NM + 1));
        const uint32_t m_own = pre[NM];
        // distinct slots own disjoint segments: the lengths add up to at most the terms kept, every prefix sum is exact in 32 bits
        if (m_own > NT || !std::is_sorted(pre.begin(), pre.end())) FAIL(c, LIG_E_STATE, std::string(who) + ": the share's index does not add up to its term count");
        for (uint32_t i = 0; i < NM; i++) if (pre[i + 1] - pre[i] > lig::HEAVY_MIN) heavy.push_back(i);
        lig::SlotItem* d_items = nullptr;
        TRY(f.alloc(d_items, m_own));
        if (m_own) TRY(f.launch(lig::k_slot_collect_shard, m_own, d_lslots, d_mine, NM, d_pre, m_own, a.begin, a.ent, a.need, d_items));
        if (!heavy.empty()) {
            uint32_t* d_heavy = nullptr;
            TRY(f.upload(d_heavy, heavy.data(), heavy.size()));
            TRY(f.launch_blocks(lig::k_slot_collect_shard_heavy, (uint32_t)heavy.size(), d_heavy, (uint32_t)heavy.size(), d_lslots, d_mine, d_pre, a.begin, a.ent, a.need, d_items));
        }
        TRY(f.mark(SPH_SELECT));
        // 2. the headers: every m_r, the holder of every slot with its count and value
        TRY(f.all_gather(d_hdr, d_hdr_all, hw * 4, "all_gather(counts and values of the asked slots)"));
        hdr_all.resize((size_t)W * hw);
        TRY(f.fetch(hdr_all.data(), d_hdr_all, (size_t)W * hw));
        if (!lig::slot_header_merge(hdr_all.data(), W, NA, m_of, holder, n_terms, values) || m_of[v.rank] != m_own)
            FAIL(c, LIG_E_STATE, std::string(who) + ": a rank's header block is malformed");
        const lig::ExplainRecordSchedule x = lig::explain_record_schedule(m_of, v.slice);
        if ((uint64_t)W * x.P >= (1ull << 32)) FAIL(c, LIG_E_STATE, std::string(who) + ": a piece of the item exchange exceeds 2^32 items");
        total = (uint32_t)x.off[W];
        rep = (uint32_t)std::min<uint64_t>(total, term_cap);
        TRY(f.mark(SPH_EXCHANGE));
        // 3. the items, in pieces of P per rank
        const size_t WP = (size_t)W * x.P;
        lig::SlotItem *d_send = nullptr, *d_recv = nullptr, *d_all = nullptr;
        TRY(f.alloc(d_send, x.P));
        TRY(f.alloc(d_recv, WP));
        TRY(f.alloc(d_all, (size_t)x.pieces * WP));
        for (uint64_t j = 0; j < x.pieces; j++) {
            const uint64_t lo = std::min<uint64_t>(j * x.P, m_own), n = std::min<uint64_t>(x.P, m_own - lo);      // this rank's items of the piece
            if (n) HIP_TRY(c, hipMemcpyAsync(d_send, d_items + lo, (size_t)n * sizeof(lig::SlotItem), hipMemcpyDeviceToDevice, s));
            if (n < x.P) TRY(f.zero(d_send + n, x.P - n));
            TRY(f.mark(SPH_SELECT));
            TRY(f.all_gather(d_send, d_recv, (size_t)x.P * sizeof(lig::SlotItem), "all_gather(the terms through the asked slots of every rank)"));
            HIP_TRY(c, hipMemcpyAsync(d_all + j * WP, d_recv, WP * sizeof(lig::SlotItem), hipMemcpyDeviceToDevice, s));
            TRY(f.mark(SPH_EXCHANGE));
        }
        // 4. walk, order, the distinct constraints -- on the host of every rank.  The fetch drains the stream: every collective above is complete.
        recv_all.resize((size_t)x.pieces * WP);
        TRY(f.fetch(recv_all.data(), d_all, recv_all.size()));
        if (!lig::slot_items_walk(recv_all.data(), W, x, m_of, NA, holder, n_terms, items)) FAIL(c, LIG_E_STATE, std::string(who) + ": a rank's item block is malformed");
        if (!lig::explain_order(items, NA, first)) FAIL(c, LIG_E_STATE, std::string(who) + ": a collected term names no asked slot");
        distinct.resize(total);
        for (uint32_t i = 0; i < total; i++) {
            if (items[i].slot >= a.n_constraints) FAIL(c, LIG_E_STATE, std::string(who) + ": an item names no constraint of the system");
            distinct[i] = items[i].slot;
        }
        std::sort(distinct.begin(), distinct.end());
        distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
        ND = (uint32_t)distinct.size();
        con.resize(ND);
        TRY(f.mark(SPH_MERGE));
        // 5. their sizes and residuals: the attached selection pass of the shard itself, asked for the constraint records alone
        if (ND) {
            lig_explain_info einfo;
            std::memset(&einfo, 0, sizeof einfo);
            einfo.struct_bytes = sizeof einfo;
            TRY(lig_internal_shard_explain_attached(c, v, att, alone, distinct.data(), ND, con.data(), nullptr, 0, &einfo));
        }
        TRY(f.mark(SPH_RESIDUALS));
        // 6. the records, with the table in force
        if (rep) {
            cidx.resize(rep);
            for (uint32_t i = 0; i < rep; i++) cidx[i] = (uint32_t)(std::lower_bound(distinct.begin(), distinct.end(), items[i].slot) - distinct.begin());
            lig::ExplainItem* d_ordered = nullptr; uint32_t* d_cidx = nullptr; lig_explain_constraint* d_con = nullptr; lig_slot_term* d_out = nullptr;
            TRY(f.upload(d_ordered, items.data(), rep));
            TRY(f.upload(d_cidx, cidx.data(), rep));
            TRY(f.upload(d_con, con.data(), ND));
            TRY(f.alloc(d_out, rep));
            // values set on the side stream (lig_shard_rows_set_linear_values): the table is read in place once its conversion has finished
            if (a.coef_ready) HIP_TRY(c, hipStreamWaitEvent(s, a.coef_ready, 0));
            TRY(f.launch(lig::k_slot_fill, rep, d_ordered, d_cidx, rep, d_slots, d_con, a.coef, d_out));
            TRY(f.fetch(terms_out, d_out, rep));
        }
        return f.mark(SPH_RECORDS);
    }));
    for (uint32_t i = 0; i < NA; i++) {
        lig_slot_record& r = slot_out[i];
        std::memset(&r, 0, sizeof r);
        r.slot = slots[i]; r.row_kind = kinds[slots[i] / l] & 0x7fu;
        r.n_terms = n_terms[i]; r.first_term = first[i];
        std::memcpy(r.value, values.data() + 8 * (size_t)i, 32);
    }
    info->n_terms_total = total;
    info->n_terms_reported = rep;
    info->n_constraints_distinct = ND;
    return LIG_OK;
}

// One rank of a sharded rows job (lig_shard_rows_untouched_slots*, lig_hip.h); att, kinds and alone as above.  The rank runs the one-GPU pass
// over its LOCAL LINEAR .. QZ rows against its local begin[] in slices of DIAG_UNTOUCHED_ITEMS, writes the slots of the WHOLE trace and keeps
// its first min(cap, selected) records on the device.  Collective: ONE all-gather of the 32-byte header {n_untouched, n_untouched_nonzero,
// kept, 0}, then -- with M = max kept -- explain_piece_count(M, P) all-gathers of 40 P bytes per rank.  The host merges the W ascending
// lists and cuts at cap (untouched_merge): the first cap of all are among each rank's first cap.
// Scratch: 16 bytes per local LINEAR .. QZ row, 16 per slot of a slice, 40 kept, 32 (W + 1), 40 P (send) + 40 W P (receive) + 40 J W P.
int lig_internal_shard_untouched_slots(lig_ctx* c, const lig_diag_shard& v, const lig_linear* att, bool alone, const uint8_t* kinds, int nonzero_only, lig_slot_value* out,
                                       uint64_t cap, lig_untouched_info* info) {
    static const char* const who = "lig_shard_rows_untouched_slots";
    const lig_linear_view a = lig_internal_linear_view(att);
    const uint32_t W = v.world, l = c->l, k = c->k;
    const uint64_t rows_local = v.grow->size();
    if (!a.sharded || a.rows_local != rows_local || (uint64_t)a.n_slots != rows_local * l || v.rows_global * (uint64_t)l > (1ull << 32) || v.rank >= W || (alone && W != 1))
        FAIL(c, LIG_E_STATE, std::string(who) + ": the linear structure is not this rank's share of the sharded trace");
    // (sources and targets of queued copies: declared before the frame, whose scratch drains the stream when it goes)
    std::vector<uint4> lrows;
    for (size_t lr = 0; lr < rows_local; lr++) {
        const size_t g = (*v.grow)[lr];
        if (g >= v.rows_global) FAIL(c, LIG_E_STATE, std::string(who) + ": a local row lies outside the trace");
        if ((kinds[g] & 0x7fu) <= LIG_ROW_QZ) lrows.push_back(make_uint4((uint32_t)lr, kinds[g] & 0x7fu, (uint32_t)g, 0u));
    }
    const uint64_t NL = lrows.size();
    uint64_t header[lig::UNTOUCHED_HEADER_WORDS] = {0, 0, 0, 0}, n_untouched = 0, n_nonzero = 0;
    std::vector<uint64_t> hdr_all, kept;
    std::vector<lig_slot_value> recv_all, merged;
    enum { UPH_LOCAL, UPH_EXCHANGE, UPH_MERGE };
    DiagShardFrame f(c, v, who, "shard_untouched_slots", {"local", "exchange", "merge"}, alone);
    hipStream_t s = f.s;

    TRY(f.run([&]() -> int {
        // 1. the rank's own rows
        const uint64_t per = std::max<uint64_t>(lig::DIAG_UNTOUCHED_ITEMS / l, 1);      // rows per slice: per * l < 2^32 (rows_global * l <= 2^32)
        const uint64_t slice_items = std::min(per, NL) * l, keep_cap = std::min<uint64_t>(cap, NL * l);
        uint4* d_lrows = nullptr; uint64_t *d_flag = nullptr, *d_pos = nullptr, *d_hdr = nullptr, *d_hdr_all = nullptr; lig_slot_value* d_keep = nullptr;
        TRY(f.upload(d_lrows, lrows.data(), NL));
        TRY(f.alloc(d_flag, (size_t)slice_items + 1));
        TRY(f.alloc(d_pos, (size_t)slice_items + 1));
        TRY(f.alloc(d_keep, keep_cap));
        TRY(f.alloc(d_hdr_all, (size_t)W * lig::UNTOUCHED_HEADER_WORDS));
        uint64_t un_mine = 0, nz_mine = 0, kept_mine = 0;
        for (uint64_t r0 = 0; r0 < NL; r0 += per) {      // (the first slice is the largest: its scan sizes the temp for all of them)
            const uint32_t items = (uint32_t)(std::min(per, NL - r0) * l);
            TRY(f.zero(d_flag + items, 1));
            TRY(f.launch(lig::k_untouched_flag<uint4>, items, d_lrows, (uint32_t)r0, items, a.begin, v.msgs, l, k, f.l_recip, d_flag));
            uint64_t both = 0;      // the two counts of the slice, packed
            TRY(f.scan(d_flag, d_pos, items, &both));
            const uint32_t un = (uint32_t)both, nz = (uint32_t)(both >> 32);
            if (un > items || nz > un) FAIL(c, LIG_E_STATE, std::string(who) + ": counted more slots than the slice holds");
            un_mine += un; nz_mine += nz;
            const uint32_t rep = (uint32_t)std::min<uint64_t>(nonzero_only ? nz : un, keep_cap - kept_mine);
            if (rep) {
                TRY(f.launch(lig::k_untouched_compact<uint4>, items, d_flag, d_pos, d_lrows, (uint32_t)r0, items, v.msgs, l, k, f.l_recip, nonzero_only ? 1u : 0u, rep,
                             d_keep + kept_mine));
                kept_mine += rep;
            }
        }
        header[0] = un_mine; header[1] = nz_mine; header[2] = kept_mine;
        TRY(f.upload(d_hdr, header, lig::UNTOUCHED_HEADER_WORDS));
        TRY(f.mark(UPH_LOCAL));
        // 2. the counts of every rank
        TRY(f.all_gather(d_hdr, d_hdr_all, sizeof header, "all_gather(counts of the untouched slots)"));
        hdr_all.resize((size_t)W * lig::UNTOUCHED_HEADER_WORDS);
        TRY(f.fetch(hdr_all.data(), d_hdr_all, hdr_all.size()));
        if (!lig::untouched_header_merge(hdr_all.data(), W, nonzero_only != 0, cap, n_untouched, n_nonzero, kept) || kept[v.rank] != kept_mine)
            FAIL(c, LIG_E_STATE, std::string(who) + ": a rank's header block is malformed");
        // 3. the kept records, in pieces of P per rank
        const lig::ExplainRecordSchedule x = lig::explain_record_schedule(kept, v.slice);
        if ((uint64_t)W * x.P >= (1ull << 32)) FAIL(c, LIG_E_STATE, std::string(who) + ": a piece of the record exchange exceeds 2^32 records");
        const size_t WP = (size_t)W * x.P;
        lig_slot_value *d_send = nullptr, *d_recv = nullptr, *d_all = nullptr;
        TRY(f.alloc(d_send, x.P));
        TRY(f.alloc(d_recv, WP));
        TRY(f.alloc(d_all, (size_t)x.pieces * WP));
        for (uint64_t j = 0; j < x.pieces; j++) {
            const uint64_t lo = std::min<uint64_t>(j * x.P, kept_mine), n = std::min<uint64_t>(x.P, kept_mine - lo);
            if (n) HIP_TRY(c, hipMemcpyAsync(d_send, d_keep + lo, (size_t)n * sizeof(lig_slot_value), hipMemcpyDeviceToDevice, s));
            if (n < x.P) TRY(f.zero(d_send + n, x.P - n));
            TRY(f.all_gather(d_send, d_recv, (size_t)x.P * sizeof(lig_slot_value), "all_gather(the untouched slots of every rank)"));
            HIP_TRY(c, hipMemcpyAsync(d_all + j * WP, d_recv, WP * sizeof(lig_slot_value), hipMemcpyDeviceToDevice, s));
        }
        recv_all.resize((size_t)x.pieces * WP);
        TRY(f.fetch(recv_all.data(), d_all, recv_all.size()));
        TRY(f.mark(UPH_EXCHANGE));
        // 4. W ascending lists -> the first cap of all
        if (!lig::untouched_merge(recv_all.data(), W, x, kept, cap, merged)) FAIL(c, LIG_E_STATE, std::string(who) + ": a rank's record block is malformed");
        return f.mark(UPH_MERGE);
    }));
    if (!merged.empty()) std::memcpy(out, merged.data(), merged.size() * sizeof(lig_slot_value));
    info->n_untouched = n_untouched;
    info->n_untouched_nonzero = n_nonzero;
    info->n_reported = merged.size();
    return LIG_OK;
}
