// linear.hip -- sparse linear constraints: the linear-test randomness rows formed on the device (lig_linear_*, lig_rows_set_linear).
//
// The reference draws ONE element r_c per linear constraint c from the linear random engine and adds a * r_c to the randomness of
// every witness the constraint touches, b_c * r_c to the public constant (witness_manager.hpp:344-388).  For constraints
// sum_j a_cj * w[slot_cj] = b_c that is
//     Rn[slot s] = sum over terms (c, s, a) of a * r_c            const_sum = - sum_c b_c * r_c
// The structure (which constraint touches which slot with which coefficient) does not depend on the stage-1 seed, so the work is
// split in two:
//   prepare (once per lig_rows_set_linear, off the proving path): the term list, given constraint by constraint, is regrouped BY
//     SLOT -- a per-slot count (32-bit atomics: they only decide where a term lands inside its slot's segment, and the sum over a
//     segment is exact, so the result does not depend on them), an exclusive scan (rocPRIM), a scatter of (constraint, coefficient)
//     pairs.  Rows no term touches and slots with very many terms are found here.
//   form (per proof, on the side stream under the encodes): r = n_constraints elements of the AES-256-CTR field stream keyed by the
//     stage-1 seed (aes.hip), then ONE pass in slot order in which every slot has exactly one owner:
//       k_lin_form         one lane per slot of a touched row: gathers r_c (32 bytes, random), adds / subtracts it, or multiplies it
//                          by a table coefficient first (the table is kept in Montgomery form: one product per such term, none for
//                          +1 / -1); writes the canonical sum, zeros for slots without terms and for the pad slots [l, k)
//       k_lin_heavy_part   a slot with more than HEAVY_MIN terms: HEAVY_PARTS workgroups each sum a fixed slice of its segment
//       k_lin_heavy_fin    (LDS tree), one lane adds the HEAVY_PARTS partial sums in a fixed order -- a deterministic tree
//       k_lin_const_*      block-wise modular reduction over the n_rhs products b_c * r_c, finished (and negated) by a last block
//     rows no term touches are cleared with a memset.
// Field arithmetic: canonical 8 x u32 (fr.hpp).  A term costs one 256-bit modular add (~50 VALU instructions) against a random
// 32-byte gather from a vector that does not fit the last-level cache at 2^24 constraints: the pass is bound by the gather, not by
// VALU, so the 29-bit-limb forms of fr29.hpp would buy nothing here.
// Ownership: what the prepare makes is a lig_linear_program -- immutable once lig_linear_prepare returns,
// reference counted, bound to a device and (l, k), read by any number of traces of any context at once.  What one user of it writes
// per proof is a lig_linear, the ATTACHMENT: r, the heavy / constant partial sums, the pinned constant, and the Montgomery copy of a
// coefficient table that overrides the program's own (lig_rows_set_linear_values: k_lin_coefs_mont converts it on the device).
// One rank of a sharded trace (lig_shard_rows_set_linear) keeps the terms of its own rows and samples only the
// constraints those need: the k_lin_shard_* kernels of the prepare phase below, k_rng_fill_indexed (aes.hip) in the form phase.
#include <cstring>

#include <rocprim/device/device_scan.hpp>

#include "lin_common.hpp"
#include "prover_common.hpp"

namespace lig {
static constexpr uint32_t HEAVY_PARTS = 32;       // a slot with more than HEAVY_MIN terms is summed by this many workgroups
static constexpr uint32_t CONST_BLOCKS = 256;     // partial sums of the constant (one per workgroup), reduced by a last block

// ---------------------------------------------------------------- prepare
// constraint of term t: the c with term_begin[c] <= t < term_begin[c + 1] (constraints may be empty)
static __device__ __forceinline__ uint32_t lin_constraint_of(const uint32_t* __restrict__ term_begin, uint32_t n_constraints, uint32_t t) {
    uint32_t lo = 0, hi = n_constraints;          // first index in (0, n_constraints] whose entry is > t, minus one
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (term_begin[mid + 1] > t) hi = mid; else lo = mid + 1;
    }
    return lo;
}
__global__ void __launch_bounds__(LIN_WG) k_lin_count(const lig_lin_term* __restrict__ terms, uint32_t n_terms, uint32_t* __restrict__ count) {
    for (uint64_t t = blockIdx.x * LIN_WG + threadIdx.x; t < n_terms; t += gridDim.x * LIN_WG) atomicAdd(count + terms[t].slot, 1u);
}
__global__ void __launch_bounds__(LIN_WG) k_lin_scatter(const lig_lin_term* __restrict__ terms, uint32_t n_terms, const uint32_t* __restrict__ term_begin,
                                                        uint32_t n_constraints, const uint32_t* __restrict__ begin, uint32_t* __restrict__ cursor,
                                                        uint2* __restrict__ ent) {
    for (uint64_t t = blockIdx.x * LIN_WG + threadIdx.x; t < n_terms; t += gridDim.x * LIN_WG) {
        const lig_lin_term tm = terms[t];
        const uint32_t pos = begin[tm.slot] + atomicAdd(cursor + tm.slot, 1u);
        ent[pos] = make_uint2(lin_constraint_of(term_begin, n_constraints, (uint32_t)t), tm.coef);
    }
}
// which rows carry a term at all; which slots are heavy (appended in any order: the host sorts the list)
__global__ void __launch_bounds__(LIN_WG) k_lin_classify(const uint32_t* __restrict__ begin, uint32_t n_slots, uint32_t l, uint8_t* __restrict__ row_touched,
                                                         uint32_t* __restrict__ heavy, uint32_t heavy_cap, uint32_t* __restrict__ n_heavy) {
    for (uint64_t s = blockIdx.x * LIN_WG + threadIdx.x; s < n_slots; s += gridDim.x * LIN_WG) {
        const uint32_t cnt = begin[s + 1] - begin[s];
        if (cnt) row_touched[s / l] = 1;
        if (cnt > HEAVY_MIN) { const uint32_t i = atomicAdd(n_heavy, 1u); if (i < heavy_cap) heavy[i] = (uint32_t)s; }
    }
}

// ---------------------------------------------------------------- prepare, one rank of a sharded trace (lig_shard_rows_set_linear)
// The system describes the WHOLE trace; a rank keeps the terms whose row it was dealt (local_of: global row -> local row, LIN_NOT_LOCAL
// for the rows of other ranks), renumbered to local slots, and samples only the constraints it NEEDS: those with a kept term and those
// of its slice of the right-hand sides.  flag[c] = 1 marks them (plain stores of the same value from any number of lanes), an exclusive
// scan of the flags numbers them in ascending order, and the per-slot entries carry those compact numbers: r is need-list long.
static __device__ __forceinline__ uint32_t lin_local_slot(uint32_t slot, uint32_t l, const uint32_t* __restrict__ local_of) {
    const uint32_t row = slot / l, lr = local_of[row];
    return lr == LIN_NOT_LOCAL ? LIN_NOT_LOCAL : lr * l + (slot - row * l);
}
__global__ void __launch_bounds__(LIN_WG) k_lin_shard_count(const lig_lin_term* __restrict__ terms, uint32_t n_terms, const uint32_t* __restrict__ term_begin,
                                                            uint32_t n_constraints, uint32_t l, const uint32_t* __restrict__ local_of,
                                                            uint32_t* __restrict__ count, uint32_t* __restrict__ flag) {
    for (uint64_t t = blockIdx.x * LIN_WG + threadIdx.x; t < n_terms; t += gridDim.x * LIN_WG) {
        const uint32_t ls = lin_local_slot(terms[t].slot, l, local_of);
        if (ls == LIN_NOT_LOCAL) continue;
        atomicAdd(count + ls, 1u);
        flag[lin_constraint_of(term_begin, n_constraints, (uint32_t)t)] = 1u;
    }
}
// the rank's slice [lo, hi) of the right-hand sides
__global__ void __launch_bounds__(LIN_WG) k_lin_shard_mark_rhs(const uint32_t* __restrict__ rhs_c, uint32_t n, uint32_t* __restrict__ flag) {
    for (uint64_t i = blockIdx.x * LIN_WG + threadIdx.x; i < n; i += gridDim.x * LIN_WG) flag[rhs_c[i]] = 1u;
}
__global__ void __launch_bounds__(LIN_WG) k_lin_shard_scatter(const lig_lin_term* __restrict__ terms, uint32_t n_terms, const uint32_t* __restrict__ term_begin,
                                                              uint32_t n_constraints, uint32_t l, const uint32_t* __restrict__ local_of,
                                                              const uint32_t* __restrict__ compact, const uint32_t* __restrict__ begin,
                                                              uint32_t* __restrict__ cursor, uint2* __restrict__ ent) {
    for (uint64_t t = blockIdx.x * LIN_WG + threadIdx.x; t < n_terms; t += gridDim.x * LIN_WG) {
        const lig_lin_term tm = terms[t];
        const uint32_t ls = lin_local_slot(tm.slot, l, local_of);
        if (ls == LIN_NOT_LOCAL) continue;
        const uint32_t pos = begin[ls] + atomicAdd(cursor + ls, 1u);
        ent[pos] = make_uint2(compact[lin_constraint_of(term_begin, n_constraints, (uint32_t)t)], tm.coef);
    }
}
// need[compact[c]] = c for the marked constraints: ascending, every entry written exactly once
__global__ void __launch_bounds__(LIN_WG) k_lin_shard_need(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ compact, uint32_t n_constraints,
                                                           uint32_t* __restrict__ need) {
    for (uint64_t c = blockIdx.x * LIN_WG + threadIdx.x; c < n_constraints; c += gridDim.x * LIN_WG) if (flag[c]) need[compact[c]] = (uint32_t)c;
}
__global__ void __launch_bounds__(LIN_WG) k_lin_shard_rhs(uint32_t* __restrict__ rhs_c, uint32_t n, const uint32_t* __restrict__ compact) {
    for (uint64_t i = blockIdx.x * LIN_WG + threadIdx.x; i < n; i += gridDim.x * LIN_WG) rhs_c[i] = compact[rhs_c[i]];
}

// ---------------------------------------------------------------- form
// acc (canonical) += coef * r_c for one (constraint, coefficient) entry
static __device__ __forceinline__ fr lin_accumulate(const fr& acc, const uint2 e, const fr* __restrict__ r, const fr* __restrict__ coef_mont) {
    const fr v = fr_load(r + e.x);
    if (e.y == LIG_COEF_ONE) return fr_add(acc, v);
    if (e.y == LIG_COEF_NEG_ONE) return fr_sub(acc, v);
    return fr_add(acc, fr_montmul(v, fr_load(coef_mont + e.y)));      // (a R) * r / R = a * r, canonical
}
// lane = slot `col` of touched row trows[blockIdx.y + ...]; heavy slots are left to k_lin_heavy_*
__global__ void __launch_bounds__(LIN_WG) k_lin_form(const uint32_t* __restrict__ trows, uint32_t n_trows, uint32_t l, uint32_t k,
                                                     const uint32_t* __restrict__ begin, const uint2* __restrict__ ent, const fr* __restrict__ r,
                                                     const fr* __restrict__ coef_mont, fr* __restrict__ out) {
    const uint32_t col = blockIdx.x * LIN_WG + threadIdx.x;
    if (col >= k) return;
    for (uint32_t ti = blockIdx.y; ti < n_trows; ti += gridDim.y) {
        const uint32_t row = trows[ti];
        fr acc = fr_zero();
        if (col < l) {
            const uint32_t s = row * l + col, b = begin[s], e = begin[s + 1];
            if (e - b > HEAVY_MIN) continue;
            for (uint32_t i = b; i < e; i++) acc = lin_accumulate(acc, ent[i], r, coef_mont);
        }
        fr_store(out + (size_t)row * k + col, acc);
    }
}
// workgroup (h, p): slice p of the segment of heavy slot heavy[h]
__global__ void __launch_bounds__(LIN_WG) k_lin_heavy_part(const uint32_t* __restrict__ heavy, const uint32_t* __restrict__ begin, const uint2* __restrict__ ent,
                                                           const fr* __restrict__ r, const fr* __restrict__ coef_mont, fr* __restrict__ part) {
    __shared__ fr sh[LIN_WG];
    const uint32_t s = heavy[blockIdx.x], b = begin[s], cnt = begin[s + 1] - b;
    const uint32_t per = (cnt + HEAVY_PARTS - 1) / HEAVY_PARTS;
    const uint32_t lo = min(cnt, blockIdx.y * per), hi = min(cnt, lo + per);
    fr acc = fr_zero();
    for (uint32_t i = lo + threadIdx.x; i < hi; i += LIN_WG) acc = lin_accumulate(acc, ent[b + i], r, coef_mont);
    acc = lin_block_sum(acc, sh);
    if (threadIdx.x == 0) fr_store(part + (size_t)blockIdx.x * HEAVY_PARTS + blockIdx.y, acc);
}
__global__ void __launch_bounds__(LIN_WG) k_lin_heavy_fin(const uint32_t* __restrict__ heavy, uint32_t n_heavy, uint32_t l, uint32_t k, const fr* __restrict__ part,
                                                          fr* __restrict__ out) {
    const uint32_t h = blockIdx.x * LIN_WG + threadIdx.x;
    if (h >= n_heavy) return;
    fr acc = fr_zero();
    for (uint32_t p = 0; p < HEAVY_PARTS; p++) acc = fr_add(acc, fr_load(part + (size_t)h * HEAVY_PARTS + p));
    const uint32_t s = heavy[h];
    fr_store(out + (size_t)(s / l) * k + s % l, acc);
}
// partial sums of sum_i b_i * r_{c_i} over the constraints with a right-hand side
__global__ void __launch_bounds__(LIN_WG) k_lin_const_part(const uint32_t* __restrict__ rhs_c, const uint32_t* __restrict__ rhs_coef, uint32_t n_rhs,
                                                           const fr* __restrict__ r, const fr* __restrict__ coef_mont, fr* __restrict__ part) {
    __shared__ fr sh[LIN_WG];
    fr acc = fr_zero();
    for (uint64_t i = blockIdx.x * LIN_WG + threadIdx.x; i < n_rhs; i += gridDim.x * LIN_WG) acc = lin_accumulate(acc, make_uint2(rhs_c[i], rhs_coef[i]), r, coef_mont);
    acc = lin_block_sum(acc, sh);
    if (threadIdx.x == 0) fr_store(part + blockIdx.x, acc);
}
// one workgroup: out = - sum of the n_part partial sums; NEGATE = false (one rank of a sharded trace): the sum itself -- the ranks' sums
// are added in rank order and negated after the all-gather (shard.hip)
template <bool NEGATE>
__global__ void __launch_bounds__(LIN_WG) k_lin_const_fin(const fr* __restrict__ part, uint32_t n_part, fr* __restrict__ out) {
    __shared__ fr sh[LIN_WG];
    fr acc = fr_zero();
    for (uint32_t i = threadIdx.x; i < n_part; i += LIN_WG) acc = fr_add(acc, fr_load(part + i));
    acc = lin_block_sum(acc, sh);
    if (threadIdx.x == 0) fr_store(out, NEGATE ? fr_neg(acc) : acc);
}
// per-proof coefficient table (lig_rows_set_linear_values): canonical -> Montgomery form in place, one lane per entry, a * R^2 / R = a R;
// 16-byte loads and stores (fr_load / fr_store), no LDS, no atomics; the host has checked every entry < p
__global__ void __launch_bounds__(LIN_WG) k_lin_coefs_mont(fr* __restrict__ tab, uint64_t n) {
    const fr r2 = fr_const(FR_R2);
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LIN_WG) fr_store(tab + i, fr_montmul(fr_load(tab + i), r2));
}
void launch_lin_coefs_mont(hipStream_t st, fr* tab, uint64_t n) {
    if (!n) return;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + LIN_WG - 1) / LIN_WG, COEFS_MAX_BLOCKS);
    hipLaunchKernelGGL(k_lin_coefs_mont, dim3(blocks), dim3(LIN_WG), 0, st, tab, n);
}
}  // namespace lig

// a linear system on the device, regrouped by slot (lig_linear_prepare): nothing writes its device memory once the prepare has returned
struct lig_linear_program {
    mutable std::atomic<uint32_t> refs{1};
    int device = 0;
    std::vector<uint8_t> kinds;         // the row kinds it was checked against, LIG_ROW_DRAW_PAD masked off (empty: one rank of a sharded trace)
    size_t dev_bytes = 0;               // device memory it holds
    uint32_t l = 0, k = 0;
    uint64_t rows = 0, n_constraints = 0, n_terms = 0, n_rhs = 0, n_coefs = 0, first_random = 0;
    uint32_t n_slots = 0, n_heavy = 0, n_trows = 0;
    uint32_t* begin = nullptr;          // n_slots + 1: the segment of slot s is ent[begin[s] .. begin[s + 1])
    uint2* ent = nullptr;               // n_terms (constraint, coefficient index) pairs in slot order
    fr* coef_mont = nullptr;            // the coefficient table, Montgomery form
    uint32_t* rhs_c = nullptr; uint32_t* rhs_coef = nullptr;
    uint32_t* heavy = nullptr;          // slots with more than HEAVY_MIN terms, ascending
    uint32_t* trows = nullptr;          // rows with at least one term, ascending
    // one rank of a sharded trace (lig_internal_linear_create_shard): rows / n_slots / trows / zero_runs are LOCAL, n_terms = the terms kept,
    // n_rhs = the rank's slice of the right-hand sides, ent[].x and rhs_c[] index r through the need list
    bool sharded = false;
    uint32_t* need = nullptr;           // n_need constraint numbers, ascending: r[i] = stream element first_random + need[i]
    uint64_t n_need = 0;
    std::vector<std::pair<uint64_t, uint64_t>> zero_runs;      // (first row, rows) no term touches
};
// one user of a program (a trace, a verifier trace, one lig_linear_program_form call): holds a reference and everything a form writes
struct lig_linear {
    lig_ctx* c = nullptr;
    const lig_linear_program* P = nullptr;
    fr* r = nullptr;                    // n_constraints stream elements (per proof); one rank of a sharded trace: n_need
    fr* part = nullptr;                 // n_heavy x HEAVY_PARTS | CONST_BLOCKS | the constant
    uint8_t* h_const = nullptr;         // pinned, 32 bytes: the constant of the last form
    const fr* coef = nullptr;           // the table the form kernels read: P->coef_mont, or vals
    fr* vals = nullptr;                 // lig_rows_set_linear_values: n_coefs elements, Montgomery form once k_lin_coefs_mont has run
    uint8_t* h_vals = nullptr;          // pinned staging of the canonical table: the caller's memory is free when set_values returns
    hipEvent_t ev_vals = nullptr;       // the copy out of h_vals has finished
    hipEvent_t ev_mont = nullptr;       // ... and k_lin_coefs_mont behind it: `vals` is in Montgomery form (a reader on another stream waits for it)
};

static bool lin_coef_ok(uint32_t coef, uint64_t n_coefs) { return coef == LIG_COEF_ONE || coef == LIG_COEF_NEG_ONE || coef < n_coefs; }

extern "C" int lig_linear_check(const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, uint32_t l) {
    if (!sys || sys->struct_bytes < sizeof(lig_linear_system)) return LIG_E_ARG;
    if (!l || (rows && !kinds) || rows * (uint64_t)l >= (1ull << 32) || rows >= (1ull << 32)) return LIG_E_ARG;
    if (sys->n_terms >= (1ull << 32) || sys->n_constraints >= 0xFFFFFFFFull || sys->n_rhs > sys->n_constraints || sys->n_coefs >= LIG_COEF_NEG_ONE) return LIG_E_ARG;
    if (sys->first_random + sys->n_constraints < sys->first_random) return LIG_E_ARG;
    if (!sys->term_begin || (sys->n_terms && !sys->terms) || (sys->n_rhs && (!sys->rhs_constraint || !sys->rhs_coef)) || (sys->n_coefs && !sys->coefs)) return LIG_E_ARG;
    if (sys->term_begin[0] != 0 || sys->term_begin[sys->n_constraints] != sys->n_terms) return LIG_E_ARG;
    for (uint64_t c = 0; c < sys->n_constraints; c++) if (sys->term_begin[c + 1] < sys->term_begin[c]) return LIG_E_ARG;
    for (uint64_t t = 0; t < sys->n_terms; t++) {
        const uint64_t row = sys->terms[t].slot / l;
        if (row >= rows || (kinds[row] & 0x7f) > LIG_ROW_QZ || !lin_coef_ok(sys->terms[t].coef, sys->n_coefs)) return LIG_E_ARG;
    }
    for (uint64_t i = 0; i < sys->n_rhs; i++) {
        if (sys->rhs_constraint[i] >= sys->n_constraints || (i && sys->rhs_constraint[i] <= sys->rhs_constraint[i - 1])) return LIG_E_ARG;
        if (!lin_coef_ok(sys->rhs_coef[i], sys->n_coefs)) return LIG_E_ARG;
    }
    for (uint64_t i = 0; i < sys->n_coefs; i++) {
        H::Fr v;
        std::memcpy(v.v, sys->coefs + 32 * i, 32);
        if (H::geq(v, H::P)) return LIG_E_ARG;
    }
    return LIG_OK;
}

static void linear_program_retain(const lig_linear_program* P) { P->refs.fetch_add(1, std::memory_order_relaxed); }
// the last reference frees the device memory; every attachment has drained its own streams before it drops its reference
// (lig_internal_linear_destroy), so nothing reads the program any more
static void linear_program_release(const lig_linear_program* P) {
    if (!P || P->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(P->device);
    for (void* p : {(void*)P->begin, (void*)P->ent, (void*)P->coef_mont, (void*)P->rhs_c, (void*)P->rhs_coef, (void*)P->heavy, (void*)P->trows, (void*)P->need})
        (void)hipFree(p);
    if (prev >= 0 && prev != P->device) (void)hipSetDevice(prev);
    delete P;
}
void lig_internal_linear_destroy(lig_linear* L) {
    if (!L) return;
    (void)hipSetDevice(L->c->device);
    for (hipStream_t st : {L->c->stream, L->c->stream2}) if (st) (void)hipStreamSynchronize(st);
    for (void* p : {(void*)L->r, (void*)L->part, (void*)L->vals}) (void)hipFree(p);
    (void)hipHostFree(L->h_const);
    (void)hipHostFree(L->h_vals);
    if (L->ev_vals) (void)hipEventDestroy(L->ev_vals);
    if (L->ev_mont) (void)hipEventDestroy(L->ev_mont);
    linear_program_release(L->P);
    delete L;
}

static uint32_t lin_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + lig::LIN_WG - 1) / lig::LIN_WG, 1), 65535); }

// the end of both prepares: heavy slots sorted, touched rows listed, runs of untouched rows
static int linear_prepare_lists(lig_ctx* c, lig_linear_program* L, const uint8_t* d_touched, const uint32_t* d_nheavy, uint32_t heavy_cap) {
    hipStream_t s = c->stream;
    auto dmalloc = [&](void** p, size_t bytes) -> int { HIP_TRY(c, hipMalloc(p, bytes ? bytes : 16)); L->dev_bytes += bytes ? bytes : 16; return LIG_OK; };
    std::vector<uint8_t> touched(L->rows);
    uint32_t n_heavy = 0;
    if (L->rows) HIP_TRY(c, hipMemcpyAsync(touched.data(), d_touched, L->rows, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&n_heavy, d_nheavy, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (n_heavy > heavy_cap) FAIL(c, LIG_E_STATE, "linear system: heavy-slot list overflow");      // (cannot happen: more than HEAVY_MIN terms each)
    L->n_heavy = n_heavy;
    if (n_heavy) {      // ascending: the same launch geometry whatever order the atomics appended them in
        std::vector<uint32_t> hv(n_heavy);
        HIP_TRY(c, hipMemcpy(hv.data(), L->heavy, (size_t)n_heavy * 4, hipMemcpyDeviceToHost));
        std::sort(hv.begin(), hv.end());
        HIP_TRY(c, hipMemcpy(L->heavy, hv.data(), (size_t)n_heavy * 4, hipMemcpyHostToDevice));
    }
    std::vector<uint32_t> trows;
    for (uint64_t r = 0; r < L->rows;) {
        if (touched[r]) { trows.push_back((uint32_t)r); r++; continue; }
        uint64_t e = r + 1;
        while (e < L->rows && !touched[e]) e++;
        L->zero_runs.push_back({r, e - r});
        r = e;
    }
    L->n_trows = (uint32_t)trows.size();
    TRY(dmalloc((void**)&L->trows, trows.size() * 4));
    if (!trows.empty()) HIP_TRY(c, hipMemcpy(L->trows, trows.data(), trows.size() * 4, hipMemcpyHostToDevice));
    return LIG_OK;
}

static int linear_prepare(lig_ctx* c, const lig_linear_system* sys, lig_linear_program* L) {
    hipStream_t s = c->stream;
    const uint32_t S = L->n_slots, NT = (uint32_t)L->n_terms, NC = (uint32_t)L->n_constraints;
    auto dmalloc = [&](void** p, size_t bytes) -> int { HIP_TRY(c, hipMalloc(p, bytes ? bytes : 16)); return LIG_OK; };
    auto keep = [&](void** p, size_t bytes) -> int { TRY(dmalloc(p, bytes)); L->dev_bytes += bytes ? bytes : 16; return LIG_OK; };      // memory of the program
    TRY(keep((void**)&L->begin, ((size_t)S + 1) * 4));
    TRY(keep((void**)&L->ent, (size_t)NT * sizeof(uint2)));
    TRY(keep((void**)&L->coef_mont, L->n_coefs * 32));
    TRY(keep((void**)&L->rhs_c, L->n_rhs * 4));
    TRY(keep((void**)&L->rhs_coef, L->n_rhs * 4));
    const uint32_t heavy_cap = NT / (lig::HEAVY_MIN + 1) + 1;
    TRY(keep((void**)&L->heavy, (size_t)heavy_cap * 4));
    // scratch of this call only
    lig_lin_term* d_terms = nullptr; uint32_t *d_tb = nullptr, *d_cursor = nullptr, *d_count = nullptr, *d_nheavy = nullptr; uint8_t* d_touched = nullptr; void* d_scan = nullptr;
    struct Scratch { std::vector<void**> v; lig_ctx* c; ~Scratch() { (void)hipStreamSynchronize(c->stream); for (void** p : v) (void)hipFree(*p); } }
        scratch{{(void**)&d_terms, (void**)&d_tb, (void**)&d_cursor, (void**)&d_count, (void**)&d_nheavy, (void**)&d_touched, &d_scan}, c};
    TRY(dmalloc((void**)&d_terms, (size_t)NT * sizeof(lig_lin_term)));
    TRY(dmalloc((void**)&d_tb, ((size_t)NC + 1) * 4));
    TRY(dmalloc((void**)&d_cursor, (size_t)S * 4));
    TRY(dmalloc((void**)&d_count, ((size_t)S + 1) * 4));
    TRY(dmalloc((void**)&d_nheavy, 4));
    TRY(dmalloc((void**)&d_touched, L->rows));
    // the coefficient table in Montgomery form: a term with a table coefficient is one Montgomery product
    std::vector<H::Fr> cm(L->n_coefs);
    for (uint64_t i = 0; i < L->n_coefs; i++) { H::Fr v; std::memcpy(v.v, sys->coefs + 32 * i, 32); cm[i] = H::to_mont(v); }
    if (NT) HIP_TRY(c, hipMemcpyAsync(d_terms, sys->terms, (size_t)NT * sizeof(lig_lin_term), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_tb, sys->term_begin, ((size_t)NC + 1) * 4, hipMemcpyHostToDevice, s));
    if (L->n_coefs) HIP_TRY(c, hipMemcpyAsync(L->coef_mont, cm.data(), L->n_coefs * 32, hipMemcpyHostToDevice, s));
    if (L->n_rhs) {
        HIP_TRY(c, hipMemcpyAsync(L->rhs_c, sys->rhs_constraint, L->n_rhs * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(L->rhs_coef, sys->rhs_coef, L->n_rhs * 4, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(c, hipMemsetAsync(d_count, 0, ((size_t)S + 1) * 4, s));
    HIP_TRY(c, hipMemsetAsync(d_cursor, 0, (size_t)S * 4, s));
    HIP_TRY(c, hipMemsetAsync(d_nheavy, 0, 4, s));
    if (L->rows) HIP_TRY(c, hipMemsetAsync(d_touched, 0, L->rows, s));
    if (NT) hipLaunchKernelGGL(lig::k_lin_count, dim3(lin_grid(NT)), dim3(lig::LIN_WG), 0, s, d_terms, NT, d_count);
    size_t scan_bytes = 0;
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, d_count, L->begin, 0u, (size_t)S + 1, rocprim::plus<uint32_t>(), s));
    TRY(dmalloc(&d_scan, scan_bytes));
    HIP_TRY(c, rocprim::exclusive_scan(d_scan, scan_bytes, d_count, L->begin, 0u, (size_t)S + 1, rocprim::plus<uint32_t>(), s));
    if (NT) hipLaunchKernelGGL(lig::k_lin_scatter, dim3(lin_grid(NT)), dim3(lig::LIN_WG), 0, s, d_terms, NT, d_tb, NC, L->begin, d_cursor, L->ent);
    if (S) hipLaunchKernelGGL(lig::k_lin_classify, dim3(lin_grid(S)), dim3(lig::LIN_WG), 0, s, L->begin, S, L->l, d_touched, L->heavy, heavy_cap, d_nheavy);
    HIP_TRY(c, hipGetLastError());
    return linear_prepare_lists(c, L, d_touched, d_nheavy, heavy_cap);
}

// one rank of a sharded trace: local_of = global row -> local row (LIN_NOT_LOCAL: another rank's), rows_local = the rank's rows;
// the rank's slice of the right-hand sides = entries [rhs_lo, rhs_hi)
static int linear_prepare_shard(lig_ctx* c, const lig_linear_system* sys, lig_linear_program* L, const uint32_t* local_of, uint64_t rows_global, uint64_t rhs_lo,
                                uint64_t rhs_hi) {
    hipStream_t s = c->stream;
    const uint32_t S = L->n_slots, NT = (uint32_t)sys->n_terms, NC = (uint32_t)L->n_constraints, NR = (uint32_t)(rhs_hi - rhs_lo);
    auto dmalloc = [&](void** p, size_t bytes) -> int { HIP_TRY(c, hipMalloc(p, bytes ? bytes : 16)); return LIG_OK; };
    auto keep = [&](void** p, size_t bytes) -> int { TRY(dmalloc(p, bytes)); L->dev_bytes += bytes ? bytes : 16; return LIG_OK; };      // memory of the program
    L->n_rhs = NR;
    TRY(keep((void**)&L->begin, ((size_t)S + 1) * 4));
    TRY(keep((void**)&L->coef_mont, L->n_coefs * 32));
    TRY(keep((void**)&L->rhs_c, (size_t)NR * 4));
    TRY(keep((void**)&L->rhs_coef, (size_t)NR * 4));
    const uint32_t heavy_cap = NT / (lig::HEAVY_MIN + 1) + 1;
    TRY(keep((void**)&L->heavy, (size_t)heavy_cap * 4));
    std::vector<H::Fr> cm(L->n_coefs);         // (declared before the guard below: it outlives the guard's synchronise, an async copy reads it)
    // scratch of this call only
    lig_lin_term* d_terms = nullptr; uint32_t *d_tb = nullptr, *d_cursor = nullptr, *d_count = nullptr, *d_nheavy = nullptr, *d_local = nullptr, *d_flag = nullptr, *d_compact = nullptr;
    uint8_t* d_touched = nullptr; void* d_scan = nullptr;
    struct Scratch { std::vector<void**> v; lig_ctx* c; ~Scratch() { (void)hipStreamSynchronize(c->stream); for (void** p : v) (void)hipFree(*p); } }
        scratch{{(void**)&d_terms, (void**)&d_tb, (void**)&d_cursor, (void**)&d_count, (void**)&d_nheavy, (void**)&d_local, (void**)&d_flag, (void**)&d_compact,
                 (void**)&d_touched, &d_scan}, c};
    TRY(dmalloc((void**)&d_terms, (size_t)NT * sizeof(lig_lin_term)));
    TRY(dmalloc((void**)&d_tb, ((size_t)NC + 1) * 4));
    TRY(dmalloc((void**)&d_cursor, (size_t)S * 4));
    TRY(dmalloc((void**)&d_count, ((size_t)S + 1) * 4));
    TRY(dmalloc((void**)&d_nheavy, 4));
    TRY(dmalloc((void**)&d_local, rows_global * 4));
    TRY(dmalloc((void**)&d_flag, ((size_t)NC + 1) * 4));
    TRY(dmalloc((void**)&d_compact, ((size_t)NC + 1) * 4));
    TRY(dmalloc((void**)&d_touched, L->rows));
    for (uint64_t i = 0; i < L->n_coefs; i++) { H::Fr v; std::memcpy(v.v, sys->coefs + 32 * i, 32); cm[i] = H::to_mont(v); }
    if (NT) HIP_TRY(c, hipMemcpyAsync(d_terms, sys->terms, (size_t)NT * sizeof(lig_lin_term), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_tb, sys->term_begin, ((size_t)NC + 1) * 4, hipMemcpyHostToDevice, s));
    if (rows_global) HIP_TRY(c, hipMemcpyAsync(d_local, local_of, rows_global * 4, hipMemcpyHostToDevice, s));
    if (L->n_coefs) HIP_TRY(c, hipMemcpyAsync(L->coef_mont, cm.data(), L->n_coefs * 32, hipMemcpyHostToDevice, s));
    if (NR) {
        HIP_TRY(c, hipMemcpyAsync(L->rhs_c, sys->rhs_constraint + rhs_lo, (size_t)NR * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(L->rhs_coef, sys->rhs_coef + rhs_lo, (size_t)NR * 4, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(c, hipMemsetAsync(d_count, 0, ((size_t)S + 1) * 4, s));
    HIP_TRY(c, hipMemsetAsync(d_cursor, 0, (size_t)S * 4, s));
    HIP_TRY(c, hipMemsetAsync(d_flag, 0, ((size_t)NC + 1) * 4, s));
    HIP_TRY(c, hipMemsetAsync(d_nheavy, 0, 4, s));
    if (L->rows) HIP_TRY(c, hipMemsetAsync(d_touched, 0, L->rows, s));
    if (NT) hipLaunchKernelGGL(lig::k_lin_shard_count, dim3(lin_grid(NT)), dim3(lig::LIN_WG), 0, s, d_terms, NT, d_tb, NC, L->l, d_local, d_count, d_flag);
    if (NR) hipLaunchKernelGGL(lig::k_lin_shard_mark_rhs, dim3(lin_grid(NR)), dim3(lig::LIN_WG), 0, s, L->rhs_c, NR, d_flag);
    size_t scan_slots = 0, scan_flags = 0;
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_slots, d_count, L->begin, 0u, (size_t)S + 1, rocprim::plus<uint32_t>(), s));
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_flags, d_flag, d_compact, 0u, (size_t)NC + 1, rocprim::plus<uint32_t>(), s));
    const size_t scan_bytes = std::max(scan_slots, scan_flags);
    TRY(dmalloc(&d_scan, scan_bytes));
    scan_slots = scan_flags = scan_bytes;
    HIP_TRY(c, rocprim::exclusive_scan(d_scan, scan_slots, d_count, L->begin, 0u, (size_t)S + 1, rocprim::plus<uint32_t>(), s));
    HIP_TRY(c, rocprim::exclusive_scan(d_scan, scan_flags, d_flag, d_compact, 0u, (size_t)NC + 1, rocprim::plus<uint32_t>(), s));
    // how many terms were kept, how many constraints are needed: the sizes of ent / need / r
    uint32_t kept = 0, n_need = 0;
    HIP_TRY(c, hipMemcpyAsync(&kept, L->begin + S, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&n_need, d_compact + NC, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (kept > NT || n_need > NC) FAIL(c, LIG_E_STATE, "linear system: sharded prepare counted more than the system holds");
    L->n_terms = kept; L->n_need = n_need;
    TRY(keep((void**)&L->ent, (size_t)kept * sizeof(uint2)));
    TRY(keep((void**)&L->need, (size_t)n_need * 4));
    if (NT) hipLaunchKernelGGL(lig::k_lin_shard_scatter, dim3(lin_grid(NT)), dim3(lig::LIN_WG), 0, s, d_terms, NT, d_tb, NC, L->l, d_local, d_compact, L->begin, d_cursor, L->ent);
    if (NC) hipLaunchKernelGGL(lig::k_lin_shard_need, dim3(lin_grid(NC)), dim3(lig::LIN_WG), 0, s, d_flag, d_compact, NC, L->need);
    if (NR) hipLaunchKernelGGL(lig::k_lin_shard_rhs, dim3(lin_grid(NR)), dim3(lig::LIN_WG), 0, s, L->rhs_c, NR, d_compact);
    if (S) hipLaunchKernelGGL(lig::k_lin_classify, dim3(lin_grid(S)), dim3(lig::LIN_WG), 0, s, L->begin, S, L->l, d_touched, L->heavy, heavy_cap, d_nheavy);
    HIP_TRY(c, hipGetLastError());
    return linear_prepare_lists(c, L, d_touched, d_nheavy, heavy_cap);
}

// check, upload, regroup by slot; synchronous (every pointer of *sys may be released when it returns).  The caller owns one reference.
int lig_internal_linear_prepare(lig_ctx* c, const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, lig_linear_program** out) {
    *out = nullptr;
    if (lig_linear_check(sys, kinds, rows, c->l) != LIG_OK) FAIL(c, LIG_E_ARG, "linear system: rejected by lig_linear_check");
    lig_linear_program* L = new lig_linear_program();
    L->device = c->device; L->l = c->l; L->k = c->k; L->rows = rows;
    L->kinds.resize(rows);
    for (uint64_t r = 0; r < rows; r++) L->kinds[r] = kinds[r] & 0x7f;
    L->n_constraints = sys->n_constraints; L->n_terms = sys->n_terms; L->n_rhs = sys->n_rhs; L->n_coefs = sys->n_coefs; L->first_random = sys->first_random;
    L->n_slots = (uint32_t)(rows * c->l);
    const int rc = linear_prepare(c, sys, L);
    if (rc != LIG_OK) { linear_program_release(L); return rc; }
    *out = L;
    return LIG_OK;
}
// device memory of one attachment: the sampled elements, the partial sums (+ n_coefs x 32 once values are set)
static size_t linear_r_bytes(const lig_linear_program* P) { return std::max<size_t>((size_t)(P->sharded ? P->n_need : P->n_constraints) * 32, 16); }
static size_t linear_part_bytes(const lig_linear_program* P) { return ((size_t)P->n_heavy * lig::HEAVY_PARTS + lig::CONST_BLOCKS + 1) * 32; }
// the per-proof buffers of one user of P on context c; holds a reference to P until lig_internal_linear_destroy
int lig_internal_linear_attach(lig_ctx* c, const lig_linear_program* P, lig_linear** out) {
    *out = nullptr;
    lig_linear* L = new lig_linear();
    L->c = c; L->P = P; L->coef = P->coef_mont;
    linear_program_retain(P);
    const size_t r_bytes = linear_r_bytes(P), part_bytes = linear_part_bytes(P);
    hipError_t e = hipMalloc((void**)&L->r, r_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&L->part, part_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void**)&L->h_const, 32, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        lig_internal_linear_destroy(L);
        FAIL(c, LIG_E_NOMEM, std::string("linear system: per-proof buffers: ") + hipGetErrorString(e));
    }
    std::memset(L->h_const, 0, 32);
    *out = L;
    return LIG_OK;
}
// what lig_rows_set_linear has always done: a program of its own, attached, the only reference held by the attachment
int lig_internal_linear_create(lig_ctx* c, const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, lig_linear** out) {
    *out = nullptr;
    lig_linear_program* P = nullptr;
    TRY(lig_internal_linear_prepare(c, sys, kinds, rows, &P));
    const int rc = lig_internal_linear_attach(c, P, out);
    linear_program_release(P);
    return rc;
}
// does a trace of context c with these rows fit P?  (host only)
bool lig_internal_linear_fits(const lig_ctx* c, const lig_linear_program* P, const uint8_t* kinds, uint64_t rows) {
    if (P->sharded || c->device != P->device || c->l != P->l || c->k != P->k || rows != P->rows) return false;
    for (uint64_t r = 0; r < rows; r++) if ((kinds[r] & 0x7f) != P->kinds[r]) return false;
    return true;
}
// per-proof values of the coefficient table: host check, pinned copy, upload and k_lin_coefs_mont on `st` -- the stream the
// attachment's forms run on, so a form queued later reads the converted table.  coefs == NULL: the program's own table again.
int lig_internal_linear_set_values(lig_ctx* c, lig_linear* L, const uint8_t* coefs, uint64_t n_coefs, hipStream_t st) {
    const lig_linear_program* P = L->P;
    if (!coefs) { L->coef = P->coef_mont; return LIG_OK; }
    if (n_coefs != P->n_coefs) FAIL(c, LIG_E_ARG, "linear values: n_coefs differs from the program's");
    for (uint64_t i = 0; i < n_coefs; i++) {
        H::Fr v;
        std::memcpy(v.v, coefs + 32 * i, 32);
        if (H::geq(v, H::P)) FAIL(c, LIG_E_ARG, "linear values: an entry is not reduced mod p");
    }
    if (!n_coefs) { L->coef = P->coef_mont; return LIG_OK; }
    const size_t bytes = (size_t)n_coefs * 32;
    if (!L->vals) HIP_TRY(c, hipMalloc((void**)&L->vals, bytes));
    if (!L->h_vals) HIP_TRY(c, hipHostMalloc((void**)&L->h_vals, bytes, hipHostMallocDefault));
    if (!L->ev_vals) HIP_TRY(c, hipEventCreateWithFlags(&L->ev_vals, hipEventDisableTiming));
    else HIP_TRY(c, hipEventSynchronize(L->ev_vals));          // the copy of the previous table out of the staging buffer
    if (!L->ev_mont) HIP_TRY(c, hipEventCreateWithFlags(&L->ev_mont, hipEventDisableTiming));
    std::memcpy(L->h_vals, coefs, bytes);
    HIP_TRY(c, hipMemcpyAsync(L->vals, L->h_vals, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(L->ev_vals, st));
    lig::launch_lin_coefs_mont(st, L->vals, n_coefs);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(L->ev_mont, st));
    L->coef = L->vals;
    return LIG_OK;
}
// what lig_rows_diagnose_attached / lig_shard_rows_diagnose_attached (diagnose.hip) read of an attachment; nothing of it is written through the view
lig_linear_view lig_internal_linear_view(const lig_linear* L) {
    lig_linear_view v = lig_internal_linear_program_view(L->P);
    v.coef = L->coef;
    v.coef_ready = L->coef == L->vals && L->vals ? L->ev_mont : nullptr;
    return v;
}
// a program nobody is attached to (the temporary one of lig_rows_explain_slots / lig_rows_untouched_slots): its own table is in force
lig_linear_view lig_internal_linear_program_view(const lig_linear_program* P) {
    lig_linear_view v;
    v.sharded = P->sharded;
    v.n_constraints = P->n_constraints; v.n_terms = P->n_terms; v.n_rhs = P->n_rhs; v.n_slots = P->n_slots;
    v.begin = P->begin; v.ent = P->ent; v.rhs_c = P->rhs_c; v.rhs_coef = P->rhs_coef;
    v.need = P->need; v.n_need = P->n_need; v.rows_local = P->sharded ? P->rows : 0;
    v.coef = P->coef_mont;
    return v;
}

// this rank's share of a deal: which rows are local, its slice of the right-hand sides.  grow = the global row of every local row.
static void linear_shard_share(const lig_linear_system* sys, const std::vector<size_t>& grow, uint64_t rows, uint32_t rank, uint32_t world,
                               std::vector<uint32_t>& local_of, uint64_t& rhs_lo, uint64_t& rhs_hi) {
    local_of.assign(rows, lig::LIN_NOT_LOCAL);
    for (size_t lr = 0; lr < grow.size(); lr++) local_of[grow[lr]] = (uint32_t)lr;
    rhs_lo = (uint64_t)((unsigned __int128)rank * sys->n_rhs / world);
    rhs_hi = (uint64_t)((unsigned __int128)(rank + 1) * sys->n_rhs / world);
}
// the two numbers of lig_shard_rows_linear_stats on the host (lig_linear_shard_count); sys has passed lig_linear_check
void lig_internal_linear_shard_count(const lig_linear_system* sys, uint32_t l, const std::vector<size_t>& grow, uint64_t rows, uint32_t rank, uint32_t world,
                                     uint64_t* local_terms, uint64_t* needed) {
    std::vector<uint32_t> local_of;
    uint64_t lo, hi;
    linear_shard_share(sys, grow, rows, rank, world, local_of, lo, hi);
    uint64_t kept = 0, need = 0, i = lo;
    for (uint64_t cn = 0; cn < sys->n_constraints; cn++) {
        uint64_t mine = 0;
        for (uint32_t t = sys->term_begin[cn]; t < sys->term_begin[cn + 1]; t++) mine += local_of[sys->terms[t].slot / l] != lig::LIN_NOT_LOCAL;
        while (i < hi && sys->rhs_constraint[i] < cn) i++;
        kept += mine;
        need += mine || (i < hi && sys->rhs_constraint[i] == cn);
    }
    *local_terms = kept; *needed = need;
}
// one rank of a sharded trace (lig_shard_rows_set_linear): kinds / rows describe the WHOLE trace (lig_linear_check runs on it), grow is the
// global row of every row dealt to this rank; the structure that comes out addresses the rank's local rows x k matrix
int lig_internal_linear_create_shard(lig_ctx* c, const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, const std::vector<size_t>& grow, uint32_t rank,
                                     uint32_t world, lig_linear** out) {
    *out = nullptr;
    if (lig_linear_check(sys, kinds, rows, c->l) != LIG_OK) FAIL(c, LIG_E_ARG, "linear system: rejected by lig_linear_check");
    std::vector<uint32_t> local_of;
    uint64_t lo, hi;
    linear_shard_share(sys, grow, rows, rank, world, local_of, lo, hi);
    lig_linear_program* L = new lig_linear_program();      // the rank's own: it depends on the deal, nothing shares it
    L->device = c->device; L->l = c->l; L->k = c->k; L->rows = grow.size(); L->sharded = true;
    L->n_constraints = sys->n_constraints; L->n_coefs = sys->n_coefs; L->first_random = sys->first_random;
    L->n_slots = (uint32_t)(grow.size() * c->l);
    int rc = linear_prepare_shard(c, sys, L, local_of.data(), rows, lo, hi);
    if (rc == LIG_OK) rc = lig_internal_linear_attach(c, L, out);
    linear_program_release(L);
    return rc;
}
void lig_internal_linear_stats(const lig_linear* L, uint64_t* local_terms, uint64_t* sampled) { *local_terms = L->P->n_terms; *sampled = L->P->sharded ? L->P->n_need : L->P->n_constraints; }
// one rank of a sharded trace: the rank's sum of b_c r_c (NOT negated), one element of device memory, final once the form queued on its stream is
const fr* lig_internal_linear_partial_dev(const lig_linear* L) { return L->part + (size_t)L->P->n_heavy * lig::HEAVY_PARTS + lig::CONST_BLOCKS; }
uint8_t* lig_internal_linear_const_buf(lig_linear* L) { return L->h_const; }

// enqueue on `st`: rands_dev (rows x k) <- the randomness matrix of the system for the stream whose round keys are in rk60_dev;
// the constant lands in lig_internal_linear_const() once the work queued on `st` has been waited for.  One rank of a sharded trace: the
// LOCAL rows x k matrix from the need-list long r (indexed sampler), and the rank's un-negated sum in lig_internal_linear_partial_dev()
int lig_internal_linear_form(lig_ctx* c, lig_linear* A, const uint32_t* rk60_dev, fr* rands_dev, hipStream_t st) {
    const lig_linear_program* L = A->P;
    const size_t row_bytes = (size_t)L->k * 32;
    for (const auto& z : L->zero_runs) HIP_TRY(c, hipMemsetAsync(rands_dev + z.first * L->k, 0, z.second * row_bytes, st));
    if (L->sharded) lig::launch_rng_fill_indexed(st, rk60_dev, L->first_random, L->need, A->r, L->n_need);
    else lig::launch_rng_fill(st, rk60_dev, L->first_random, A->r, L->n_constraints);
    fr* hpart = A->part; fr* cpart = A->part + (size_t)L->n_heavy * lig::HEAVY_PARTS; fr* cst = cpart + lig::CONST_BLOCKS;
    if (L->n_trows) {
        const dim3 grid((L->k + lig::LIN_WG - 1) / lig::LIN_WG, std::min<uint32_t>(L->n_trows, 65535));
        hipLaunchKernelGGL(lig::k_lin_form, grid, dim3(lig::LIN_WG), 0, st, L->trows, L->n_trows, L->l, L->k, L->begin, L->ent, A->r, A->coef, rands_dev);
    }
    if (L->n_heavy) {
        hipLaunchKernelGGL(lig::k_lin_heavy_part, dim3(L->n_heavy, lig::HEAVY_PARTS), dim3(lig::LIN_WG), 0, st, L->heavy, L->begin, L->ent, A->r, A->coef, hpart);
        hipLaunchKernelGGL(lig::k_lin_heavy_fin, dim3((L->n_heavy + lig::LIN_WG - 1) / lig::LIN_WG), dim3(lig::LIN_WG), 0, st, L->heavy, L->n_heavy, L->l, L->k, hpart, rands_dev);
    }
    const uint32_t cb = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((L->n_rhs + lig::LIN_WG - 1) / lig::LIN_WG, 1), lig::CONST_BLOCKS);
    hipLaunchKernelGGL(lig::k_lin_const_part, dim3(cb), dim3(lig::LIN_WG), 0, st, L->rhs_c, L->rhs_coef, (uint32_t)L->n_rhs, A->r, A->coef, cpart);
    if (L->sharded) {
        hipLaunchKernelGGL(lig::k_lin_const_fin<false>, dim3(1), dim3(lig::LIN_WG), 0, st, cpart, cb, cst);
        HIP_TRY(c, hipGetLastError());
        return LIG_OK;
    }
    hipLaunchKernelGGL(lig::k_lin_const_fin<true>, dim3(1), dim3(lig::LIN_WG), 0, st, cpart, cb, cst);
    HIP_TRY(c, hipGetLastError());
    return lig_internal_download(c, A->h_const, cst, 32, st);
}
const uint8_t* lig_internal_linear_const(const lig_linear* L) { return L->h_const; }

// key -> round keys -> form on the context stream, waited for; `A` is destroyed whatever happens
static int linear_form_once(lig_ctx* c, lig_linear* A, const uint8_t key32[32], void* rands_dev, uint8_t const_sum[32], const char* who) {
    uint32_t rk[60];
    lig::aes256_expand_host(key32, rk);
    int rc = lig_internal_upload_small(c, c->rk_dev, rk, sizeof rk, c->stream);
    if (rc == LIG_OK) rc = lig_internal_linear_form(c, A, c->rk_dev, (fr*)rands_dev, c->stream);
    if (rc == LIG_OK && hipStreamSynchronize(c->stream) != hipSuccess) { c->err = std::string(who) + ": stream synchronize failed"; rc = LIG_E_HIP; }
    if (rc == LIG_OK) std::memcpy(const_sum, A->h_const, 32);
    const std::string why = c->err;
    lig_internal_linear_destroy(A);
    c->err = why;
    return rc;
}
extern "C" int lig_linear_form(lig_ctx* c, const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, const uint8_t key32[32], void* rands_dev,
                               uint8_t const_sum[32]) {
    CHECK_CTX(c);
    if (!key32 || !const_sum || (rows && !rands_dev)) return LIG_E_ARG;
    lig_linear* L = nullptr;
    TRY(lig_internal_linear_create(c, sys, kinds, rows, &L));
    return linear_form_once(c, L, key32, rands_dev, const_sum, "lig_linear_form");
}

extern "C" int lig_linear_prepare(lig_ctx* c, const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, lig_linear_program** out) {
    CHECK_CTX(c);
    if (!out) return LIG_E_ARG;
    return lig_internal_linear_prepare(c, sys, kinds, rows, out);
}
extern "C" void lig_linear_program_release(lig_linear_program* p) { linear_program_release(p); }
extern "C" int lig_linear_program_bytes(const lig_linear_program* p, uint64_t* program_bytes, uint64_t* attachment_bytes) {
    if (!p || !program_bytes || !attachment_bytes) return LIG_E_ARG;
    *program_bytes = p->dev_bytes;
    *attachment_bytes = linear_r_bytes(p) + linear_part_bytes(p);
    return LIG_OK;
}
extern "C" int lig_linear_program_form(lig_ctx* c, const lig_linear_program* p, const uint8_t key32[32], const uint8_t* coefs, uint64_t n_coefs, void* rands_dev,
                                       uint8_t const_sum[32]) {
    CHECK_CTX(c);
    if (!p || !key32 || !const_sum || (p->rows && !rands_dev)) return LIG_E_ARG;
    if (p->sharded || c->device != p->device || c->l != p->l || c->k != p->k) FAIL(c, LIG_E_ARG, "lig_linear_program_form: the program was prepared for another device or another (l, k)");
    if (coefs && n_coefs != p->n_coefs) FAIL(c, LIG_E_ARG, "lig_linear_program_form: n_coefs differs from the program's");
    lig_linear* L = nullptr;
    TRY(lig_internal_linear_attach(c, p, &L));
    const int rc = lig_internal_linear_set_values(c, L, coefs, n_coefs, c->stream);
    if (rc != LIG_OK) { const std::string why = c->err; lig_internal_linear_destroy(L); c->err = why; return rc; }
    return linear_form_once(c, L, key32, rands_dev, const_sum, "lig_linear_program_form");
}
