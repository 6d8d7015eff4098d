// diagnose.hip -- which constraints of a rows job does the committed witness violate?  (lig_rows_diagnose, include/lig_hip.h)
//
// The prover's self-check answers with one bit per test (valid_linear, valid_quad), computed from a random combination.  This pass
// evaluates the statement itself on the committed witness matrix, exactly and without randomness, and returns the violated constraints:
//   k_diag_lin         one lane per linear constraint with at most HEAVY_MIN terms: walks the caller's constraint-major term list
//                      (the slot-major regrouping of a lig_linear_program is of no use here: per-constraint sums over it would need
//                      256-bit atomics), gathers w[slot] (32 bytes, random), adds / subtracts it or multiplies it by a table
//                      coefficient first (Montgomery copy of the table: one product per such term), subtracts b_c
//   k_diag_lin_heavy   one workgroup per constraint with more terms: lanes stride the segment, fixed LDS tree (lin_block_sum)
//   k_diag_quad        one lane per (quadratic term, column < l): x * y - z, b * b - b for a bit row, x - z for an equality pair
// Every lane writes its canonical residual and a 32-bit flag; the flags go through an exclusive scan (rocPRIM) and the first `cap`
// violated items are scattered into a record array in ascending order -- no atomic decides an order or a count, the output is the same
// bytes on every run.  The quadratic items (terms x l) are processed in slices of a fixed scratch budget; the running count and the
// output offset are carried on the host.  Like the form pass of linear.hip these passes are bound by the 32-byte gathers, not by VALU:
// canonical 8 x u32 arithmetic (fr.hpp).
// Everything is allocated inside the call and freed before it returns (off the proving path); all work is ENQUEUED on the context's
// main stream only -- the side stream, the uploader and the copy stream may be carrying the prefetch of the next trace.  Freeing the
// scratch (hipFree) waits for the whole device, though: with a prefetch in flight the call returns after that transfer (lig_hip.h says so).
#include <rocprim/device/device_scan.hpp>

#include "lin_common.hpp"
#include "prover_common.hpp"

namespace lig {
static constexpr uint32_t DIAG_MAX_BLOCKS = COEFS_MAX_BLOCKS;      // grid-stride passes: at most this many workgroups of LIN_WG lanes
static constexpr uint64_t DIAG_QUAD_ITEMS = 1ull << 20;            // scratch budget of the quadratic pass: (term, column) items per slice (40 bytes each)

// n / d for n < 2^32 and the launch-uniform d >= 1: m = floor(2^64 / d) + 1 (host: diag_reciprocal), exact because n * (m d - 2^64) < 2^64
static __device__ __forceinline__ uint32_t diag_div(uint32_t n, uint64_t m) { return (uint32_t)__umul64hi((uint64_t)n, m); }

static __device__ __forceinline__ fr diag_one() {
    fr o = fr_zero();
    o.v[0] = 1;
    return o;
}
// acc (canonical) += coef * w[slot] for one term
static __device__ __forceinline__ fr diag_accumulate(const fr& acc, const lig_lin_term tm, const fr* __restrict__ msgs, uint32_t l, uint32_t k, uint64_t l_recip,
                                                     const fr* __restrict__ coef_mont) {
    const uint32_t row = diag_div(tm.slot, l_recip), col = tm.slot - row * l;
    const fr w = fr_load(msgs + (size_t)row * k + col);
    if (tm.coef == LIG_COEF_ONE) return fr_add(acc, w);
    if (tm.coef == LIG_COEF_NEG_ONE) return fr_sub(acc, w);
    return fr_add(acc, fr_montmul(w, fr_load(coef_mont + tm.coef)));      // w * (a R) / R = a * w, canonical
}
// the canonical value a coefficient index stands for
static __device__ __forceinline__ fr diag_coef_value(uint32_t coef, const fr* __restrict__ coef_mont) {
    if (coef == LIG_COEF_ONE) return diag_one();
    if (coef == LIG_COEF_NEG_ONE) return fr_neg(diag_one());
    return fr_montmul(fr_load(coef_mont + coef), diag_one());             // (a R) * 1 / R = a
}
// acc - b_c -> residual and flag of constraint c; rhs_index[c] = 1 + the position of c in the right-hand-side list, 0: b_c = 0
static __device__ __forceinline__ void diag_finish(uint32_t c, fr acc, const uint32_t* __restrict__ rhs_index, const uint32_t* __restrict__ rhs_coef,
                                                   const fr* __restrict__ coef_mont, fr* __restrict__ res, uint32_t* __restrict__ flag) {
    const uint32_t ri = rhs_index[c];
    if (ri) acc = fr_sub(acc, diag_coef_value(rhs_coef[ri - 1], coef_mont));
    fr_store(res + c, acc);
    flag[c] = fr_is_zero(acc) ? 0u : 1u;
}

// rhs_constraint is strictly ascending: every entry of rhs_index is written at most once
__global__ void __launch_bounds__(LIN_WG) k_diag_rhs_index(const uint32_t* __restrict__ rhs_c, uint32_t n_rhs, uint32_t* __restrict__ rhs_index) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n_rhs; i += (uint64_t)gridDim.x * LIN_WG) rhs_index[rhs_c[i]] = (uint32_t)i + 1;
}
__global__ void __launch_bounds__(LIN_WG) k_diag_lin(const uint32_t* __restrict__ term_begin, const lig_lin_term* __restrict__ terms, uint32_t n_constraints,
                                                     const fr* __restrict__ msgs, uint32_t l, uint32_t k, uint64_t l_recip, const fr* __restrict__ coef_mont,
                                                     const uint32_t* __restrict__ rhs_index, const uint32_t* __restrict__ rhs_coef, fr* __restrict__ res,
                                                     uint32_t* __restrict__ flag) {
    for (uint64_t c = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; c < n_constraints; c += (uint64_t)gridDim.x * LIN_WG) {
        const uint32_t b = term_begin[c], e = term_begin[c + 1];
        if (e - b > HEAVY_MIN) continue;                                  // k_diag_lin_heavy
        fr acc = fr_zero();
        for (uint32_t t = b; t < e; t++) acc = diag_accumulate(acc, terms[t], msgs, l, k, l_recip, coef_mont);
        diag_finish((uint32_t)c, acc, rhs_index, rhs_coef, coef_mont, res, flag);
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
        fr acc = fr_zero();
        for (uint32_t t = b + threadIdx.x; t < e; t += LIN_WG) acc = diag_accumulate(acc, terms[t], msgs, l, k, l_recip, coef_mont);
        acc = lin_block_sum(acc, sh);
        if (threadIdx.x == 0) diag_finish(c, acc, rhs_index, rhs_coef, coef_mont, res, flag);
        __syncthreads();                                                  // sh is reused by the next constraint
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
// the violated items with a position below `cap` -> records, in ascending order (pos = exclusive scan of flag)
__global__ void __launch_bounds__(LIN_WG) k_diag_scatter_lin(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, const fr* __restrict__ res,
                                                             uint32_t n, uint32_t cap, lig_diag_linear* __restrict__ out) {
    for (uint64_t c = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; c < n; c += (uint64_t)gridDim.x * LIN_WG) {
        if (!flag[c] || pos[c] >= cap) continue;
        lig_diag_linear rec;
        rec.constraint = (uint32_t)c; rec.reserved = 0;
        const fr r = fr_load(res + c);
        for (int w = 0; w < 8; w++) for (int b = 0; b < 4; b++) rec.residual[4 * w + b] = (uint8_t)(r.v[w] >> (8 * b));
        out[pos[c]] = rec;
    }
}
__global__ void __launch_bounds__(LIN_WG) k_diag_scatter_quad(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, const fr* __restrict__ res,
                                                              const uint32_t* __restrict__ tri, uint32_t first_term, uint32_t n_items, uint32_t l, uint64_t l_recip,
                                                              uint32_t cap, lig_diag_quad* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n_items; i += (uint64_t)gridDim.x * LIN_WG) {
        if (!flag[i] || pos[i] >= cap) continue;
        const uint32_t t = diag_div((uint32_t)i, l_recip);
        const uint32_t* q = tri + 3 * (size_t)(first_term + t);
        lig_diag_quad rec;
        rec.row_x = q[0]; rec.row_y = q[1]; rec.row_z = q[2]; rec.column = (uint32_t)i - t * l;
        const fr r = fr_load(res + i);
        for (int w = 0; w < 8; w++) for (int b = 0; b < 4; b++) rec.residual[4 * w + b] = (uint8_t)(r.v[w] >> (8 * b));
        out[pos[i]] = rec;
    }
}
}  // namespace lig

namespace {
uint64_t diag_reciprocal(uint32_t d) { return d <= 1 ? ~0ull : ~0ull / d + 1; }       // floor(2^64 / d) + 1 (d = 1 is never used: l >= 2)
uint32_t diag_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + lig::LIN_WG - 1) / lig::LIN_WG, 1), lig::DIAG_MAX_BLOCKS); }

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
    int alloc(void** p, size_t bytes) {
        *p = nullptr;
        const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
        if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string("lig_rows_diagnose: scratch: ") + hipGetErrorString(e); return LIG_E_NOMEM; }
        bufs.push_back(*p);
        return LIG_OK;
    }
};

// flag[0 .. n] (flag[n] = 0) -> pos[0 .. n] = exclusive scan; *count = pos[n] = the number of set flags.  Blocks until it is known.
int diag_scan(lig_ctx* c, DiagScratch& sc, const uint32_t* flag, uint32_t* pos, size_t n, void** scan_tmp, size_t* scan_cap,
              uint32_t* count) {
    hipStream_t s = c->stream;
    size_t need = 0;
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, need, flag, pos, 0u, n + 1, rocprim::plus<uint32_t>(), s));
    if (need > *scan_cap || !*scan_tmp) { TRY(sc.alloc(scan_tmp, need)); *scan_cap = need; }
    need = *scan_cap;
    HIP_TRY(c, rocprim::exclusive_scan(*scan_tmp, need, flag, pos, 0u, n + 1, rocprim::plus<uint32_t>(), s));
    HIP_TRY(c, hipMemcpyAsync(count, pos + n, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, lig_internal_wait_stream(s));
    return LIG_OK;
}
}  // namespace

// msgs: the committed rows x k witness matrix; tri_dev / n_quad_terms: the quadratic terms of the trace (quad_terms(), rows_plan.hpp); sys (may be NULL) has
// passed lig_linear_check against the trace's kinds.  Waits with lig_internal_wait_stream (prover.hip: bounded spin, then the blocking wait).
int lig_internal_rows_diagnose(lig_ctx* c, const fr* msgs, uint64_t rows, const uint32_t* tri_dev, uint64_t n_quad_terms, const lig_linear_system* sys,
                               lig_diag_linear* lin_out, uint64_t lin_cap, lig_diag_quad* quad_out, uint64_t quad_cap, lig_diag_info* info) {
    hipStream_t s = c->stream;
    const uint32_t l = c->l, k = c->k;
    const uint64_t l_recip = diag_reciprocal(l);
    DiagScratch sc(c);
    void* scan_tmp = nullptr; size_t scan_cap = 0;

    // ---------------------------------------------------------------- linear constraints
    if (sys && sys->n_constraints) {
        const uint32_t NC = (uint32_t)sys->n_constraints, NT = (uint32_t)sys->n_terms, NR = (uint32_t)sys->n_rhs;
        std::vector<uint32_t> heavy;                                      // constraints with more than HEAVY_MIN terms, ascending
        for (uint32_t cn = 0; cn < NC; cn++) if (sys->term_begin[cn + 1] - sys->term_begin[cn] > lig::HEAVY_MIN) heavy.push_back(cn);
        uint32_t *d_tb = nullptr, *d_rhs_c = nullptr, *d_rhs_coef = nullptr, *d_rhs_index = nullptr, *d_heavy = nullptr, *d_flag = nullptr, *d_pos = nullptr;
        lig_lin_term* d_terms = nullptr; fr *d_coef = nullptr, *d_res = nullptr;
        TRY(sc.alloc((void**)&d_tb, ((size_t)NC + 1) * 4));
        TRY(sc.alloc((void**)&d_terms, (size_t)NT * sizeof(lig_lin_term)));
        TRY(sc.alloc((void**)&d_rhs_c, (size_t)NR * 4));
        TRY(sc.alloc((void**)&d_rhs_coef, (size_t)NR * 4));
        TRY(sc.alloc((void**)&d_rhs_index, (size_t)NC * 4));
        TRY(sc.alloc((void**)&d_heavy, heavy.size() * 4));
        TRY(sc.alloc((void**)&d_coef, (size_t)sys->n_coefs * 32));
        TRY(sc.alloc((void**)&d_res, (size_t)NC * 32));
        TRY(sc.alloc((void**)&d_flag, ((size_t)NC + 1) * 4));
        TRY(sc.alloc((void**)&d_pos, ((size_t)NC + 1) * 4));
        HIP_TRY(c, hipMemcpyAsync(d_tb, sys->term_begin, ((size_t)NC + 1) * 4, hipMemcpyHostToDevice, s));
        if (NT) HIP_TRY(c, hipMemcpyAsync(d_terms, sys->terms, (size_t)NT * sizeof(lig_lin_term), hipMemcpyHostToDevice, s));
        if (NR) {
            HIP_TRY(c, hipMemcpyAsync(d_rhs_c, sys->rhs_constraint, (size_t)NR * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipMemcpyAsync(d_rhs_coef, sys->rhs_coef, (size_t)NR * 4, hipMemcpyHostToDevice, s));
        }
        if (!heavy.empty()) HIP_TRY(c, hipMemcpyAsync(d_heavy, heavy.data(), heavy.size() * 4, hipMemcpyHostToDevice, s));
        // a scratch copy of the caller's table in Montgomery form: the table of an attached program is neither read nor written
        if (sys->n_coefs) HIP_TRY(c, hipMemcpyAsync(d_coef, sys->coefs, (size_t)sys->n_coefs * 32, hipMemcpyHostToDevice, s));
        lig::launch_lin_coefs_mont(s, d_coef, sys->n_coefs);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemsetAsync(d_rhs_index, 0, (size_t)NC * 4, s));
        HIP_TRY(c, hipMemsetAsync(d_flag, 0, ((size_t)NC + 1) * 4, s));
        if (NR) {
            hipLaunchKernelGGL(lig::k_diag_rhs_index, dim3(diag_grid(NR)), dim3(lig::LIN_WG), 0, s, d_rhs_c, NR, d_rhs_index);
            HIP_TRY(c, hipGetLastError());
        }
        hipLaunchKernelGGL(lig::k_diag_lin, dim3(diag_grid(NC)), dim3(lig::LIN_WG), 0, s, d_tb, d_terms, NC, msgs, l, k, l_recip, d_coef, d_rhs_index, d_rhs_coef, d_res, d_flag);
        HIP_TRY(c, hipGetLastError());
        if (!heavy.empty()) {
            hipLaunchKernelGGL(lig::k_diag_lin_heavy, dim3(std::min<uint32_t>((uint32_t)heavy.size(), lig::DIAG_MAX_BLOCKS)), dim3(lig::LIN_WG), 0, s, d_heavy,
                               (uint32_t)heavy.size(), d_tb, d_terms, msgs, l, k, l_recip, d_coef, d_rhs_index, d_rhs_coef, d_res, d_flag);
            HIP_TRY(c, hipGetLastError());
        }
        uint32_t bad = 0;
        TRY(diag_scan(c, sc, d_flag, d_pos, NC, &scan_tmp, &scan_cap, &bad));
        if (bad > NC) FAIL(c, LIG_E_STATE, "lig_rows_diagnose: counted more violated constraints than the system holds");
        info->n_linear_bad = bad;
        const uint32_t rep = (uint32_t)std::min<uint64_t>(bad, lin_cap);
        if (rep) {
            lig_diag_linear* d_out = nullptr;
            TRY(sc.alloc((void**)&d_out, (size_t)rep * sizeof(lig_diag_linear)));
            hipLaunchKernelGGL(lig::k_diag_scatter_lin, dim3(diag_grid(NC)), dim3(lig::LIN_WG), 0, s, d_flag, d_pos, d_res, NC, rep, d_out);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemcpyAsync(lin_out, d_out, (size_t)rep * sizeof(lig_diag_linear), hipMemcpyDeviceToHost, s));
            HIP_TRY(c, lig_internal_wait_stream(s));
        }
        info->n_linear_reported = rep;
    }

    // ---------------------------------------------------------------- quadratic terms, in slices of at most DIAG_QUAD_ITEMS items
    if (n_quad_terms && rows) {
        const uint64_t per = std::max<uint64_t>(lig::DIAG_QUAD_ITEMS / l, 1);        // terms per slice: per * l < 2^32 (l < 2^32, and per = 1 beyond the budget)
        const uint64_t slice_items = std::min(per, n_quad_terms) * l;
        uint32_t *d_flag = nullptr, *d_pos = nullptr; fr* d_res = nullptr; lig_diag_quad* d_out = nullptr;
        TRY(sc.alloc((void**)&d_res, (size_t)slice_items * 32));
        TRY(sc.alloc((void**)&d_flag, ((size_t)slice_items + 1) * 4));
        TRY(sc.alloc((void**)&d_pos, ((size_t)slice_items + 1) * 4));
        const uint64_t out_cap = std::min<uint64_t>(quad_cap, slice_items);
        if (out_cap) TRY(sc.alloc((void**)&d_out, (size_t)out_cap * sizeof(lig_diag_quad)));
        uint64_t bad_total = 0, reported = 0;
        for (uint64_t t0 = 0; t0 < n_quad_terms; t0 += per) {
            const uint32_t items = (uint32_t)(std::min(per, n_quad_terms - t0) * l);
            HIP_TRY(c, hipMemsetAsync(d_flag + items, 0, 4, s));
            hipLaunchKernelGGL(lig::k_diag_quad, dim3(diag_grid(items)), dim3(lig::LIN_WG), 0, s, tri_dev, (uint32_t)t0, items, msgs, l, k, l_recip, d_res, d_flag);
            HIP_TRY(c, hipGetLastError());
            uint32_t bad = 0;
            TRY(diag_scan(c, sc, d_flag, d_pos, items, &scan_tmp, &scan_cap, &bad));
            if (bad > items) FAIL(c, LIG_E_STATE, "lig_rows_diagnose: counted more violated items than the slice holds");
            bad_total += bad;
            const uint32_t rep = (uint32_t)std::min<uint64_t>(bad, quad_cap - reported);
            if (rep) {
                hipLaunchKernelGGL(lig::k_diag_scatter_quad, dim3(diag_grid(items)), dim3(lig::LIN_WG), 0, s, d_flag, d_pos, d_res, tri_dev, (uint32_t)t0, items, l, l_recip,
                                   rep, d_out);
                HIP_TRY(c, hipGetLastError());
                HIP_TRY(c, hipMemcpyAsync(quad_out + reported, d_out, (size_t)rep * sizeof(lig_diag_quad), hipMemcpyDeviceToHost, s));
                HIP_TRY(c, lig_internal_wait_stream(s));
                reported += rep;
            }
        }
        info->n_quad_bad = bad_total;
        info->n_quad_reported = reported;
    }
    return LIG_OK;
}
