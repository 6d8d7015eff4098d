// derive.hip -- derived slots: the outputs of linear constraints formed on the device (lig_derived_check, lig_rows_set_derived; lig_hip.h).
//
// Upstream every backend.eval(expr) creates a new witness w[t] that one linear constraint ties to older witnesses, with coefficient -1
// (include/zkp/backend/core.hpp:311).  A caller that has recorded its term list marks that constraint as the DEFINING constraint of t; the
// library then forms w[t] from the other terms of the constraint instead of reading it from the caller's row.  The linear counterpart of
// k_expand_product (expand.hip).
//
//   host    derive_plan.hpp checks the list and orders it in waves (a slot derived from derived slots belongs to a later wave); the program
//           -- targets, their other terms, the coefficient table -- is copied to the device once per lig_rows_set_derived, the table
//           converted to Montgomery form there (k_lin_coefs_mont, linear.hip)
//   device  k_derive_wave, one launch per wave on the encode stream of stage 1 (prover.hip), after every row of the trace is expanded and
//           before the first encode:
//             light targets (at most DERIVE_LANE_MAX = 64 other terms): one lane each walks its terms over the expanded message matrix --
//               the walk of k_diag_lin (lin_eval.hpp, shared, not copied); the specials +1 / -1 take no multiplication
//             heavy targets (more terms): one workgroup each strides the terms and adds the lanes' sums with the fixed LDS tree of
//               k_diag_lin_heavy
//           then b - sum or sum - b, canonical, two 16-byte stores into the matrix.  A target reads only slots that are not derived or
//           belong to an earlier wave (launch order on one stream), never a slot written by its own launch.  No atomic on a field
//           element: the same bytes on every run.  Every index the kernel uses was checked on the host (lig_linear_check, plan_derived).
//           PRODUCT entries ({slot, LIG_DERIVED_PRODUCT}: column i of a LIG_ELEM_PRODUCT row whose operand x_i or y_i is itself derived, or
//           whose operand row carries records): k_derive_products, a second launch of the wave, one lane per entry -- two 32-byte loads
//           from the matrix, fr_mul, one store over what k_expand_product wrote from the packed sources.  One wave numbering covers both
//           kinds of entry, so t = eval(a + b); u = t * c; v = eval(u + d) is three waves.
//   shard   lig_shard_rows_set_derived: the same list on a trace dealt over the ranks of a node.  plan_derived_shard (derive_plan.hpp) gives
//           a rank the targets on its rows, their terms split into LOCAL ones (slot = local row * l + col of the rank's matrix) and
//           IMPORTED ones (slot = position in the rank's import buffer), and the exchange schedule every rank computes alike.  Per wave,
//           on the main stream of stage 1 (shard.hip): k_derive_export copies the slots other ranks read from the matrix into a send
//           block (zero tail), ONE all-gather appends the ranks' blocks to the import buffer -- both only for a wave in which something
//           crosses ranks -- then k_derive_wave_shard: k_derive_wave with the two sources, the same walk, the same light / heavy split,
//           tree and block cap, the store into the local row.  Exact field addition: the regrouped sum is the one-GPU sum, byte for byte.
//           A product entry is formed by the rank that holds its triple (the deal never splits one) with the same k_derive_products over
//           local rows; it imports nothing, and a re-formed slot another rank reads is exported like any other slot.
#include "derive_plan.hpp"
#include "lin_eval.hpp"
#include "prover_common.hpp"

namespace lig {
static constexpr uint32_t DERIVE_MAX_BLOCKS = COEFS_MAX_BLOCKS;      // block cap of each of the two parts of a wave's grid

static __device__ __forceinline__ void derive_store(const DeriveTarget tg, fr sum, fr* msgs, uint32_t l, uint32_t k, uint64_t l_recip,
                                                    const fr* __restrict__ coef_mont) {
    const fr b = tg.rhs == DERIVE_RHS_ZERO ? fr_zero() : diag_coef_value(tg.rhs, coef_mont);
    const uint32_t row = diag_div(tg.slot, l_recip), col = tg.slot - row * l;
    fr_store(msgs + (size_t)row * k + col, tg.negate ? fr_sub(sum, b) : fr_sub(b, sum));
}
// workgroups [0, light_blocks): lane -> light target (grid-stride); the others: workgroup -> heavy target n_light + h (block-stride)
__global__ void __launch_bounds__(LIN_WG) k_derive_wave(const DeriveTarget* __restrict__ targets, uint32_t n_light, uint32_t n_heavy, uint32_t light_blocks,
                                                        const lig_lin_term* __restrict__ terms, fr* msgs, uint32_t l, uint32_t k, uint64_t l_recip,
                                                        const fr* __restrict__ coef_mont) {
    __shared__ fr sh[LIN_WG];
    if (blockIdx.x < light_blocks) {
        for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n_light; i += (uint64_t)light_blocks * LIN_WG) {
            const DeriveTarget tg = targets[i];
            derive_store(tg, diag_sum_lane(tg.begin, tg.end, terms, msgs, l, k, l_recip, coef_mont, DiagAllRows{}), msgs, l, k, l_recip, coef_mont);
        }
        return;
    }
    const uint32_t heavy_blocks = gridDim.x - light_blocks;
    for (uint32_t h = blockIdx.x - light_blocks; h < n_heavy; h += heavy_blocks) {      // (uniform over the workgroup: the barriers of lin_block_sum are reached by all lanes)
        const DeriveTarget tg = targets[n_light + h];
        const fr sum = diag_sum_block(tg.begin, tg.end, terms, msgs, l, k, l_recip, coef_mont, DiagAllRows{}, sh);
        if (threadIdx.x == 0) derive_store(tg, sum, msgs, l, k, l_recip, coef_mont);
        __syncthreads();                                                  // sh is reused by the next target
    }
}

// The product entries of a wave ({slot, LIG_DERIVED_PRODUCT}): lane -> entry (grid-stride), column `col` of the LIG_ELEM_PRODUCT row `row`
// = w[row - 2][col] * w[row - 1][col], both read from the expanded matrix -- so the records of a mixed operand row and an operand derived
// in an earlier wave are seen -- and multiplied as k_expand_product multiplies full-width operands (fr_mul: plain x plain -> plain,
// canonical).  A launch of its own next to the wave's k_derive_wave: an operand is a slot of an earlier wave or not listed, and the slot
// written is read by later waves only, so neither launch of a wave reads what the other writes.  One GPU and a rank of a shard alike (rows
// of the matrix in hand: the deal never splits a triple).
__global__ void __launch_bounds__(LIN_WG) k_derive_products(const DeriveProduct* __restrict__ products, uint32_t n, fr* msgs, uint32_t k) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LIN_WG) {
        const DeriveProduct pr = products[i];
        fr* const z = msgs + (size_t)pr.row * k + pr.col;
        fr_store(z, fr_mul(fr_load(z - 2 * (size_t)k), fr_load(z - k)));
    }
}
static void launch_derive_products(hipStream_t st, const DeriveProduct* products, uint32_t n, fr* msgs, uint32_t k) {
    if (!n) return;
    hipLaunchKernelGGL(k_derive_products, dim3(std::min((n + LIN_WG - 1) / LIN_WG, DERIVE_MAX_BLOCKS)), dim3(LIN_WG), 0, st, products, n, msgs, k);
}

// ---- a rows shard
// lane i < block: send[i] = the value of the i-th slot of this rank's E(w) (local slot -> row, column of the rank's matrix), zero for i >= n
__global__ void __launch_bounds__(LIN_WG) k_derive_export(const uint32_t* __restrict__ slots, uint32_t n, uint32_t block, const fr* __restrict__ msgs, uint32_t l, uint32_t k,
                                                          uint64_t l_recip, fr* __restrict__ send) {
    for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < block; i += (uint64_t)gridDim.x * LIN_WG) {
        fr v = fr_zero();
        if (i < n) {
            const uint32_t slot = slots[i], row = diag_div(slot, l_recip), col = slot - row * l;
            v = fr_load(msgs + (size_t)row * k + col);
        }
        fr_store(send + i, v);
    }
}
static __device__ __forceinline__ void derive_store_shard(const DeriveShardTarget tg, fr sum, fr* msgs, uint32_t k, const fr* __restrict__ coef_mont) {
    const fr b = tg.rhs == DERIVE_RHS_ZERO ? fr_zero() : diag_coef_value(tg.rhs, coef_mont);
    fr_store(msgs + (size_t)tg.row * k + tg.col, tg.negate ? fr_sub(sum, b) : fr_sub(b, sum));
}
// k_derive_wave over a rank's share: terms [begin, mid) from the rank's matrix, [mid, end) from its import buffer
__global__ void __launch_bounds__(LIN_WG) k_derive_wave_shard(const DeriveShardTarget* __restrict__ targets, uint32_t n_light, uint32_t n_heavy, uint32_t light_blocks,
                                                              const lig_lin_term* __restrict__ terms, fr* msgs, const fr* __restrict__ imported, uint32_t l, uint32_t k,
                                                              uint64_t l_recip, const fr* __restrict__ coef_mont) {
    __shared__ fr sh[LIN_WG];
    if (blockIdx.x < light_blocks) {
        for (uint64_t i = (uint64_t)blockIdx.x * LIN_WG + threadIdx.x; i < n_light; i += (uint64_t)light_blocks * LIN_WG) {
            const DeriveShardTarget tg = targets[i];
            const fr own = diag_walk(fr_zero(), tg.begin, tg.mid, 1, terms, msgs, l, k, l_recip, coef_mont, DiagAllRows{});
            derive_store_shard(tg, diag_walk(own, tg.mid, tg.end, 1, terms, imported, l, k, l_recip, coef_mont, DiagFlat{}), msgs, k, coef_mont);
        }
        return;
    }
    const uint32_t heavy_blocks = gridDim.x - light_blocks;
    for (uint32_t h = blockIdx.x - light_blocks; h < n_heavy; h += heavy_blocks) {      // (uniform over the workgroup, as in k_derive_wave)
        const DeriveShardTarget tg = targets[n_light + h];
        const fr own = diag_walk(fr_zero(), tg.begin + threadIdx.x, tg.mid, LIN_WG, terms, msgs, l, k, l_recip, coef_mont, DiagAllRows{});
        const fr sum = lin_block_sum(diag_walk(own, tg.mid + threadIdx.x, tg.end, LIN_WG, terms, imported, l, k, l_recip, coef_mont, DiagFlat{}), sh);
        if (threadIdx.x == 0) derive_store_shard(tg, sum, msgs, k, coef_mont);
        __syncthreads();                                                  // sh is reused by the next target
    }
}
}  // namespace lig

// the program of one lig_rows_set_derived on the device; nothing writes it after the call has returned
struct lig_derive {
    int device = 0;
    std::vector<uint32_t> wave_begin, wave_light, prod_begin;
    lig::DeriveTarget* targets = nullptr;
    lig::DeriveProduct* products = nullptr;
    lig_lin_term* terms = nullptr;
    fr* coef_mont = nullptr;
};

static void derived_info_fill(lig_derived_info* info, const lig::DerivePlan& p, uint64_t n) {
    if (!info) return;
    const uint32_t struct_bytes = info->struct_bytes;
    std::memset(info, 0, sizeof *info);
    info->struct_bytes = struct_bytes;
    info->n_slots = n;
    info->n_terms = p.n_terms();
    info->n_waves = p.n_waves;
}

extern "C" int lig_derived_check(const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, uint32_t l, const uint8_t* elem_bytes,
                                 const lig_derived_slot* d, uint64_t n, uint32_t* wave_out, lig_derived_info* info) {
    if (info && info->struct_bytes < sizeof(lig_derived_info)) return LIG_E_ARG;
    if (lig_linear_check(sys, kinds, rows, l) != LIG_OK) return LIG_E_ARG;
    lig::DerivePlan p;
    if (lig::plan_derived(*sys, kinds, rows, l, elem_bytes, d, n, p)) return LIG_E_ARG;
    if (wave_out) for (uint64_t i = 0; i < n; i++) wave_out[i] = p.wave_of[i];
    derived_info_fill(info, p, n);
    return LIG_OK;
}

void lig_internal_derive_destroy(lig_derive* D) {
    if (!D) return;
    (void)hipSetDevice(D->device);
    (void)hipFree(D->targets); (void)hipFree(D->products); (void)hipFree(D->terms); (void)hipFree(D->coef_mont);
    delete D;
}

int lig_internal_derive_create(lig_ctx* c, const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, const uint8_t* elem_bytes, const lig_derived_slot* d,
                               uint64_t n, lig_derive** out, lig_derived_info* info) {
    *out = nullptr;
    if (info && info->struct_bytes < sizeof(lig_derived_info)) FAIL(c, LIG_E_ARG, "lig_rows_set_derived: lig_derived_info.struct_bytes too small");
    if (lig_linear_check(sys, kinds, rows, c->l) != LIG_OK) FAIL(c, LIG_E_ARG, "lig_rows_set_derived: linear system rejected by lig_linear_check");
    lig::DerivePlan p;
    if (const char* why = lig::plan_derived(*sys, kinds, rows, c->l, elem_bytes, d, n, p)) FAIL(c, LIG_E_ARG, std::string("lig_rows_set_derived: ") + why);
    std::unique_ptr<lig_derive, void (*)(lig_derive*)> D(new lig_derive(), lig_internal_derive_destroy);
    D->device = c->device;
    D->wave_begin = p.wave_begin; D->wave_light = p.wave_light; D->prod_begin = p.prod_begin;
    auto put = [&](void** dev, const void* host, size_t bytes) -> int {      // (blocking copies from pageable memory: the plan goes when this call returns)
        const hipError_t e = hipMalloc(dev, bytes ? bytes : 16);
        if (e != hipSuccess) { (void)hipGetLastError(); FAIL(c, LIG_E_NOMEM, std::string("lig_rows_set_derived: ") + hipGetErrorString(e)); }
        if (bytes) HIP_TRY(c, hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
        return LIG_OK;
    };
    TRY(put((void**)&D->targets, p.targets.data(), p.targets.size() * sizeof(lig::DeriveTarget)));
    TRY(put((void**)&D->products, p.products.data(), p.products.size() * sizeof(lig::DeriveProduct)));
    TRY(put((void**)&D->terms, p.terms.data(), p.terms.size() * sizeof(lig_lin_term)));
    TRY(put((void**)&D->coef_mont, p.coefs.data(), p.coefs.size()));
    lig::launch_lin_coefs_mont(c->stream, D->coef_mont, p.coefs.size() / 32);      // once per call; the waves run on the same stream
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    derived_info_fill(info, p, n);
    *out = D.release();
    return LIG_OK;
}

// the waves, in order, on `st`: msgs = the expanded rows x k matrix of the commit in progress
int lig_internal_derive_run(lig_ctx* c, const lig_derive* D, fr* msgs, hipStream_t st) {
    const uint64_t l_recip = lig::lin_reciprocal(c->l);
    for (size_t w = 0; w + 1 < D->wave_begin.size(); w++) {
        const uint32_t first = D->wave_begin[w], n_all = D->wave_begin[w + 1] - first, n_light = D->wave_light[w], n_heavy = n_all - n_light;
        const uint32_t light_blocks = std::min((n_light + lig::LIN_WG - 1) / lig::LIN_WG, lig::DERIVE_MAX_BLOCKS), heavy_blocks = std::min(n_heavy, lig::DERIVE_MAX_BLOCKS);
        if (light_blocks + heavy_blocks)
            hipLaunchKernelGGL(lig::k_derive_wave, dim3(light_blocks + heavy_blocks), dim3(lig::LIN_WG), 0, st, D->targets + first, n_light, n_heavy, light_blocks,
                               D->terms, msgs, c->l, c->k, l_recip, D->coef_mont);
        lig::launch_derive_products(st, D->products + D->prod_begin[w], D->prod_begin[w + 1] - D->prod_begin[w], msgs, c->k);
    }
    HIP_TRY(c, hipGetLastError());
    return LIG_OK;
}

// ---- a rows shard: one rank's program of lig_shard_rows_set_derived; nothing writes it after the call has returned
struct lig_derive_shard {
    int device = 0;
    std::vector<uint32_t> wave_begin, wave_light, prod_begin, block, import_begin, export_begin;
    lig::DeriveShardTarget* targets = nullptr;
    lig::DeriveProduct* products = nullptr;
    lig_lin_term* terms = nullptr;
    uint32_t* exports = nullptr;
    fr* coef_mont = nullptr;
};

static void derived_shard_info_fill(lig_derived_shard_info* info, const lig::DerivePlan& p, const lig::DeriveShardPlan& sp, uint64_t n) {
    if (!info) return;
    const uint32_t struct_bytes = info->struct_bytes;
    std::memset(info, 0, sizeof *info);
    info->struct_bytes = struct_bytes;
    info->n_slots = n;
    info->n_terms = p.n_terms();
    info->n_waves = p.n_waves;
    info->n_exchanges = sp.n_exchanges;
    info->local_targets = sp.local_targets();
    info->local_terms = sp.local_terms;
    info->imported_terms = sp.imported_terms;
    info->imports = sp.n_imports;
    info->exports = sp.n_exports;
    info->exchange_bytes = 32 * sp.import_elems();      // world * sum_w B(w) elements
}
// why a list is refused on a shard (nullptr: accepted, p and sp are the plans); owner: the rank of every row of the whole trace
static const char* derive_shard_plan(const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, uint32_t l, const uint8_t* elem_bytes, const lig_derived_slot* d,
                                     uint64_t n, const std::vector<uint32_t>& owner, uint32_t rank, uint32_t world, lig::DerivePlan& p, lig::DeriveShardPlan& sp) {
    if (lig_linear_check(sys, kinds, rows, l) != LIG_OK) return "linear system rejected by lig_linear_check";
    if (const char* why = lig::plan_derived(*sys, kinds, rows, l, elem_bytes, d, n, p)) return why;
    return lig::plan_derived_shard(p, lig::derive_deal_of(owner, world), l, rank, world, sp);
}
int lig_internal_derive_shard_count(const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, uint32_t l, const uint8_t* elem_bytes, const lig_derived_slot* d,
                                    uint64_t n, const std::vector<uint32_t>& owner, uint32_t rank, uint32_t world, lig_derived_shard_info* info) {
    lig::DerivePlan p;
    lig::DeriveShardPlan sp;
    if (derive_shard_plan(sys, kinds, rows, l, elem_bytes, d, n, owner, rank, world, p, sp)) return LIG_E_ARG;
    derived_shard_info_fill(info, p, sp, n);
    return LIG_OK;
}

void lig_internal_derive_shard_destroy(lig_derive_shard* D) {
    if (!D) return;
    (void)hipSetDevice(D->device);
    (void)hipFree(D->targets); (void)hipFree(D->products); (void)hipFree(D->terms); (void)hipFree(D->exports); (void)hipFree(D->coef_mont);
    delete D;
}

int lig_internal_derive_shard_create(lig_ctx* c, const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, const uint8_t* elem_bytes, const lig_derived_slot* d,
                                     uint64_t n, const std::vector<uint32_t>& owner, uint32_t rank, uint32_t world, lig_derive_shard** out, uint64_t* send_elems,
                                     uint64_t* import_elems, lig_derived_shard_info* info) {
    *out = nullptr;
    lig::DerivePlan p;
    lig::DeriveShardPlan sp;
    if (const char* why = derive_shard_plan(sys, kinds, rows, c->l, elem_bytes, d, n, owner, rank, world, p, sp)) FAIL(c, LIG_E_ARG, std::string("lig_shard_rows_set_derived: ") + why);
    std::unique_ptr<lig_derive_shard, void (*)(lig_derive_shard*)> D(new lig_derive_shard(), lig_internal_derive_shard_destroy);
    D->device = c->device;
    D->wave_begin = sp.wave_begin; D->wave_light = sp.wave_light; D->prod_begin = sp.prod_begin; D->block = sp.block; D->import_begin = sp.import_begin; D->export_begin = sp.export_begin;
    auto put = [&](void** dev, const void* host, size_t bytes) -> int {      // (blocking copies from pageable memory: the plan goes when this call returns)
        const hipError_t e = hipMalloc(dev, bytes ? bytes : 16);
        if (e != hipSuccess) { (void)hipGetLastError(); FAIL(c, LIG_E_NOMEM, std::string("lig_shard_rows_set_derived: ") + hipGetErrorString(e)); }
        if (bytes) HIP_TRY(c, hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
        return LIG_OK;
    };
    TRY(put((void**)&D->targets, sp.targets.data(), sp.targets.size() * sizeof(lig::DeriveShardTarget)));
    TRY(put((void**)&D->products, sp.products.data(), sp.products.size() * sizeof(lig::DeriveProduct)));
    TRY(put((void**)&D->terms, sp.terms.data(), sp.terms.size() * sizeof(lig_lin_term)));
    TRY(put((void**)&D->exports, sp.exports.data(), sp.exports.size() * sizeof(uint32_t)));
    TRY(put((void**)&D->coef_mont, p.coefs.data(), p.coefs.size()));
    lig::launch_lin_coefs_mont(c->stream, D->coef_mont, p.coefs.size() / 32);      // once per call; the waves run on the same stream
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *send_elems = 0;
    for (const uint32_t b : sp.block) *send_elems = std::max<uint64_t>(*send_elems, b);
    *import_elems = sp.import_elems();
    derived_shard_info_fill(info, p, sp, n);
    *out = D.release();
    return LIG_OK;
}

// the waves of one commit, in order, on `st`: msgs = the rank's expanded local rows x k matrix; send (>= max B(w) elements) and imported
// (>= world * sum B(w)) belong to the shard; all_gather(src, dst, bytes per rank) is the shard's (stream-ordered on st, or drained)
int lig_internal_derive_shard_run(lig_ctx* c, const lig_derive_shard* D, fr* msgs, fr* send, fr* imported, hipStream_t st,
                                  const std::function<int(const void*, void*, size_t, const char*)>& all_gather) {
    const uint64_t l_recip = lig::lin_reciprocal(c->l);
    for (size_t w = 0; w + 1 < D->wave_begin.size(); w++) {
        if (const uint32_t B = D->block[w]) {
            const uint32_t n_out = D->export_begin[w + 1] - D->export_begin[w];
            hipLaunchKernelGGL(lig::k_derive_export, dim3(std::min((B + lig::LIN_WG - 1) / lig::LIN_WG, lig::DERIVE_MAX_BLOCKS)), dim3(lig::LIN_WG), 0, st,
                               D->exports + D->export_begin[w], n_out, B, msgs, c->l, c->k, l_recip, send);
            HIP_TRY(c, hipGetLastError());
            TRY(all_gather(send, imported + D->import_begin[w], (size_t)B * 32, "all_gather(derived slots)"));
        }
        const uint32_t first = D->wave_begin[w], n_all = D->wave_begin[w + 1] - first, n_light = D->wave_light[w], n_heavy = n_all - n_light;
        const uint32_t light_blocks = std::min((n_light + lig::LIN_WG - 1) / lig::LIN_WG, lig::DERIVE_MAX_BLOCKS), heavy_blocks = std::min(n_heavy, lig::DERIVE_MAX_BLOCKS);
        if (light_blocks + heavy_blocks)
            hipLaunchKernelGGL(lig::k_derive_wave_shard, dim3(light_blocks + heavy_blocks), dim3(lig::LIN_WG), 0, st, D->targets + first, n_light, n_heavy, light_blocks,
                               D->terms, msgs, imported, c->l, c->k, l_recip, D->coef_mont);
        lig::launch_derive_products(st, D->products + D->prod_begin[w], D->prod_begin[w + 1] - D->prod_begin[w], msgs, c->k);
    }
    HIP_TRY(c, hipGetLastError());
    return LIG_OK;
}
