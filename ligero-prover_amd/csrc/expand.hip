// expand.hip -- caller rows in the narrow format (lig_rows_job.elem_bytes) -> full-width message rows, on the device.
//
// One kernel for every width of a chunk: bits (LIG_ELEM_BIT), 1-, 2-, 4- and 8-byte little-endian integers, and full 32-byte
// rows.  It sits on the encode stream in front of K1 (stage 1 of lig_rows_commit, lig_rows_restart with device rows, the sharded
// load), so it is write-bound by construction: the row and its width are uniform per workgroup (the row is grid.y), each lane
// produces one 32-byte element with two 16-byte stores, a bit row reads one dword per 32 slots, and no lane divides.
//
// A sibling kernel forms the DERIVED rows of a chunk (LIG_ELEM_PRODUCT: the z row of a quadratic triple, no bytes in the packed
// matrix): slot i < l = x[i] * y[i] mod p, the operands read from the PACKED sources of the two preceding rows -- never from
// the expanded matrix, so a derived row depends on no other workgroup of the launch and on no other launch.
//
// MIXED rows (lig_rows_job.wide_per_row): a narrow row followed by c records {uint32 column, 8 uint32 limbs}.  k_expand_narrow writes
// the narrow part as ever; k_expand_wide, directly behind it on the same stream, overwrites the c named slots, one lane per record.
// k_expand_product looks an operand slot up among the records of its operand row (binary search, the columns are ascending).
#include "prover_common.hpp"

namespace lig {
static constexpr uint32_t EXPAND_WG = 256;

// element i < l of a narrow row whose packed bytes start at `src` (4-byte aligned): the low 64 bits of the canonical value
static __device__ __forceinline__ uint2 narrow_slot(const uint8_t* __restrict__ src, uint32_t w, uint32_t i) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(src);
    switch (w) {
        case LIG_ELEM_BIT: return make_uint2((p[i >> 5] >> (i & 31)) & 1u, 0);
        case 1: return make_uint2((p[i >> 2] >> ((i & 3) * 8)) & 0xffu, 0);
        case 2: return make_uint2((p[i >> 1] >> ((i & 1) * 16)) & 0xffffu, 0);
        case 4: return make_uint2(p[i], 0);
        default: return make_uint2(p[2 * i], p[2 * i + 1]);           // 8
    }
}

// grid = (ceil(k / 256), min(rows, 65535)): workgroup (x, y) writes slots [256 x, 256 x + 256) of rows y, y + gridDim.y, ...
__global__ void __launch_bounds__(EXPAND_WG) k_expand_narrow(const uint8_t* __restrict__ packed, const uint64_t* __restrict__ off,
                                                             const uint8_t* __restrict__ widths, size_t first_row, uint32_t rows,
                                                             uint32_t l, uint32_t k, fr* __restrict__ out) {
    const uint32_t i = blockIdx.x * EXPAND_WG + threadIdx.x;
    if (i >= k) return;
    for (uint32_t rr = blockIdx.y; rr < rows; rr += gridDim.y) {
        const size_t r = first_row + rr;
        const uint32_t w = widths[r];
        if (w == LIG_ELEM_PRODUCT) continue;                          // a derived row: k_expand_product
        const uint8_t* src = packed + off[r];
        uint4* dst = reinterpret_cast<uint4*>(out + r * k + i);
        if (w == 32) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(src) + (size_t)i * 8;   // 4-byte aligned only: dword loads
            dst[0] = make_uint4(p[0], p[1], p[2], p[3]);
            dst[1] = make_uint4(p[4], p[5], p[6], p[7]);
        } else {
            const uint2 v = i < l ? narrow_slot(src, w, i) : make_uint2(0, 0);           // slots l..k-1: zero, their pads follow
            dst[0] = make_uint4(v.x, v.y, 0, 0);
            dst[1] = make_uint4(0, 0, 0, 0);
        }
    }
}

// element i < l of an operand row of any width (bits, 1, 2, 4, 8, 32) as a full field element
static __device__ __forceinline__ fr operand_slot(const uint8_t* __restrict__ src, uint32_t w, uint32_t i) {
    fr a;
    if (w == 32) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(src) + (size_t)i * 8;
#pragma unroll
        for (int j = 0; j < 8; j++) a.v[j] = p[j];
    } else {
        const uint2 v = narrow_slot(src, w, i);
        a = fr_zero();
        a.v[0] = v.x; a.v[1] = v.y;
    }
    return a;
}

// the c records of mixed row r end where the packed bytes of row r end (rows_plan.hpp): record j, as dwords (the packed area is only
// 4-byte aligned)
static __device__ __forceinline__ const uint32_t* wide_record(const uint8_t* __restrict__ packed, const uint64_t* __restrict__ off, size_t r,
                                                              uint32_t c, uint32_t j) {
    return reinterpret_cast<const uint32_t*>(packed + off[r + 1]) - (size_t)(c - j) * (LIG_WIDE_RECORD_BYTES / 4);
}

// The records of the mixed rows mixed_rows[0 .. rows) (row indices of the matrix; wide[r] = the records of row r) over the slots
// k_expand_narrow has written: grid = (ceil(max records / 256), min(rows, 65535)), lane j of workgroup column x = record
// 256 x + j of rows y, y + gridDim.y, ...  A record whose column is >= l (device rows: the host has not seen it) writes nothing
// and raises *flag.  Two records of one row naming the same column: one of the two values, inside the row either way.
__global__ void __launch_bounds__(EXPAND_WG) k_expand_wide(const uint8_t* __restrict__ packed, const uint64_t* __restrict__ off,
                                                           const uint32_t* __restrict__ mixed_rows, const uint32_t* __restrict__ wide,
                                                           uint32_t rows, uint32_t l, uint32_t k, fr* __restrict__ out, uint32_t* __restrict__ flag) {
    const uint32_t j = blockIdx.x * EXPAND_WG + threadIdx.x;
    for (uint32_t rr = blockIdx.y; rr < rows; rr += gridDim.y) {
        const size_t r = mixed_rows[rr];
        const uint32_t c = wide[r];
        if (j >= c) continue;
        const uint32_t* p = wide_record(packed, off, r, c, j);
        const uint32_t col = p[0];
        if (col >= l) { atomicOr(flag, 1u); continue; }
        uint4* dst = reinterpret_cast<uint4*>(out + r * k + col);
        dst[0] = make_uint4(p[1], p[2], p[3], p[4]);
        dst[1] = make_uint4(p[5], p[6], p[7], p[8]);
    }
}

// the record of mixed row r that names column i -> *v, true; false: none does.  Binary search over the ascending columns; over
// columns in any other order (device rows) it still ends after log2(c) steps and reads records of this row only.
static __device__ __forceinline__ bool wide_find(const uint8_t* __restrict__ packed, const uint64_t* __restrict__ off, size_t r, uint32_t c,
                                                 uint32_t i, fr* v) {
    const uint32_t* recs = wide_record(packed, off, r, c, 0);
    uint32_t lo = 0, hi = c;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (recs[(size_t)mid * 9] < i) lo = mid + 1; else hi = mid;
    }
    if (lo >= c || recs[(size_t)lo * 9] != i) return false;
#pragma unroll
    for (int q = 0; q < 8; q++) v->v[q] = recs[(size_t)lo * 9 + 1 + q];
    return true;
}

// The derived rows prod_rows[0 .. rows) (row indices of the matrix, each the z of a triple: its x is row r - 2, its y row r - 1).
// grid = (ceil(k / 256), min(rows, 65535)) as above.  Two wave-uniform paths: both operands at most 8 bytes wide -> the plain
// 64 x 64 -> 128-bit product (< 2^128 < p: canonical as it stands); otherwise fr_mul.  Slots l..k-1: zero, their pads follow.
// MIXED (the matrix has mixed rows; wide[r] = the records of row r): an operand row with records is searched for a record naming
// slot i -- a row-uniform branch; where neither operand has one the two paths above are taken unchanged, otherwise fr_mul.
template <bool MIXED>
__global__ void __launch_bounds__(EXPAND_WG) k_expand_product(const uint8_t* __restrict__ packed, const uint64_t* __restrict__ off,
                                                              const uint8_t* __restrict__ widths, const uint32_t* __restrict__ prod_rows,
                                                              uint32_t rows, uint32_t l, uint32_t k, fr* __restrict__ out,
                                                              const uint32_t* __restrict__ wide) {
    const uint32_t i = blockIdx.x * EXPAND_WG + threadIdx.x;
    if (i >= k) return;
    for (uint32_t rr = blockIdx.y; rr < rows; rr += gridDim.y) {
        const size_t r = prod_rows[rr];
        const uint32_t wx = widths[r - 2], wy = widths[r - 1];
        const uint8_t* sx = packed + off[r - 2];
        const uint8_t* sy = packed + off[r - 1];
        uint4* dst = reinterpret_cast<uint4*>(out + r * k + i);
        if (i >= l) {
            dst[0] = make_uint4(0, 0, 0, 0);
            dst[1] = make_uint4(0, 0, 0, 0);
            continue;
        }
        fr x, y;
        bool hx = false, hy = false;                                  // a record names slot i of the operand row
        if (MIXED) {
            const uint32_t cx = wide[r - 2], cy = wide[r - 1];
            hx = cx && wide_find(packed, off, r - 2, cx, i, &x);
            hy = cy && wide_find(packed, off, r - 1, cy, i, &y);
        }
        if (!hx && !hy && wx != 32 && wy != 32) {
            const uint2 a2 = narrow_slot(sx, wx, i), b2 = narrow_slot(sy, wy, i);
            const uint64_t a = ((uint64_t)a2.y << 32) | a2.x, b = ((uint64_t)b2.y << 32) | b2.x;
            const uint64_t lo = a * b, hi = __umul64hi(a, b);
            dst[0] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
            dst[1] = make_uint4(0, 0, 0, 0);
        } else {
            if (!hx) x = operand_slot(sx, wx, i);
            if (!hy) y = operand_slot(sy, wy, i);
            fr_store(out + r * k + i, fr_mul(x, y));
        }
    }
}

void launch_expand_rows(hipStream_t s, const uint8_t* packed, const uint64_t* off_dev, const uint8_t* widths_dev, size_t first_row,
                        size_t rows, uint32_t l, uint32_t k, fr* out, const uint32_t* prod_rows_dev, size_t n_prod, const WideArgs& wd) {
    if (!rows) return;
    const dim3 grid((k + EXPAND_WG - 1) / EXPAND_WG, (uint32_t)std::min<size_t>(rows, 65535));
    hipLaunchKernelGGL(k_expand_narrow, grid, dim3(EXPAND_WG), 0, s, packed, off_dev, widths_dev, first_row, (uint32_t)rows, l, k, out);
    if (wd.n_mixed) {
        const dim3 wgrid((wd.max_records + EXPAND_WG - 1) / EXPAND_WG, (uint32_t)std::min<size_t>(wd.n_mixed, 65535));
        hipLaunchKernelGGL(k_expand_wide, wgrid, dim3(EXPAND_WG), 0, s, packed, off_dev, wd.mixed_rows_dev, wd.wide_dev, (uint32_t)wd.n_mixed, l, k, out, wd.flag_dev);
    }
    if (!n_prod) return;
    const dim3 pgrid(grid.x, (uint32_t)std::min<size_t>(n_prod, 65535));
    if (wd.wide_dev) hipLaunchKernelGGL(k_expand_product<true>, pgrid, dim3(EXPAND_WG), 0, s, packed, off_dev, widths_dev, prod_rows_dev, (uint32_t)n_prod, l, k, out, wd.wide_dev);
    else hipLaunchKernelGGL(k_expand_product<false>, pgrid, dim3(EXPAND_WG), 0, s, packed, off_dev, widths_dev, prod_rows_dev, (uint32_t)n_prod, l, k, out, (const uint32_t*)nullptr);
}
}  // namespace lig

int lig_internal_upload_narrow_plan(lig_ctx* c, const lig::NarrowPlan& plan, uint64_t** src_off_dev, uint8_t** widths_dev, ProductRows* prod, WideRows* wide) {
    HIP_TRY(c, hipMalloc((void**)src_off_dev, plan.src_off.size() * sizeof(uint64_t)));
    HIP_TRY(c, hipMalloc((void**)widths_dev, plan.widths.size()));
    HIP_TRY(c, hipMemcpy(*src_off_dev, plan.src_off.data(), plan.src_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(*widths_dev, plan.widths.data(), plan.widths.size(), hipMemcpyHostToDevice));
    prod->rows = plan.prod_rows;
    if (!prod->rows.empty()) {
        HIP_TRY(c, hipMalloc((void**)&prod->dev, prod->rows.size() * sizeof(uint32_t)));
        HIP_TRY(c, hipMemcpy(prod->dev, prod->rows.data(), prod->rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    wide->mixed.rows = plan.mixed_rows;
    wide->wide = plan.wide;
    if (wide->mixed.rows.empty()) return LIG_OK;
    wide->max_records = *std::max_element(wide->wide.begin(), wide->wide.end());
    HIP_TRY(c, hipMalloc((void**)&wide->mixed.dev, wide->mixed.rows.size() * sizeof(uint32_t)));
    HIP_TRY(c, hipMalloc((void**)&wide->wide_dev, wide->wide.size() * sizeof(uint32_t)));
    HIP_TRY(c, hipMalloc((void**)&wide->flag_dev, sizeof(uint32_t)));
    HIP_TRY(c, hipMemcpy(wide->mixed.dev, wide->mixed.rows.data(), wide->mixed.rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(wide->wide_dev, wide->wide.data(), wide->wide.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemset(wide->flag_dev, 0, sizeof(uint32_t)));
    return LIG_OK;
}
