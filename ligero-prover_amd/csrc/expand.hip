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

// The derived rows prod_rows[0 .. rows) (row indices of the matrix, each the z of a triple: its x is row r - 2, its y row r - 1).
// grid = (ceil(k / 256), min(rows, 65535)) as above.  Two wave-uniform paths: both operands at most 8 bytes wide -> the plain
// 64 x 64 -> 128-bit product (< 2^128 < p: canonical as it stands); otherwise fr_mul.  Slots l..k-1: zero, their pads follow.
__global__ void __launch_bounds__(EXPAND_WG) k_expand_product(const uint8_t* __restrict__ packed, const uint64_t* __restrict__ off,
                                                              const uint8_t* __restrict__ widths, const uint32_t* __restrict__ prod_rows,
                                                              uint32_t rows, uint32_t l, uint32_t k, fr* __restrict__ out) {
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
        } else if (wx != 32 && wy != 32) {
            const uint2 x = narrow_slot(sx, wx, i), y = narrow_slot(sy, wy, i);
            const uint64_t a = ((uint64_t)x.y << 32) | x.x, b = ((uint64_t)y.y << 32) | y.x;
            const uint64_t lo = a * b, hi = __umul64hi(a, b);
            dst[0] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
            dst[1] = make_uint4(0, 0, 0, 0);
        } else {
            fr_store(out + r * k + i, fr_mul(operand_slot(sx, wx, i), operand_slot(sy, wy, i)));
        }
    }
}

void launch_expand_rows(hipStream_t s, const uint8_t* packed, const uint64_t* off_dev, const uint8_t* widths_dev, size_t first_row,
                        size_t rows, uint32_t l, uint32_t k, fr* out, const uint32_t* prod_rows_dev, size_t n_prod) {
    if (!rows) return;
    const dim3 grid((k + EXPAND_WG - 1) / EXPAND_WG, (uint32_t)std::min<size_t>(rows, 65535));
    hipLaunchKernelGGL(k_expand_narrow, grid, dim3(EXPAND_WG), 0, s, packed, off_dev, widths_dev, first_row, (uint32_t)rows, l, k, out);
    if (!n_prod) return;
    const dim3 pgrid(grid.x, (uint32_t)std::min<size_t>(n_prod, 65535));
    hipLaunchKernelGGL(k_expand_product, pgrid, dim3(EXPAND_WG), 0, s, packed, off_dev, widths_dev, prod_rows_dev, (uint32_t)n_prod, l, k, out);
}
}  // namespace lig

int lig_internal_upload_narrow_plan(lig_ctx* c, const lig::NarrowPlan& plan, uint64_t** src_off_dev, uint8_t** widths_dev, ProductRows* prod) {
    HIP_TRY(c, hipMalloc((void**)src_off_dev, plan.src_off.size() * sizeof(uint64_t)));
    HIP_TRY(c, hipMalloc((void**)widths_dev, plan.widths.size()));
    HIP_TRY(c, hipMemcpy(*src_off_dev, plan.src_off.data(), plan.src_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(*widths_dev, plan.widths.data(), plan.widths.size(), hipMemcpyHostToDevice));
    prod->rows = plan.prod_rows;
    if (prod->rows.empty()) return LIG_OK;
    HIP_TRY(c, hipMalloc((void**)&prod->dev, prod->rows.size() * sizeof(uint32_t)));
    HIP_TRY(c, hipMemcpy(prod->dev, prod->rows.data(), prod->rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return LIG_OK;
}
