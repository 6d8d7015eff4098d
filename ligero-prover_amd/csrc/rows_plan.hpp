// rows_plan.hpp -- the host-side rules of a rows job (lig_hip.h: lig_rows_job), written once for the prover, the sharded prover and
// the verifier: the row kinds and what they draw from the encoding stream, the quadratic-test terms, the narrow row format.
// Host only: nothing but lig_hip.h and the standard library, so that a plain host compiler builds it (tests/cpp/rows_plan_prog.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/lig_hip.h"

// kind: 0 linear, 1 x, 2 y, 3 z of the synthetic stream; rows committed by the batch program (lig_hip.h, lig_batch_op):
// 4 init, 5 bit, 6 / 7 the two rows of an equality, 8 / 9 / 10 the x, y, z of a batch product or quotient
struct RowDesc { uint8_t kind; uint32_t data; };
// `count` consecutive rows from `first` whose k-l pads are element pos, pos + (k-l), ... of the encoding stream
struct PadRun { size_t first, count; uint64_t pos; };

enum : uint8_t { RK_INIT = 4, RK_BIT = 5, RK_EQX = 6, RK_EQY = 7, RK_BQX = 8, RK_BQY = 9, RK_BQZ = 10 };
inline bool has_code_check(uint8_t kind) { return kind != RK_EQX && kind != RK_EQY; }      // nonbatch_context.hpp:811-825

// the kinds alone, as lig_linear_check and the linear entry points take them
inline std::vector<uint8_t> kinds_of(const std::vector<RowDesc>& rows) {
    std::vector<uint8_t> kinds(rows.size());
    for (size_t r = 0; r < rows.size(); r++) kinds[r] = rows[r].kind;
    return kinds;
}
// quadratic-test terms in hook order (one quadratic-stream draw each): (x, y, z) row indices; y = 0xFFFFFFFF marks the
// equality term r * (x - z) (prover_kernels.hip k_quad_rows)
inline std::vector<uint32_t> quad_terms(const std::vector<RowDesc>& rows) {
    std::vector<uint32_t> t;
    for (size_t r = 0; r < rows.size(); r++) {
        const uint8_t kd = rows[r].kind;
        if (kd == 3 || kd == RK_BQZ) { t.push_back((uint32_t)r - 2); t.push_back((uint32_t)r - 1); t.push_back((uint32_t)r); }
        else if (kd == RK_BIT) { t.push_back((uint32_t)r); t.push_back((uint32_t)r); t.push_back((uint32_t)r); }
        else if (kd == RK_EQY) { t.push_back((uint32_t)r - 1); t.push_back(0xFFFFFFFFu); t.push_back((uint32_t)r); }
    }
    return t;
}

namespace lig {
// The kinds of a rows job -> rows (kind without the flag; data = the row's dense count), draw (LIG_ROW_DRAW_PAD given) and pos (R + 1
// entries: the encoding-stream position of every row's pads; pos[R] = the masks').  nullptr = accepted, else why not.
// Groups must be complete and consecutive -- checked for every caller.  Which kinds draw padding from the encoding stream at the
// time they are formed: linear rows and the rows of a quadratic triple (witness_manager.hpp:200-269), on_batch_init rows
// (nonbatch_context.hpp:497-510); bit / equal / batch-quadratic rows are copies of variables and draw nothing.
// prover: the rules of forming the rows as well (the flag only where upstream draws, the pad geometry of on_batch_init, the dense
// counts).  The verifier forms no row: it skips them, ignores the dense counts and gets data = 0.
inline const char* parse_row_kinds(const lig_rows_job& job, uint32_t l, uint32_t k, bool prover, std::vector<RowDesc>& rows,
                                   std::vector<uint8_t>& draw, std::vector<uint64_t>& pos) {
    const size_t R = job.rows;
    const uint32_t pad = k - l;
    const uint8_t* kinds = job.kinds;
    rows.resize(R); draw.assign(R, 0); pos.assign(R + 1, 0);
    for (size_t r = 0; r < R; r++) {
        const uint8_t kd = kinds[r] & 0x7f;
        if (kd > RK_BQZ) return "unknown row kind";
        const bool first_of_3 = kd == 1 || kd == RK_BQX, first_of_2 = kd == RK_EQX;
        if (first_of_3 && !(r + 2 < R && (kinds[r + 1] & 0x7f) == kd + 1 && (kinds[r + 2] & 0x7f) == kd + 2)) return "incomplete x,y,z triple";
        if (first_of_2 && !(r + 1 < R && (kinds[r + 1] & 0x7f) == RK_EQY)) return "incomplete equality pair";
        const bool follower = kd == 2 || kd == 3 || kd == RK_EQY || kd == RK_BQY || kd == RK_BQZ;
        if (follower && !(r > 0 && (kinds[r - 1] & 0x7f) == kd - 1)) return "row of a group without its predecessor";
        const bool draws = kd <= 3 || kd == RK_INIT;
        draw[r] = (kinds[r] & LIG_ROW_DRAW_PAD) ? 1 : 0;
        pos[r + 1] = pos[r] + (draws ? pad : 0);
        rows[r] = RowDesc{kd, 0};
        if (!prover) continue;
        // on_batch_init draws params::sample_size = 192 elements (nonbatch_context.hpp:497-510), the rows of witness_manager
        // k - l; upstream the two are the same number (params.hpp:27-30).  Batch rows are only accepted in that geometry:
        // otherwise the encoding stream would run out of step with the reference's
        if (kd == RK_INIT && pad != 192) return "on_batch_init rows need k - l = 192 (params::sample_size)";
        if (draw[r] && !draws) return "LIG_ROW_DRAW_PAD on a row kind that draws no padding upstream";
        const uint32_t dense = job.dense_rands_per_row ? job.dense_rands_per_row[r] : 0;
        if (dense > k || (dense && kd > 3)) return "dense_rands_per_row out of range or on a batch row";
        rows[r].data = dense;
    }
    return nullptr;
}

// packed bytes of one row of width w (NOT_A_WIDTH = no width of the format): 32 -> all k slots; bits, 1, 2, 4, 8 -> the l data
// slots, rounded up to a multiple of 4 so that every row starts 4-byte aligned; LIG_ELEM_PRODUCT -> 0, the row is derived
static constexpr uint64_t NOT_A_WIDTH = ~(uint64_t)0;
inline uint64_t narrow_row_bytes(uint32_t w, uint32_t l, uint32_t k) {
    switch (w) {
        case 32: return (uint64_t)k * 32;
        case LIG_ELEM_BIT: return ((uint64_t)l + 31) / 32 * 4;
        case 1: case 2: case 4: case 8: return ((uint64_t)l * w + 3) & ~(uint64_t)3;
        case LIG_ELEM_PRODUCT: return 0;
        default: return NOT_A_WIDTH;
    }
}
// elem_bytes[r] of a rows job checked against the row's kind (kind: without the flag; draws: LIG_ROW_DRAW_PAD given).  nullptr = accepted.
inline const char* narrow_row_refusal(const uint8_t* elem_bytes, size_t r, uint8_t kind, bool draws, uint32_t l, uint32_t k) {
    const uint8_t w = elem_bytes[r] ? elem_bytes[r] : 32;
    if (narrow_row_bytes(w, l, k) == NOT_A_WIDTH) return "elem_bytes must be 0, 1, 2, 4, 8, 32, LIG_ELEM_BIT or LIG_ELEM_PRODUCT";
    if (w == LIG_ELEM_PRODUCT) {
        // (a QZ row has its QX and QY in front of it -- the kinds were checked first -- and neither of them can be derived)
        return kind == 3 && draws ? nullptr : "LIG_ELEM_PRODUCT is only accepted on a QZ row with LIG_ROW_DRAW_PAD";
    }
    if (w != 32 && (kind > 3 || !draws)) return "a narrow row must be LINEAR / QX / QY / QZ with LIG_ROW_DRAW_PAD";
    return nullptr;
}

// the record counts of a rows job: the member is read only from a struct that says it has it (lig_hip.h, LIG_ROWS_JOB_WIDE: a caller
// built before the member existed passes a shorter struct)
inline const uint32_t* job_wide_per_row(const lig_rows_job& job) { return (job.reserved & LIG_ROWS_JOB_WIDE) ? job.wide_per_row : nullptr; }
// wide_per_row[r] of a rows job (mixed rows: a narrow row followed by c records of LIG_WIDE_RECORD_BYTES) checked against the row's
// width (elem_bytes == NULL: every row is full width).  nullptr = accepted.
inline const char* wide_row_refusal(const uint8_t* elem_bytes, const uint32_t* wide, size_t r, uint32_t l) {
    if (!wide || !wide[r]) return nullptr;
    const uint8_t w = elem_bytes ? elem_bytes[r] : 32;
    if (w != LIG_ELEM_BIT && w != 1 && w != 2 && w != 4 && w != 8) return "wide_per_row is only accepted on a row of width LIG_ELEM_BIT, 1, 2, 4 or 8";
    if (wide[r] > l) return "wide_per_row: more records than the row has data slots";
    return nullptr;
}

// The narrow row format (lig_rows_job.elem_bytes) of the rows a device holds.  `local` = the global row of every local row, commit
// order: all rows on one GPU, the rows a rank was dealt on a shard (the deal never splits a triple: the x and y of a derived local
// row lr are local rows lr - 2, lr - 1).  Every row of the job is checked, whoever holds it; packed = some row of the JOB is not
// full width (a derived row alone counts) -- false: the plain path, the rest is left empty.
// Mixed rows (lig_rows_job.wide_per_row, one count per row of the JOB; nullptr: none): the c records of a local row lr are the last
// 36 c bytes of its packed range, [src_off[lr + 1] - 36 c, src_off[lr + 1]).
struct NarrowPlan {
    bool packed = false;
    std::vector<uint8_t> widths;          // per local row (one entry at least: nothing of size 0 goes to the device)
    std::vector<uint64_t> src_off;        // packed byte offset of every local row (+1 entry = all the bytes this device is given), records included
    std::vector<uint32_t> prod_rows;      // local indices of the derived rows (LIG_ELEM_PRODUCT), ascending
    std::vector<uint32_t> wide;           // records per local row; EMPTY when no local row is mixed
    std::vector<uint32_t> mixed_rows;     // local indices of the mixed rows, ascending
};
inline const char* plan_narrow_rows(const uint8_t* elem_bytes, const std::vector<RowDesc>& rows, const std::vector<uint8_t>& draw, uint32_t l,
                                    uint32_t k, const std::vector<size_t>& local, NarrowPlan& out, const uint32_t* wide_per_row = nullptr) {
    out = NarrowPlan{};
    for (size_t r = 0; r < rows.size(); r++) {
        if (elem_bytes) {
            if (const char* why = narrow_row_refusal(elem_bytes, r, rows[r].kind, draw[r] != 0, l, k)) return why;
            out.packed = out.packed || (elem_bytes[r] != 0 && elem_bytes[r] != 32);
        }
        if (const char* why = wide_row_refusal(elem_bytes, wide_per_row, r, l)) return why;
    }
    if (!out.packed) return nullptr;
    out.widths.assign(local.empty() ? 1 : local.size(), 32);
    out.src_off.assign(local.size() + 1, 0);
    for (size_t lr = 0; lr < local.size(); lr++) {
        const uint8_t w = elem_bytes[local[lr]] ? elem_bytes[local[lr]] : 32;
        const uint32_t c = wide_per_row ? wide_per_row[local[lr]] : 0;
        out.widths[lr] = w;
        out.src_off[lr + 1] = out.src_off[lr] + narrow_row_bytes(w, l, k) + (uint64_t)c * LIG_WIDE_RECORD_BYTES;
        if (w == LIG_ELEM_PRODUCT) out.prod_rows.push_back((uint32_t)lr);
        if (c) out.mixed_rows.push_back((uint32_t)lr);
    }
    if (!out.mixed_rows.empty()) {
        out.wide.assign(local.size(), 0);
        for (const uint32_t lr : out.mixed_rows) out.wide[lr] = wide_per_row[local[lr]];
    }
    return nullptr;
}
// The records of mixed HOST rows, read before any copy starts: `packed` = the rows of the plan back to back (src_off), mixed_rows /
// wide as in the plan.  nullptr = every column is < l and the columns of every row are strictly ascending.
inline const char* wide_records_refusal(const uint8_t* packed, const std::vector<uint64_t>& src_off, const std::vector<uint32_t>& mixed_rows,
                                        const std::vector<uint32_t>& wide, uint32_t l) {
    for (const uint32_t lr : mixed_rows) {
        const uint8_t* rec = packed + src_off[lr + 1] - (uint64_t)wide[lr] * LIG_WIDE_RECORD_BYTES;
        uint32_t prev = 0;
        for (uint32_t j = 0; j < wide[lr]; j++, rec += LIG_WIDE_RECORD_BYTES) {
            uint32_t col;
            std::memcpy(&col, rec, 4);
            if (col >= l) return "a wide slot names a column >= l";
            if (j && col <= prev) return "the wide slots of a row are not in strictly ascending column order";
            prev = col;
        }
    }
    return nullptr;
}
}  // namespace lig
