// lig_hip_row_batcher.hpp -- the row-batching shim between the reference's per-row stage callbacks and the batched
// caller-rows prover entry of liblig_hip.so (lig_rows_*, include/lig_hip.h).
//
// The reference's stage contexts push ONE row through the executor per callback and run the guest three times
// (include/zkp/nonbatch_context.hpp: stage 1 :445-553, stage 2 :654-850, stage 3 :924-1047; src/webgpu_prover.cpp:266,305,408).
// `ligero::hip_row_batcher` offers the same callbacks -- linear_callback / quadratic_callback / mask_callback /
// on_batch_init / on_batch_bit / on_batch_equal / on_batch_quadratic, called by witness_manager
// (include/zkp/backend/witness_manager.hpp:200-321) and vbn254fr_module (include/host_modules/vbn254fr.hpp) -- but only
// RECORDS the rows; the GPU sees them in one batch per stage:
//
//     hip_row_batcher b(ctx, meta);                       // meta: encoding seed, program hash, timestamp, public arguments
//     run_program(..., b)            pass 1               // callbacks record the message rows (pads included, as the
//     root, seed1 = b.commit();                           //   witness_manager forms them) -> stage 1 on the GPU
//     init_witness_random(seed1); run_program(..., b)     // pass 2: the same callbacks now also carry the per-witness
//     proof = b.prove(linear_sums);                       //   randomness rows -> stages 2 + 3 on the GPU
//
// A third run of the guest (the reference's stage 3) is not needed: the codewords stayed resident, the opened columns
// are gathered from them.  Rows are `k * 4` little-endian u64 limbs, exactly what mpz_vector::export_limbs produces
// (include/util/mpz_vector.hpp:108-127; nonbatch_context.hpp:447); batch rows are device rows of the vbn254fr slab.
// The three mask rows arrive through mask_callback upstream; the library forms the identical rows itself from the
// encoding seed (same stream, same position: after the pads of all rows), so mask_callback only checks sizes.
//
// Data path (round 4): rows are written ONCE, into page-locked staging (lig_host_alloc; `next_slot()` lets a driver export a
// row's limbs straight into it), the staging is kept for the next pass and the next proof (`reset()`), `commit()` uploads
// from it chunk by chunk under the encodes, and in pass 2 every 256 completed randomness rows are handed to the library at
// once (lig_rows_push_rands) -- their upload runs while the guest is still producing the next ones, `prove()` only waits for
// the tail.  tests/cpp/row_batcher_bench.cpp measures it (profiles/r04_row_batcher_bench.md).
#pragma once
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "lig_hip.h"

namespace ligero {

struct hip_proof_meta {
    uint8_t encoding_seed[32] = {0};          // src/webgpu_prover.cpp:239-245
    uint8_t program_hash[32] = {0};           // :222-223
    int64_t generated_at = 0;                 // :422-427
    std::string version = "1.5.0";
    std::vector<std::vector<uint8_t>> public_args;   // input_args entries of the PUBLIC arguments after arg0 (:110-168)
    // Ship narrow rows (lig_rows_job.elem_bytes): a linear / x / y / z row all of whose data slots fit 8 bytes is uploaded as
    // l x 8 bytes instead of k x 32, and its k - l pad slots are drawn by the library.  Sound only because those pads ARE the
    // encoding stream at the row's position (witness_manager::pad_encoding_random, witness_manager.hpp:323-336, keyed by
    // encoding_seed): the library draws the same elements the row arrived with.
    bool narrow_rows = false;
    // With narrow_rows: ship every such row in the NARROWEST width its data slots fit -- bits, 1, 2, 4 or 8 bytes per slot
    // (LIG_ELEM_BIT / elem_bytes) -- on one GPU and on every rank of a sharded trace (shard_over).  Off: 8 bytes per slot on one
    // GPU, full rows when sharded.
    bool narrowest = false;
    // With narrow_rows and narrowest: MIXED rows (lig_rows_job.wide_per_row).  The OR of a row's slots no longer decides: every linear /
    // x / y / z row is shipped in the base width -- bits, 1, 2, 4 or 8 bytes -- for which the narrow row plus one 36-byte record per
    // data slot that does not fit is the fewest bytes (the narrower base on a tie), at full width only where that is not more bytes.
    // A bit row with a few machine words among its slots stays a bit row.  Without the other two options it has no effect.
    bool wide_slots = false;
    // With narrow_rows: the z row of every triple recorded by quadratic_callback is NOT shipped (LIG_ELEM_PRODUCT): the library forms
    // x * y mod p on the device from the x and y rows it received, on one GPU and on every rank of a sharded trace, and draws the
    // row's pads.  The z the guest handed over is ignored: the prover's valid_quad says nothing about such a triple -- a guest whose z
    // was wrong proves the product instead, and a linear constraint on that z fails (valid_linear with set_linear_system).
    bool derive_products = false;
    // Rows the guest is expected to commit (0: unknown).  The staging is page-locked memory that grows geometrically when the
    // guest outruns it; a driver that proves the same program again (or knows its size) saves the re-allocations.
    size_t expected_rows = 0;
};

// Page-locked host staging for rows of k x 4 u64 (lig_host_alloc): the callbacks write rows straight into it -- no pageable
// std::vector, no second copy at commit() -- and it is kept for the next pass and the next proof (reset()).
class hip_row_staging {
public:
    hip_row_staging(lig_ctx* ctx, size_t row_words) : ctx_(ctx), words_(row_words) {}
    hip_row_staging(const hip_row_staging&) = delete;
    hip_row_staging& operator=(const hip_row_staging&) = delete;
    ~hip_row_staging() { if (base_) (void)lig_host_free(ctx_, base_); }
    uint64_t* row(size_t r) { return base_ + r * words_; }
    const uint64_t* data() const { return base_; }
    size_t capacity() const { return cap_; }
    // room for `rows` rows; the first `keep` rows survive a re-allocation
    void reserve(size_t rows, size_t keep) {
        if (rows <= cap_) return;
        size_t want = cap_ ? cap_ : 64;
        while (want < rows) want += want < 4096 ? want : 4096;         // double up to 4096 rows (1 GiB at k = 8192), then 1 GiB steps
        void* p = nullptr;
        if (lig_host_alloc(ctx_, want * words_ * 8, &p) != LIG_OK) throw std::runtime_error(std::string("lig_host_alloc: ") + lig_last_error(ctx_));
        if (keep) std::memcpy(p, base_, keep * words_ * 8);
        if (base_) (void)lig_host_free(ctx_, base_);
        base_ = static_cast<uint64_t*>(p);
        cap_ = want;
    }
private:
    lig_ctx* ctx_;
    size_t words_, cap_ = 0;
    uint64_t* base_ = nullptr;
};

// A deep copy of a lig_linear_system (include/lig_hip.h): the shims keep the caller's description until there is a trace to set it on.
class hip_linear_system_copy {
public:
    void assign(const lig_linear_system& s) {
        if (s.struct_bytes < sizeof(lig_linear_system)) throw std::invalid_argument("set_linear_system: struct_bytes too small");
        if (!s.term_begin || (s.n_terms && !s.terms) || (s.n_rhs && (!s.rhs_constraint || !s.rhs_coef)) || (s.n_coefs && !s.coefs))
            throw std::invalid_argument("set_linear_system: null array");
        term_begin_.assign(s.term_begin, s.term_begin + s.n_constraints + 1);
        terms_.assign(s.terms, s.terms + s.n_terms);
        rhs_c_.assign(s.rhs_constraint, s.rhs_constraint + s.n_rhs);
        rhs_b_.assign(s.rhs_coef, s.rhs_coef + s.n_rhs);
        coefs_.assign(s.coefs, s.coefs + s.n_coefs * 32);
        sys_ = s;
        sys_.struct_bytes = sizeof(lig_linear_system);
        sys_.term_begin = term_begin_.data(); sys_.terms = terms_.data(); sys_.rhs_constraint = rhs_c_.data(); sys_.rhs_coef = rhs_b_.data();
        sys_.coefs = coefs_.data();
        set_ = true;
    }
    bool is_set() const { return set_; }
    void clear() { sys_ = lig_linear_system{}; set_ = false; }
    const lig_linear_system* get() const { return &sys_; }
private:
    bool set_ = false;
    lig_linear_system sys_{};
    std::vector<uint32_t> term_begin_, rhs_c_, rhs_b_;
    std::vector<lig_lin_term> terms_;
    std::vector<uint8_t> coefs_;
};

class hip_row_batcher {
public:
    hip_row_batcher(lig_ctx* ctx, hip_proof_meta meta)
        : ctx_(ctx), meta_(std::move(meta)), k_(ctx ? lig_padding_size(ctx) : 0), l_(ctx ? lig_message_size(ctx) : 0),
          rows_(ctx, (size_t)k_ * 4), rands_(ctx, (size_t)k_ * 4) {
        if (!ctx_) throw std::invalid_argument("hip_row_batcher: null context");
        if (meta_.expected_rows) rows_.reserve(meta_.expected_rows, 0);
    }
    hip_row_batcher(const hip_row_batcher&) = delete;
    hip_row_batcher& operator=(const hip_row_batcher&) = delete;
    ~hip_row_batcher() { if (trace_) lig_trace_destroy(trace_); if (shard_) lig_shard_destroy(shard_); }

    // ONE trace over the GPUs of a node (configs[4]: the guest's rows on 8 GPUs): every rank runs the same guest, so every rank's
    // callbacks see all rows; after pass 1 the batcher keeps the rows of its own chunks (lig_shard_rows_plan), in pass 2 the
    // randomness rows of those.  Call before commit(); `comm` from lig_rccl_comm_create (or lig_ipc_comm_create) must outlive
    // the batcher.  Every rank's prove() returns the same envelope as an unsharded batcher would.
    void shard_over(uint32_t rank, uint32_t world, const lig_comm* comm) {
        if (pass_ != 1 || !comm || !world || rank >= world) throw std::invalid_argument("hip_row_batcher::shard_over");
        if (program_) throw std::logic_error("hip_row_batcher::shard_over: a prepared linear program is not for a sharded batcher (set_linear_system)");
        if (!derived_.empty()) throw std::logic_error("hip_row_batcher::shard_over: derived slots are not for a sharded batcher (set_derived_slots)");
        if (shard_) { lig_shard_destroy(shard_); shard_ = nullptr; linear_on_trace_ = false; shard_derived_on_shard_ = shard_derived_.empty(); }      // another deal: nothing of the old shard is reused
        sharded_ = true; rank_ = rank; world_ = world; comm_ = *comm;
    }

    // The linear constraints of the program as a sparse term list (lig_linear_system): the library then
    // forms the linear-test randomness rows and the public constant on the GPU.  Pass 2 -- the second run of the guest -- is no
    // longer needed: prove() may follow commit() directly (callbacks of a pass 2 that is replayed all the same are only counted),
    // and prove(nullptr) takes the system's own constant.  Any time before prove(); copied; kept across reset() for the next proof
    // of the same program, where the structure stays resident on the device.  With shard_over() (before or after it): the system
    // describes the WHOLE trace and every rank sets the same one (lig_shard_rows_set_linear); each rank forms the rows of its own chunks.
    void set_linear_system(const lig_linear_system& sys) {
        if (pass_ == 3) throw std::logic_error("hip_row_batcher::set_linear_system after prove (reset() first)");
        if (pass_ == 2 && pushed_) throw std::logic_error("hip_row_batcher::set_linear_system: randomness rows have already been handed over");
        linear_.assign(sys);
        program_ = nullptr; values_set_ = false;          // (a system and a program replace each other; values belong to what they were set on)
        linear_on_trace_ = values_on_trace_ = false;
        if (pass_ == 2) apply_linear();
    }
    // The same with a structure prepared once (lig_linear_prepare): one lig_linear_program may feed any
    // number of batchers and verifiers, of any context on its device, at the same time; nothing is uploaded or regrouped here.  Not
    // copied and not owned: the caller keeps its reference for as long as this batcher may still begin a trace with it (the trace
    // itself holds a reference of its own once the program is attached).  Kept across reset(); nullptr removes it.  Not with
    // shard_over(): a rank's structure depends on its deal (set_linear_system there).
    void set_linear_program(const lig_linear_program* p) {
        if (pass_ == 3) throw std::logic_error("hip_row_batcher::set_linear_program after prove (reset() first)");
        if (pass_ == 2 && pushed_) throw std::logic_error("hip_row_batcher::set_linear_program: randomness rows have already been handed over");
        if (p && sharded_) throw std::logic_error("hip_row_batcher::set_linear_program: not on a sharded batcher (set_linear_system)");
        linear_.clear();
        program_ = p; values_set_ = false;
        linear_on_trace_ = values_on_trace_ = false;
        if (pass_ == 2) {
            if (p) apply_linear();
            else check(lig_rows_attach_linear(trace_, nullptr), "lig_rows_attach_linear");
        }
    }
    // The values of the coefficient table for the proofs that follow (lig_rows_set_linear_values): n_coefs x 32 bytes, canonical,
    // n_coefs as in the system / program -- the public right-hand sides of a new statement of the same program are the entries that
    // rhs_coef names.  Copied; kept across reset() until set again; nullptr: the table the system / program came with.
    // With shard_over(): lig_shard_rows_set_linear_values -- every rank sets the same values (no collective is involved); the rank's
    // share of the system stays as it is, nothing is checked, uploaded or regrouped again.
    void set_linear_values(const uint8_t* coefs, uint64_t n_coefs) {
        if (pass_ == 3) throw std::logic_error("hip_row_batcher::set_linear_values after prove (reset() first)");
        if (!has_linear()) throw std::logic_error("hip_row_batcher::set_linear_values without a linear system or program");
        values_set_ = coefs != nullptr;
        values_.assign(coefs, coefs + (coefs ? n_coefs * 32 : 0));
        values_on_trace_ = false;
        if (pass_ == 2 && linear_on_trace_) apply_values();      // (pass 1: with the attach / after the restart of the next commit())
    }

    // Derived slots (lig_rows_set_derived): the outputs of the guest's eval() calls.  d[i] = (slot, its
    // DEFINING constraint in `sys`): the library forms w[slot] from the other terms of that constraint in commit(), whatever the row
    // carries there (the driver writes 0, so a bit row stays a bit row).  In pass 1, before commit(); sys and d are copied (sys need
    // not be the system of set_linear_system); kept across reset() for the next proof of the same shape, where the list stays
    // resident on the trace -- for other right-hand sides call it again; n == 0 removes the list.  Not with shard_over(): a sharded
    // batcher takes its list through shard_set_derived_slots() below.  A product a * b of the guest whose operand is an eval() output
    // (or whose product feeds one): list product_entry(slot of z) next to the operand's own entry -- column i of a derive_products z row
    // is then re-formed from the committed operands in wave order (lig_hip.h: LIG_DERIVED_PRODUCT).
    static lig_derived_slot product_entry(uint32_t slot) { return lig_derived_slot{slot, LIG_DERIVED_PRODUCT}; }
    void set_derived_slots(const lig_linear_system& sys, const lig_derived_slot* d, uint64_t n) {
        if (pass_ != 1) throw std::logic_error("hip_row_batcher::set_derived_slots after commit (reset() first)");
        if (sharded_) throw std::logic_error("hip_row_batcher::set_derived_slots: not on a sharded batcher");
        if (n && !d) throw std::invalid_argument("hip_row_batcher::set_derived_slots: null list");
        if (n) derived_sys_.assign(sys); else derived_sys_.clear();
        derived_.assign(d, d + n);
        derived_on_trace_ = false;
    }
    // set_derived_slots() for a batcher with shard_over(): lig_shard_rows_set_derived (lig_hip.h).  sys and d describe the WHOLE trace with
    // global slots and EVERY RANK PASSES THE SAME LIST (the ranks compute their exchange schedule from it; no collective is involved in the
    // call).  Each rank forms the targets on its own rows in commit(), importing the operands other ranks hold; a list whose constraints
    // are row-local exchanges nothing.  In pass 1, before commit(); copied; kept across reset() -- the list stays resident on the shard,
    // applied before lig_shard_rows_commit; n == 0 removes it.  std::logic_error on an unsharded batcher and after commit().
    void shard_set_derived_slots(const lig_linear_system& sys, const lig_derived_slot* d, uint64_t n) {
        if (!sharded_) throw std::logic_error("hip_row_batcher::shard_set_derived_slots: not a sharded batcher (set_derived_slots)");
        if (pass_ != 1) throw std::logic_error("hip_row_batcher::shard_set_derived_slots after commit (reset() first)");
        if (n && !d) throw std::invalid_argument("hip_row_batcher::shard_set_derived_slots: null list");
        if (n) shard_derived_sys_.assign(sys); else shard_derived_sys_.clear();
        shard_derived_.assign(d, d + n);
        shard_derived_on_shard_ = false;
    }

    // ---- the callbacks of nonbatch_context_base (nonbatch_context.hpp:78-86).  `rand` rows are null in pass 1.
    void linear_callback(const uint64_t* val, const uint64_t* rand = nullptr) { row(LIG_ROW_LINEAR, val, rand); }
    void quadratic_callback(const uint64_t* x, const uint64_t* y, const uint64_t* z, const uint64_t* x_rand = nullptr,
                            const uint64_t* y_rand = nullptr, const uint64_t* z_rand = nullptr) {
        row(LIG_ROW_QX, x, x_rand); row(LIG_ROW_QY, y, y_rand); row(LIG_ROW_QZ, z, z_rand);
    }
    // The same callbacks without the copy: where the reference exports a row's limbs into its `limbs_` vector
    // (mpz_vector::export_limbs, nonbatch_context.hpp:447 / :657-663) an integrated driver exports them straight into the slot --
    // k x 4 u64 of page-locked staging -- and then commits the slot.  Pass 1: the slot of the next message row; pass 2: the slot
    // of the next row's randomness row (nullptr for a row this rank does not own when sharded: nothing to export).
    uint64_t* next_slot() {
        if (pass_ == 1) { rows_.reserve(kinds_.size() + 1, kinds_.size()); return rows_.row(kinds_.size()); }
        if (pass_ != 2 || next_ >= kinds_.size()) throw std::logic_error("hip_row_batcher::next_slot: no row expected");
        if (sharded_ && has_linear()) return rands_.row(0);  // the library forms the randomness rows: what is exported here is never read
        if (!sharded_) return rands_.row(n_present_);            // randomness rows are kept packed: only rows that have one take a slot
        const size_t slot = local_of_[next_];
        return slot == (size_t)-1 ? nullptr : rands_.row(slot);
    }
    // has_rand = false in pass 2: the row has no randomness row (nothing was exported into the slot; it stays free for the next row)
    void commit_slot(uint8_t kind, bool has_rand = true) { row(kind, pass_ == 1 ? rows_.row(kinds_.size()) : nullptr, nullptr, true, has_rand); }
    void mask_callback(size_t code_size, size_t linear_size, size_t quad_size) const {
        if (code_size != k_ || linear_size != 2 * (size_t)k_ || quad_size != 2 * (size_t)k_) throw std::invalid_argument("mask_callback: unexpected mask sizes");
    }
    // vbn254fr hooks (nonbatch_context.hpp:497-553, :782-850): device rows of k elements; they carry no linear-test randomness.
    // on_batch_init (:497-510) first draws params::sample_size = 192 elements from the encoding stream
    // (pad_encoding_random) and writes them INTO the variable at slot message_size, then commits the row -- the pad is part of
    // the variable from then on and flows into every batch row derived from it.  Every stage re-runs the guest with the
    // encoding engine re-seeded, so pass 2 writes the same 192 elements again.
    void on_batch_init(void* dev_x) { on_batch_init(dev_x, static_cast<uint8_t*>(dev_x) + (size_t)l_ * 32); }
    // `pad_dst`: where the 192 pad elements go.  The declared semantics of buffer_view::slice put them into x's own pad slots
    // (the overload above); upstream's buffer_view::slice_bytes as DEFINED (src/webgpu/buffer_view.cpp:91-95 swaps its parameters)
    // puts them at byte l * 32 of the whole variable slab, i.e. into variable 0 -- hip_context's upstream_slice_compat mode hands
    // that address in.
    void on_batch_init(void* dev_x, void* pad_dst) {
        if (pass_ != 1 && pass_ != 2) throw std::logic_error("hip_row_batcher: callback after prove");
        if (k_ - l_ != init_pad) throw std::invalid_argument("hip_row_batcher::on_batch_init: k - l must be params::sample_size (192)");
        check(lig_rng_fill(ctx_, meta_.encoding_seed, enc_pos_, pad_dst, init_pad), "lig_rng_fill(init pad)");
        enc_pos_ += init_pad;
        dev_row(LIG_ROW_INIT, dev_x);
    }
    void on_batch_bit(const void* dev_x) { dev_row(LIG_ROW_BIT, dev_x); }
    void on_batch_equal(const void* dev_x, const void* dev_y) { dev_row(LIG_ROW_EQX, dev_x); dev_row(LIG_ROW_EQY, dev_y); }
    void on_batch_quadratic(const void* dev_x, const void* dev_y, const void* dev_z) {
        dev_row(LIG_ROW_BQX, dev_x); dev_row(LIG_ROW_BQY, dev_y); dev_row(LIG_ROW_BQZ, dev_z);
    }

    // ---- end of pass 1: stage 1 on the GPU.  Returns the Merkle root and the stage-1 seed (= the key of the code /
    // linear / quadratic random engines of pass 2, nonbatch_context.hpp:105-112).
    void commit(uint8_t root[32], uint8_t stage1_seed[32]) {
        if (pass_ != 1) throw std::logic_error("hip_row_batcher::commit called twice");
        std::vector<uint8_t> args;
        std::vector<uint64_t> lens;
        for (const auto& a : meta_.public_args) { args.insert(args.end(), a.begin(), a.end()); lens.push_back(a.size()); }
        lig_rows_job job;
        std::memset(&job, 0, sizeof job);
        job.rows = kinds_.size();
        job.kinds = kinds_.data();
        job.msgs = rows_.data();
        job.msgs_on_device = 0;
        std::memcpy(job.encoding_seed, meta_.encoding_seed, 32);
        std::memcpy(job.program_hash, meta_.program_hash, 32);
        job.generated_at = meta_.generated_at;
        std::strncpy(job.version, meta_.version.c_str(), sizeof job.version - 1);
        job.public_args = args.empty() ? nullptr : args.data();
        job.public_arg_lens = lens.empty() ? nullptr : lens.data();
        job.n_public_args = lens.size();
        shipped_ = kinds_.size() * (size_t)k_ * 32;
        if (sharded_) { commit_sharded(job, root, stage1_seed); return; }
        std::vector<uint8_t> widths;
        std::vector<uint32_t> wide;
        if (meta_.narrow_rows) {
            // packed IN PLACE: a narrow row shrinks to l x (its width) bytes, rows only ever move towards the front of the staging
            const size_t R = kinds_.size();
            if (plan_widths(widths, true, wide)) {
                uint8_t* out = reinterpret_cast<uint8_t*>(rows_.row(0));
                for (size_t r = 0; r < R; r++) {
                    if (widths[r] != 32) kinds_[r] |= LIG_ROW_DRAW_PAD;
                    out = pack_row(rows_.row(r), widths[r], out, wide.empty() ? 0 : wide[r]);
                }
                job.elem_bytes = widths.data();
                job.wide_per_row = wide.empty() ? nullptr : wide.data();
                job.reserved = LIG_ROWS_JOB_WIDE;
                shipped_ = out - reinterpret_cast<uint8_t*>(rows_.row(0));
            }
        }
        if (trace_) {                                      // the next proof of the same program: every device buffer is reused
            if (same_shape(job)) check(lig_rows_restart(trace_, job.msgs, 0), "lig_rows_restart");
            else { lig_trace_destroy(trace_); trace_ = nullptr; linear_on_trace_ = values_on_trace_ = false; derived_on_trace_ = derived_.empty(); }
        }
        if (!trace_) check(lig_rows_begin(ctx_, &job, &trace_), "lig_rows_begin");
        shape_kinds_ = kinds_; shape_widths_ = widths; shape_wide_ = wide; shape_meta_ = meta_;
        apply_linear();                                   // (a trace that was restarted keeps the structure it has)
        if (!derived_on_trace_) {                         // (... and the list of derived slots)
            check(lig_rows_set_derived(trace_, derived_.empty() ? nullptr : derived_sys_.get(), derived_.empty() ? nullptr : derived_.data(), derived_.size(), nullptr), "lig_rows_set_derived");
            derived_on_trace_ = true;
        }
        check(lig_rows_commit(trace_, root, stage1_seed), "lig_rows_commit");
        for (auto& kd : kinds_) kd &= 0x7f;               // (pass 2 compares plain kinds)
        begin_pass2(kinds_.size());
    }

    // ---- end of pass 2: stages 2 + 3 on the GPU.  const_sum = the public constant of the linear test, 32 bytes little
    // endian (linear_sums(), src/webgpu_prover.cpp:307).  The returned bytes are the serialized LigeroProofEnvelope
    // (owned by the batcher, valid until it is destroyed or reset); `info` (optional) receives the prover's self-check.
    const uint8_t* prove(const uint8_t const_sum[32], size_t* proof_len, lig_proof_info* info = nullptr) {
        if (pass_ != 2) throw std::logic_error("hip_row_batcher::prove before commit");
        const bool linear = has_linear();
        if (!linear && next_ != kinds_.size()) throw std::logic_error("hip_row_batcher::prove: pass 2 replayed " + std::to_string(next_) + " of " + std::to_string(kinds_.size()) + " rows");
        const uint8_t* proof = nullptr;
        lig_proof_info local;
        if (sharded_) check(lig_shard_rows_prove(shard_, linear ? nullptr : rands_.data(), 0, const_sum, &proof, proof_len, info ? info : &local), "lig_shard_rows_prove");
        else {
            if (!linear) push_rands(kinds_.size());        // the tail; everything else went out while the guest was running
            check(lig_rows_prove(trace_, nullptr, 0, const_sum, &proof, proof_len, info ? info : &local), "lig_rows_prove");
        }
        pass_ = 3;
        return proof;
    }
    // ---- when valid_linear or valid_quad came out 0 (or before prove(), to save the proof): WHICH constraints does the committed
    // witness violate?  lig_rows_diagnose (lig_hip.h) with the system given to set_linear_system -- with the table of
    // set_linear_values, if one was set -- after commit(), before or after prove(), until the next commit().  A batcher that was
    // given a prepared program (set_linear_program) or no system has no term list to evaluate: the quadratic part only -- the linear
    // constraints of such a batcher are named by diagnose_attached() below, which needs no term list.  Upstream
    // the same witness would have tripped the asserts of constrain_equal / constrain_bit while the guest ran
    // (witness_manager.hpp:418-431).  With shard_over(): lig_shard_rows_diagnose, a COLLECTIVE call -- every rank calls it with the same
    // caps and gets the output of the unsharded batcher, global row numbers included (a constraint may span ranks: the ranks' partial
    // sums are reduced across them).
    void diagnose(lig_diag_linear* lin_out, uint64_t lin_cap, lig_diag_quad* quad_out, uint64_t quad_cap, lig_diag_info* info) {
        if (pass_ == 1 || !(sharded_ ? (bool)shard_ : (bool)trace_)) throw std::logic_error("hip_row_batcher::diagnose before commit");
        if (!info) throw std::invalid_argument("hip_row_batcher::diagnose: null info");
        lig_linear_system sys = *linear_.get();
        if (values_set_) { sys.coefs = values_.data(); sys.n_coefs = values_.size() / 32; }
        info->struct_bytes = sizeof(lig_diag_info);
        if (sharded_) {
            check(lig_shard_rows_diagnose(shard_, linear_.is_set() ? &sys : nullptr, lin_out, lin_cap, quad_out, quad_cap, info), "lig_shard_rows_diagnose");
            return;
        }
        check(lig_rows_diagnose(trace_, linear_.is_set() ? &sys : nullptr, lin_out, lin_cap, quad_out, quad_cap, info), "lig_rows_diagnose");
    }
    // The same question put to the statement ATTACHED to the trace (lig_rows_diagnose_attached, lig_hip.h): the structure of
    // set_linear_system or set_linear_program as it lies on the device, with the values of set_linear_values in force if any were set --
    // exactly what prove(nullptr) proves.  No term list is needed: the caller of set_linear_program may have released its own long ago.
    // After commit(), before or after prove(), until the next commit(); same output as diagnose().  std::logic_error before commit() and
    // without a system or program.  With shard_over(): lig_shard_rows_diagnose_attached, a COLLECTIVE call over every rank's share of
    // the system as it lies on its device -- every rank calls it with the same caps and gets the output of the unsharded batcher.
    void diagnose_attached(lig_diag_linear* lin_out, uint64_t lin_cap, lig_diag_quad* quad_out, uint64_t quad_cap, lig_diag_info* info) {
        if (pass_ == 1 || !(sharded_ ? (bool)shard_ : (bool)trace_)) throw std::logic_error("hip_row_batcher::diagnose_attached before commit");
        if (!has_linear() || !linear_on_trace_) throw std::logic_error("hip_row_batcher::diagnose_attached without a linear system or program");
        if (!info) throw std::invalid_argument("hip_row_batcher::diagnose_attached: null info");
        info->struct_bytes = sizeof(lig_diag_info);
        if (sharded_) {
            check(lig_shard_rows_diagnose_attached(shard_, lin_out, lin_cap, quad_out, quad_cap, info), "lig_shard_rows_diagnose_attached");
            return;
        }
        check(lig_rows_diagnose_attached(trace_, lin_out, lin_cap, quad_out, quad_cap, info), "lig_rows_diagnose_attached");
    }
    // ---- diagnose() names the violated constraints; these SHOW constraints: every term with its slot, coefficient index, coefficient
    // value and the witness value the library committed, the right-hand side and the residual (lig_rows_explain, lig_hip.h).
    // constraints: n_asked numbers, strictly ascending; con_out: n_asked records; terms_out: the first term_cap term records in
    // ascending (constraint, slot, coef_index) order (NULL with term_cap = 0: con_out and the counts only).
    // explain(): the system given to set_linear_system, with the table of set_linear_values if one was set -- as diagnose() does; a
    // batcher with a prepared program or without a system has no term list: std::logic_error (explain_attached()).
    // explain_attached(): the statement attached to the trace, as diagnose_attached(): no term list is needed.
    // Both after commit(), before or after prove(), until the next commit(); the same bytes for the same statement.  std::logic_error
    // before commit().  With shard_over(): explain() is lig_shard_rows_explain, a COLLECTIVE call -- every rank calls it with the same
    // asked list and term_cap and gets the records of the unsharded batcher, whichever rank holds the rows of a term; explain_attached()
    // stays std::logic_error there: the attached statement of a sharded batcher is shown by shard_explain_attached() below.
    void explain(const uint32_t* constraints, uint64_t n_asked, lig_explain_constraint* con_out, lig_explain_term* terms_out, uint64_t term_cap,
                 lig_explain_info* info) {
        if (pass_ == 1 || !(sharded_ ? (bool)shard_ : (bool)trace_)) throw std::logic_error("hip_row_batcher::explain before commit");
        if (!linear_.is_set()) throw std::logic_error("hip_row_batcher::explain without a linear system (explain_attached)");
        if (!info) throw std::invalid_argument("hip_row_batcher::explain: null info");
        lig_linear_system sys = *linear_.get();
        if (values_set_) { sys.coefs = values_.data(); sys.n_coefs = values_.size() / 32; }
        info->struct_bytes = sizeof(lig_explain_info);
        if (sharded_) {
            check(lig_shard_rows_explain(shard_, &sys, constraints, n_asked, con_out, terms_out, term_cap, info), "lig_shard_rows_explain");
            return;
        }
        check(lig_rows_explain(trace_, &sys, constraints, n_asked, con_out, terms_out, term_cap, info), "lig_rows_explain");
    }
    void explain_attached(const uint32_t* constraints, uint64_t n_asked, lig_explain_constraint* con_out, lig_explain_term* terms_out, uint64_t term_cap,
                          lig_explain_info* info) {
        if (sharded_) throw std::logic_error("hip_row_batcher::explain_attached: not on a sharded batcher");
        if (pass_ == 1 || !trace_) throw std::logic_error("hip_row_batcher::explain_attached before commit");
        if (!has_linear() || !linear_on_trace_) throw std::logic_error("hip_row_batcher::explain_attached without a linear system or program");
        if (!info) throw std::invalid_argument("hip_row_batcher::explain_attached: null info");
        info->struct_bytes = sizeof(lig_explain_info);
        check(lig_rows_explain_attached(trace_, constraints, n_asked, con_out, terms_out, term_cap, info), "lig_rows_explain_attached");
    }
    // explain_attached() for a batcher with shard_over(): lig_shard_rows_explain_attached (lig_hip.h), a COLLECTIVE call over every rank's
    // share of the system as it lies on its device, with the values of set_linear_values in force -- what diagnose_attached() evaluated.
    // Every rank calls it with the same asked list and term_cap and gets the bytes of explain() on the same batcher; no term list is
    // read.  After commit(), before or after prove(), until the next commit().  std::logic_error on an unsharded batcher, before commit()
    // and without a system.
    void shard_explain_attached(const uint32_t* constraints, uint64_t n_asked, lig_explain_constraint* con_out, lig_explain_term* terms_out,
                                uint64_t term_cap, lig_explain_info* info) {
        if (!sharded_) throw std::logic_error("hip_row_batcher::shard_explain_attached: not a sharded batcher (explain_attached)");
        if (pass_ == 1 || !shard_) throw std::logic_error("hip_row_batcher::shard_explain_attached before commit");
        if (!has_linear() || !linear_on_trace_) throw std::logic_error("hip_row_batcher::shard_explain_attached without a linear system");
        if (!info) throw std::invalid_argument("hip_row_batcher::shard_explain_attached: null info");
        info->struct_bytes = sizeof(lig_explain_info);
        check(lig_shard_rows_explain_attached(shard_, constraints, n_asked, con_out, terms_out, term_cap, info), "lig_shard_rows_explain_attached");
    }
    // the committed witness elements of `slots` (row * l + column over the committed rows of any kind: derived and mixed rows as the
    // device holds them; any order, repeats allowed) -> values, n_slots x 32 canonical bytes (lig_rows_read_slots).  Window as explain().
    // With shard_over(): lig_shard_rows_read_slots, COLLECTIVE -- the slots are those of the whole trace, every rank passes the same list.
    void read_slots(const uint32_t* slots, uint64_t n_slots, uint8_t* values) {
        if (pass_ == 1 || !(sharded_ ? (bool)shard_ : (bool)trace_)) throw std::logic_error("hip_row_batcher::read_slots before commit");
        if (sharded_) {
            check(lig_shard_rows_read_slots(shard_, slots, n_slots, values), "lig_shard_rows_read_slots");
            return;
        }
        check(lig_rows_read_slots(trace_, slots, n_slots, values), "lig_rows_read_slots");
    }
    // ---- explain() starts from a constraint; these start from a SLOT: the constraints through each asked slot with their sizes,
    // coefficient values and residuals, and the witness slots of the LINEAR / QX / QY / QZ rows that no constraint touches
    // (lig_rows_explain_slots*, lig_rows_untouched_slots*, lig_hip.h).  slots: n_asked numbers row * l + column, strictly ascending;
    // slot_out: n_asked records; terms_out: the first term_cap term records in ascending (slot, constraint, coef_index) order (NULL with
    // term_cap = 0: slot_out and the counts only).  untouched_slots*: the first `cap` such slots in ascending order (NULL with cap = 0:
    // the counts only), nonzero_only: those with a nonzero committed value.
    // explain_slots() / untouched_slots(): the system given to set_linear_system, with the table of set_linear_values if one was set -- as
    // explain() does; a batcher with a prepared program or without a system has no term list: std::logic_error (the _attached forms).
    // explain_slots_attached() / untouched_slots_attached(): the statement attached to the trace, as explain_attached().
    // All after commit(), before or after prove(), until the next commit(); the same bytes for the same statement.  std::logic_error
    // before commit(), and on a batcher with shard_over(): a rank's share holds only the terms of its rows (the shard_ forms below).
    void explain_slots(const uint32_t* slots, uint64_t n_asked, lig_slot_record* slot_out, lig_slot_term* terms_out, uint64_t term_cap, lig_slot_info* info) {
        slots_ready("explain_slots", false);
        if (!info) throw std::invalid_argument("hip_row_batcher::explain_slots: null info");
        lig_linear_system sys = *linear_.get();
        if (values_set_) { sys.coefs = values_.data(); sys.n_coefs = values_.size() / 32; }
        info->struct_bytes = sizeof(lig_slot_info);
        check(lig_rows_explain_slots(trace_, &sys, slots, n_asked, slot_out, terms_out, term_cap, info), "lig_rows_explain_slots");
    }
    void explain_slots_attached(const uint32_t* slots, uint64_t n_asked, lig_slot_record* slot_out, lig_slot_term* terms_out, uint64_t term_cap,
                                lig_slot_info* info) {
        slots_ready("explain_slots_attached", true);
        if (!info) throw std::invalid_argument("hip_row_batcher::explain_slots_attached: null info");
        info->struct_bytes = sizeof(lig_slot_info);
        check(lig_rows_explain_slots_attached(trace_, slots, n_asked, slot_out, terms_out, term_cap, info), "lig_rows_explain_slots_attached");
    }
    void untouched_slots(bool nonzero_only, lig_slot_value* out, uint64_t cap, lig_untouched_info* info) {
        slots_ready("untouched_slots", false);
        if (!info) throw std::invalid_argument("hip_row_batcher::untouched_slots: null info");
        lig_linear_system sys = *linear_.get();
        if (values_set_) { sys.coefs = values_.data(); sys.n_coefs = values_.size() / 32; }
        info->struct_bytes = sizeof(lig_untouched_info);
        check(lig_rows_untouched_slots(trace_, &sys, nonzero_only ? 1 : 0, out, cap, info), "lig_rows_untouched_slots");
    }
    void untouched_slots_attached(bool nonzero_only, lig_slot_value* out, uint64_t cap, lig_untouched_info* info) {
        slots_ready("untouched_slots_attached", true);
        if (!info) throw std::invalid_argument("hip_row_batcher::untouched_slots_attached: null info");
        info->struct_bytes = sizeof(lig_untouched_info);
        check(lig_rows_untouched_slots_attached(trace_, nonzero_only ? 1 : 0, out, cap, info), "lig_rows_untouched_slots_attached");
    }
    // The four calls above for a batcher with shard_over(): lig_shard_rows_explain_slots* / lig_shard_rows_untouched_slots* (lig_hip.h),
    // COLLECTIVE calls over every rank's share -- the slots are those of the WHOLE trace, every rank passes the same arguments and gets the
    // bytes the unsharded batcher returns.  shard_explain_slots() / shard_untouched_slots(): the system given to set_linear_system with the
    // table of set_linear_values if one was set (a temporary share is made of it on every rank and released); the _attached forms: the
    // share attached to the shard, no term list.  Window as explain_slots(); std::logic_error before commit(), on an unsharded batcher
    // and without a linear system.
    void shard_explain_slots(const uint32_t* slots, uint64_t n_asked, lig_slot_record* slot_out, lig_slot_term* terms_out, uint64_t term_cap, lig_slot_info* info) {
        shard_slots_ready("shard_explain_slots", false);
        if (!info) throw std::invalid_argument("hip_row_batcher::shard_explain_slots: null info");
        lig_linear_system sys = *linear_.get();
        if (values_set_) { sys.coefs = values_.data(); sys.n_coefs = values_.size() / 32; }
        info->struct_bytes = sizeof(lig_slot_info);
        check(lig_shard_rows_explain_slots(shard_, &sys, slots, n_asked, slot_out, terms_out, term_cap, info), "lig_shard_rows_explain_slots");
    }
    void shard_explain_slots_attached(const uint32_t* slots, uint64_t n_asked, lig_slot_record* slot_out, lig_slot_term* terms_out, uint64_t term_cap,
                                      lig_slot_info* info) {
        shard_slots_ready("shard_explain_slots_attached", true);
        if (!info) throw std::invalid_argument("hip_row_batcher::shard_explain_slots_attached: null info");
        info->struct_bytes = sizeof(lig_slot_info);
        check(lig_shard_rows_explain_slots_attached(shard_, slots, n_asked, slot_out, terms_out, term_cap, info), "lig_shard_rows_explain_slots_attached");
    }
    void shard_untouched_slots(bool nonzero_only, lig_slot_value* out, uint64_t cap, lig_untouched_info* info) {
        shard_slots_ready("shard_untouched_slots", false);
        if (!info) throw std::invalid_argument("hip_row_batcher::shard_untouched_slots: null info");
        lig_linear_system sys = *linear_.get();
        if (values_set_) { sys.coefs = values_.data(); sys.n_coefs = values_.size() / 32; }
        info->struct_bytes = sizeof(lig_untouched_info);
        check(lig_shard_rows_untouched_slots(shard_, &sys, nonzero_only ? 1 : 0, out, cap, info), "lig_shard_rows_untouched_slots");
    }
    void shard_untouched_slots_attached(bool nonzero_only, lig_slot_value* out, uint64_t cap, lig_untouched_info* info) {
        shard_slots_ready("shard_untouched_slots_attached", true);
        if (!info) throw std::invalid_argument("hip_row_batcher::shard_untouched_slots_attached: null info");
        info->struct_bytes = sizeof(lig_untouched_info);
        check(lig_shard_rows_untouched_slots_attached(shard_, nonzero_only ? 1 : 0, out, cap, info), "lig_shard_rows_untouched_slots_attached");
    }
    // the next proof with this batcher: staging and (for the same row kinds) every device buffer of the trace are kept
    void reset(const hip_proof_meta* meta = nullptr) {
        if (pass_ == 2) throw std::logic_error("hip_row_batcher::reset between commit and prove");
        if (meta) meta_ = *meta;
        kinds_.clear();
        pass_ = 1; next_ = 0; enc_pos_ = 0; pushed_ = 0;
    }
    size_t rows() const { return kinds_.size(); }
    size_t local_rows() const { return sharded_ ? n_local_ : kinds_.size(); }
    // bytes of message rows the last commit() handed to the library (this rank's rows when sharded): what crosses the link
    size_t shipped_bytes() const { return shipped_; }

private:
    static constexpr size_t push_rows = 256;             // randomness rows per lig_rows_push_rands (64 MiB at k = 8192)

    bool same_shape(const lig_rows_job& job) const {           // lig_rows_restart keeps kinds, seeds and metadata of the trace
        if (kinds_ != shape_kinds_) return false;
        if (std::memcmp(meta_.encoding_seed, shape_meta_.encoding_seed, 32) || std::memcmp(meta_.program_hash, shape_meta_.program_hash, 32) ||
            meta_.generated_at != shape_meta_.generated_at || meta_.version != shape_meta_.version || meta_.public_args != shape_meta_.public_args) return false;
        const std::vector<uint8_t> w = job.elem_bytes ? std::vector<uint8_t>(job.elem_bytes, job.elem_bytes + kinds_.size()) : std::vector<uint8_t>();
        if (!(w == shape_widths_ || (w.empty() && shape_widths_.empty()))) return false;
        // (the record counts of mixed rows belong to the shape as the widths do)
        return (job.wide_per_row ? std::vector<uint32_t>(job.wide_per_row, job.wide_per_row + kinds_.size()) : std::vector<uint32_t>()) == shape_wide_;
    }
    void begin_pass2(size_t local_rows) {
        rands_.reserve(local_rows ? local_rows : 1, 0);
        present_.assign(kinds_.size(), 0);
        pass_ = 2; next_ = 0; enc_pos_ = 0; pushed_ = 0; n_present_ = 0; pushed_present_ = 0;  // the guest's second run starts the encoding stream over
    }
    // randomness rows [pushed_, upto) are complete: hand them to the library while the guest goes on.  Only the rows that HAVE a
    // randomness row are in the staging (packed) and go over the link; the library zero-fills the others on the device
    // (lig_rows_push_rands_sparse) -- batch rows never have one, quadratic rows often do not.
    bool has_linear() const { return linear_.is_set() || program_ != nullptr; }
    // explain_slots* / untouched_slots*: not sharded, after commit(), with the statement the entry reads
    void slots_ready(const char* what, bool attached) const {
        const std::string w = std::string("hip_row_batcher::") + what;
        if (sharded_) throw std::logic_error(w + ": not on a sharded batcher");
        if (pass_ == 1 || !trace_) throw std::logic_error(w + " before commit");
        if (attached && (!has_linear() || !linear_on_trace_)) throw std::logic_error(w + " without a linear system or program");
        if (!attached && !linear_.is_set()) throw std::logic_error(w + " without a linear system (the _attached form)");
    }
    // shard_explain_slots* / shard_untouched_slots*: sharded, after commit(), with the statement the entry reads
    void shard_slots_ready(const char* what, bool attached) const {
        const std::string w = std::string("hip_row_batcher::") + what;
        if (!sharded_) throw std::logic_error(w + ": not a sharded batcher (the call without shard_)");
        if (pass_ == 1 || !shard_) throw std::logic_error(w + " before commit");
        if (attached && (!has_linear() || !linear_on_trace_)) throw std::logic_error(w + " without a linear system");
        if (!attached && !linear_.is_set()) throw std::logic_error(w + " without a linear system");
    }
    void apply_linear() {
        if (!has_linear() || !(sharded_ ? (bool)shard_ : (bool)trace_)) return;
        if (!linear_on_trace_) {
            if (sharded_ && program_) throw std::logic_error("hip_row_batcher: a prepared linear program on a sharded batcher (set_linear_system)");
            if (sharded_) check(lig_shard_rows_set_linear(shard_, linear_.get()), "lig_shard_rows_set_linear");
            else if (program_) check(lig_rows_attach_linear(trace_, program_), "lig_rows_attach_linear");
            else check(lig_rows_set_linear(trace_, linear_.get()), "lig_rows_set_linear");
            linear_on_trace_ = true;
            values_on_trace_ = !values_set_;              // a fresh attachment reads the table it came with
        }
        if (!values_on_trace_) apply_values();
    }
    void apply_values() {                                 // (the trace / the shard keeps them across its restart)
        if (sharded_) check(lig_shard_rows_set_linear_values(shard_, values_set_ ? values_.data() : nullptr, values_.size() / 32), "lig_shard_rows_set_linear_values");
        else check(lig_rows_set_linear_values(trace_, values_set_ ? values_.data() : nullptr, values_.size() / 32), "lig_rows_set_linear_values");
        values_on_trace_ = true;
    }
    void push_rands(size_t upto) {
        if (sharded_ || upto <= pushed_ || has_linear()) return;
        check(lig_rows_push_rands_sparse(trace_, pushed_, upto - pushed_, present_.data() + pushed_, rands_.row(pushed_present_)), "lig_rows_push_rands_sparse");
        pushed_ = upto; pushed_present_ = n_present_;
    }
    void commit_sharded(lig_rows_job& job, uint8_t root[32], uint8_t stage1_seed[32]) {
        const size_t R = kinds_.size(), words = (size_t)k_ * 4;
        uint64_t rounds = 0;
        std::vector<uint64_t> b((size_t)world_ * ((R + 511) / 512 + 2) + 2);
        if (lig_shard_rows_plan(kinds_.data(), R, world_, &rounds, b.data(), b.size()) != LIG_OK) throw std::runtime_error("lig_shard_rows_plan failed");
        local_of_.assign(R, (size_t)-1);
        n_local_ = 0;
        // narrowest: the widths of ALL rows (every rank sees the same rows), this rank's rows packed in place behind the compaction
        // (derive_products without narrowest: the derived z rows leave the matrix, every other row stays full)
        std::vector<uint8_t> widths;
        std::vector<uint32_t> wide;
        if (meta_.narrow_rows && (meta_.narrowest || meta_.derive_products)) {
            if (plan_widths(widths, meta_.narrowest, wide)) {
                for (size_t r = 0; r < R; r++) if (widths[r] != 32) kinds_[r] |= LIG_ROW_DRAW_PAD;
                job.elem_bytes = widths.data();
                job.wide_per_row = wide.empty() ? nullptr : wide.data();
                job.reserved = LIG_ROWS_JOB_WIDE;
            }
        }
        uint8_t* out = reinterpret_cast<uint8_t*>(rows_.row(0));
        // this rank's rows, compacted IN PLACE to the front of the staging (commit order is kept, rows only move forward)
        for (uint64_t g = rank_; g < rounds * world_; g += world_)
            for (uint64_t r = b[g]; r < b[g + 1]; r++) {
                if (job.elem_bytes) out = pack_row(rows_.row(r), widths[r], out, wide.empty() ? 0 : wide[r]);
                else if (n_local_ != r) std::memmove(rows_.row(n_local_), rows_.row(r), words * 8);
                local_of_[r] = n_local_++;
            }
        job.msgs = n_local_ ? rows_.data() : nullptr;
        shipped_ = job.elem_bytes ? (size_t)(out - reinterpret_cast<uint8_t*>(rows_.row(0))) : n_local_ * words * 8;
        if (shard_) {                                      // the next proof of the same program: the shard's buffers and its share of the system are reused
            if (same_shape(job)) check(lig_shard_rows_restart(shard_, job.msgs, 0), "lig_shard_rows_restart");
            else { lig_shard_destroy(shard_); shard_ = nullptr; linear_on_trace_ = false; shard_derived_on_shard_ = shard_derived_.empty(); }
        }
        if (!shard_) check(lig_shard_rows_begin(ctx_, &job, rank_, world_, &comm_, &shard_), "lig_shard_rows_begin");
        shape_kinds_ = kinds_; shape_widths_ = job.elem_bytes ? widths : std::vector<uint8_t>(); shape_wide_ = wide; shape_meta_ = meta_;
        apply_linear();                                   // this rank's share of the system, under the commit
        if (!shard_derived_on_shard_) {                   // (... and its program of the derived slots: the shard keeps it across its restart)
            check(lig_shard_rows_set_derived(shard_, shard_derived_.empty() ? nullptr : shard_derived_sys_.get(), shard_derived_.empty() ? nullptr : shard_derived_.data(),
                                             shard_derived_.size(), nullptr), "lig_shard_rows_set_derived");
            shard_derived_on_shard_ = true;
        }
        check(lig_shard_rows_commit(shard_, root, stage1_seed), "lig_shard_rows_commit");
        for (auto& kd : kinds_) kd &= 0x7f;               // (pass 2 compares plain kinds)
        const size_t rand_rows = has_linear() ? 0 : n_local_;      // with a system no randomness row is staged (one scratch row for next_slot)
        begin_pass2(rand_rows);
        std::memset(rands_.row(0), 0, (rand_rows ? rand_rows : 1) * words * 8);     // batch rows and rows without a callback keep zero rows
    }
    // widths of all rows: a derived z row (derive_products) LIG_ELEM_PRODUCT, every other row ship_width() or, with narrow_others off,
    // 32; false = every row is full width (the plain format).  wide_slots (with narrowest): mixed_width() chooses instead of
    // ship_width(), `wide` = the records of every row -- left EMPTY when no row has any (and always without the option)
    bool plan_widths(std::vector<uint8_t>& widths, bool narrow_others, std::vector<uint32_t>& wide) const {
        const size_t R = kinds_.size();
        const bool mixed = narrow_others && meta_.narrowest && meta_.wide_slots;
        widths.assign(R ? R : 1, 32);
        wide.clear();
        if (mixed) wide.assign(R ? R : 1, 0);
        bool any = false, any_wide = false;
        for (size_t r = 0; r < R; r++) {
            widths[r] = meta_.derive_products && kinds_[r] == LIG_ROW_QZ ? (uint8_t)LIG_ELEM_PRODUCT : !narrow_others ? 32 : mixed ? mixed_width(r, &wide[r]) : ship_width(r);
            any = any || widths[r] != 32;
            any_wide = any_wide || (mixed && wide[r]);
        }
        if (!any_wide) wide.clear();
        return any;
    }
    // the smallest base index (0 bits, 1 .. 4 = 1, 2, 4, 8 bytes; 5 = none) slot `v` (4 u64) fits
    static unsigned slot_class(const uint64_t* v) {
        if (v[1] | v[2] | v[3]) return 5;
        return v[0] <= 1 ? 0 : v[0] <= 0xff ? 1 : v[0] <= 0xffff ? 2 : v[0] <= 0xffffffffu ? 3 : 4;
    }
    size_t narrow_bytes(uint8_t w) const { return w == LIG_ELEM_BIT ? ((size_t)l_ + 31) / 32 * 4 : ((size_t)l_ * w + 3) / 4 * 4; }
    // wide_slots: the base width of row r of the staging and its record count -- the base whose narrow row + 36 bytes per data slot
    // that does not fit it is the fewest bytes, the narrower base on a tie; 32 (no records) for batch rows and where the full row is
    // not more bytes (as mixed_widths of the Python binding)
    uint8_t mixed_width(size_t r, uint32_t* records) const {
        *records = 0;
        if (kinds_[r] > LIG_ROW_QZ) return 32;
        const uint64_t* rw = const_cast<hip_row_staging&>(rows_).row(r);
        size_t n_class[6] = {0, 0, 0, 0, 0, 0};
        for (uint32_t i = 0; i < l_; i++) n_class[slot_class(rw + 4 * i)]++;
        static const uint8_t base[5] = {LIG_ELEM_BIT, 1, 2, 4, 8};
        size_t best = (size_t)k_ * 32, misfit = l_;
        uint8_t w = 32;
        for (unsigned b = 0; b < 5; b++) {
            misfit -= n_class[b];                         // slots of a class above b
            const size_t cost = narrow_bytes(base[b]) + misfit * LIG_WIDE_RECORD_BYTES;
            if (cost < best) { best = cost; w = base[b]; *records = (uint32_t)misfit; }
        }
        if (w == 32) *records = 0;
        return w;
    }
    // the width row r of the staging is shipped in: 32 for batch rows and rows whose data slots need more than 8 bytes; else 8,
    // or with `narrowest` the smallest of bits / 1 / 2 / 4 / 8 bytes that holds every data slot (the OR of the slots decides)
    uint8_t ship_width(size_t r) const {
        if (kinds_[r] > LIG_ROW_QZ) return 32;
        const uint64_t* rw = const_cast<hip_row_staging&>(rows_).row(r);
        uint64_t lo = 0, hi = 0;
        for (uint32_t i = 0; i < l_ && !hi; i++) { lo |= rw[4 * i]; hi |= rw[4 * i + 1] | rw[4 * i + 2] | rw[4 * i + 3]; }
        if (hi) return 32;
        if (!meta_.narrowest) return 8;
        return lo <= 1 ? (uint8_t)LIG_ELEM_BIT : lo <= 0xff ? 1 : lo <= 0xffff ? 2 : lo <= 0xffffffffu ? 4 : 8;
    }
    // row `rw` (k x 4 u64) in the packed layout of width w written at `out` <= rw (the same staging: the write never overtakes
    // the read); returns the next row's start -- narrow rows take l x w bytes (bits: ceil(l / 8)) zero-padded to a multiple of 4,
    // derived rows nothing.  records > 0 (a mixed row): the slots that do not fit w are 0 in the narrow part and follow it as
    // {uint32 column, 32 bytes}, ascending -- collected before the narrow part is written over them; narrow part + records stay below
    // k x 32 bytes (mixed_width), so the next row of the staging is not reached
    uint8_t* pack_row(const uint64_t* rw, uint8_t w, uint8_t* out, uint32_t records = 0) const {
        if (w == LIG_ELEM_PRODUCT) return out;            // a derived row: nothing is shipped
        if (w == 32) {
            if ((const void*)out != (const void*)rw) std::memmove(out, rw, (size_t)k_ * 32);
            return out + (size_t)k_ * 32;
        }
        if (records) {
            const unsigned b = w == LIG_ELEM_BIT ? 0 : w == 1 ? 1 : w == 2 ? 2 : w == 4 ? 3 : 4;
            std::vector<uint8_t> rec((size_t)records * LIG_WIDE_RECORD_BYTES);
            std::vector<uint32_t> cols;
            for (uint32_t i = 0; i < l_; i++)
                if (slot_class(rw + 4 * i) > b) {
                    std::memcpy(rec.data() + cols.size() * LIG_WIDE_RECORD_BYTES, &i, 4);
                    std::memcpy(rec.data() + cols.size() * LIG_WIDE_RECORD_BYTES + 4, rw + 4 * i, 32);
                    cols.push_back(i);
                }
            if (cols.size() != records) throw std::logic_error("hip_row_batcher: a mixed row changed between planning and packing");
            uint64_t* w_rw = const_cast<uint64_t*>(rw);   // (the staging is ours: the slots that travel as records are 0 in the narrow part)
            for (uint32_t i : cols) w_rw[4 * i] = 0;
            uint8_t* end = pack_row(rw, w, out, 0);
            std::memcpy(end, rec.data(), rec.size());
            return end + rec.size();
        }
        size_t bytes = 0;
        if (w == LIG_ELEM_BIT) {
            for (uint32_t i = 0; i < l_; i += 8) {
                uint8_t v = 0;
                for (uint32_t j = 0; j < 8 && i + j < l_; j++) v |= (uint8_t)((rw[4 * (i + j)] & 1) << j);
                out[bytes++] = v;
            }
        } else {
            for (uint32_t i = 0; i < l_; i++) {
                const uint64_t v = rw[4 * i];
                std::memmove(out + bytes, &v, w);         // little endian host
                bytes += w;
            }
        }
        while (bytes % 4) out[bytes++] = 0;
        return out + bytes;
    }
    void check(int rc, const char* what) const {
        if (rc != LIG_OK) throw std::runtime_error(std::string(what) + ": " + lig_last_error(ctx_));
    }
    void row(uint8_t kind, const uint64_t* val, const uint64_t* rand, bool in_slot = false, bool slot_has_rand = true) {
        const size_t words = (size_t)k_ * 4;
        // witness_manager pads every linear row and every row of a quadratic triple with k - l stream elements when it forms
        // it (the rows arrive with their pads): the position of the next on_batch_init pad moves past them
        if (kind <= LIG_ROW_QZ) enc_pos_ += k_ - l_;
        if (pass_ == 1) {
            if (!val) throw std::invalid_argument("hip_row_batcher: null row");
            const size_t r = kinds_.size();
            if (!in_slot) { rows_.reserve(r + 1, r); std::memcpy(rows_.row(r), val, words * 8); }
            kinds_.push_back(kind);
        } else if (pass_ == 2) {
            // the guest is deterministic: pass 2 must replay the callbacks of pass 1 in the same order
            if (next_ >= kinds_.size() || kinds_[next_] != kind) throw std::logic_error("hip_row_batcher: pass 2 diverges from pass 1");
            if (has_linear()) {                                                  // the library forms the randomness rows: the replay is only counted
            } else if (sharded_) {                                                   // dense local matrix: only the rows of this rank's chunks are kept
                const size_t slot = local_of_[next_];
                if (slot != (size_t)-1 && !in_slot && rand) std::memcpy(rands_.row(slot), rand, words * 8);
            } else if (in_slot ? slot_has_rand : rand != nullptr) {                   // packed: this row takes the next slot
                if (!in_slot) std::memcpy(rands_.row(n_present_), rand, words * 8);
                present_[next_] = 1;
                n_present_++;
            }
            next_++;
            if (!sharded_ && next_ - pushed_ >= push_rows) push_rands(next_);
        } else throw std::logic_error("hip_row_batcher: callback after prove");
    }
    void dev_row(uint8_t kind, const void* dev) {
        if (pass_ == 1) {
            check(lig_sync(ctx_), "lig_sync");           // (lig_read is ordered on the context stream; kept explicit: the row must be final)
            const size_t r = kinds_.size();
            rows_.reserve(r + 1, r);
            check(lig_read(ctx_, rows_.row(r), dev, (size_t)k_ * 32), "lig_read(batch row)");
            row(kind, rows_.row(r), nullptr, true);
        } else row(kind, nullptr, nullptr);
    }

    static constexpr uint32_t init_pad = 192;            // params::sample_size (include/params.hpp:27)
    lig_ctx* ctx_;
    hip_proof_meta meta_, shape_meta_;
    uint32_t k_, l_;
    int pass_ = 1;
    size_t next_ = 0, pushed_ = 0, n_present_ = 0, pushed_present_ = 0;   // pass 2: rows replayed / pushed, rows with a randomness row seen / pushed
    std::vector<uint8_t> present_;
    uint64_t enc_pos_ = 0;                                // encoding-stream position (elements) of the next row's pad
    std::vector<uint8_t> kinds_, shape_kinds_, shape_widths_;
    std::vector<uint32_t> shape_wide_;                    // record counts of the mixed rows of the last commit (empty: none)
    hip_row_staging rows_, rands_;
    lig_trace* trace_ = nullptr;
    hip_linear_system_copy linear_;
    const lig_linear_program* program_ = nullptr;         // set_linear_program: the caller's object (linear_ is then unset)
    std::vector<uint8_t> values_;                         // set_linear_values
    hip_linear_system_copy derived_sys_;                  // set_derived_slots: the system the defining constraints are in
    std::vector<lig_derived_slot> derived_;
    bool derived_on_trace_ = true;                        // the trace holds the list above (no trace, no list: nothing to do)
    hip_linear_system_copy shard_derived_sys_;            // shard_set_derived_slots: the same three for a batcher with shard_over()
    std::vector<lig_derived_slot> shard_derived_;
    bool shard_derived_on_shard_ = true;
    bool values_set_ = false;
    bool linear_on_trace_ = false;                        // trace_ holds linear_ / program_ (it stays resident across lig_rows_restart)
    bool values_on_trace_ = false;                        // ... and the values of values_ (or, !values_set_, its own table)
    bool sharded_ = false;
    uint32_t rank_ = 0, world_ = 1;
    lig_comm comm_{};
    lig_shard* shard_ = nullptr;
    std::vector<size_t> local_of_;
    size_t n_local_ = 0, shipped_ = 0;
};

// The verifier's counterpart (src/webgpu_verifier.cpp:263-452 with nonbatch_verifier_context, nonbatch_context.hpp:1081-1388):
// the verifier runs the guest as well, its callbacks deliver the public randomness rows (the "value" rows it sees are the
// 192 opened elements it pops from the proof, which the library reads from the envelope itself).  One pass suffices when the
// caller derives stage1_seed first: begin(proof) -> seed -> run_program with the callbacks below -> finish(linear_sums).
class hip_row_verifier {
public:
    hip_row_verifier(lig_ctx* ctx, hip_proof_meta meta) : ctx_(ctx), meta_(std::move(meta)), k_(lig_padding_size(ctx)) {
        if (!ctx_) throw std::invalid_argument("hip_row_verifier: null context");
    }
    hip_row_verifier(const hip_row_verifier&) = delete;
    hip_row_verifier& operator=(const hip_row_verifier&) = delete;
    ~hip_row_verifier() { lig_vtrace_destroy(vt_); }          // begin without finish (the guest threw)

    // the row kinds of the public constraint stream, in commit order (a dry run of the guest, or the prover's kinds)
    void expect_rows(const std::vector<uint8_t>& kinds) { kinds_ = kinds; }
    // the public linear constraints as a sparse term list: finish(nullptr) then forms randomness matrix and constant itself -- no
    // run of the guest, nothing but the envelope and the public structure.  Before or after begin(); copied.
    void set_linear_system(const lig_linear_system& sys) {
        linear_.assign(sys);
        program_ = nullptr; values_set_ = false;
        if (vt_ && lig_rows_verify_set_linear(vt_, linear_.get()) != LIG_OK) throw std::runtime_error(std::string("lig_rows_verify_set_linear: ") + lig_last_error(ctx_));
    }
    // the same with a structure prepared once (lig_linear_prepare): a verifier service prepares per program, not per envelope.  Not
    // copied and not owned: the caller keeps its reference while this verifier may still begin() with it.  nullptr removes it.
    void set_linear_program(const lig_linear_program* p) {
        linear_.clear();
        program_ = p; values_set_ = false;
        if (vt_ && lig_rows_verify_attach_linear(vt_, p) != LIG_OK) throw std::runtime_error(std::string("lig_rows_verify_attach_linear: ") + lig_last_error(ctx_));
    }
    // the values of the coefficient table of the statement to verify (lig_rows_verify_set_linear_values): the public right-hand
    // sides are part of the statement.  Copied; kept for the envelopes that follow until set again; nullptr: the structure's own table.
    void set_linear_values(const uint8_t* coefs, uint64_t n_coefs) {
        if (!has_linear()) throw std::logic_error("hip_row_verifier::set_linear_values without a linear system or program");
        values_set_ = coefs != nullptr;
        values_.assign(coefs, coefs + (coefs ? n_coefs * 32 : 0));
        if (vt_) apply_values();
    }
    // parse the envelope, re-derive both seeds and the sample indices; false: malformed envelope / wrong indices (reject)
    bool begin(const uint8_t* proof, size_t len, uint8_t stage1_seed[32], lig_verify_info* info = nullptr) {
        std::vector<uint8_t> args;
        std::vector<uint64_t> lens;
        for (const auto& a : meta_.public_args) { args.insert(args.end(), a.begin(), a.end()); lens.push_back(a.size()); }
        lig_rows_job job;
        std::memset(&job, 0, sizeof job);
        job.rows = kinds_.size();
        job.kinds = kinds_.data();
        job.public_args = args.empty() ? nullptr : args.data();
        job.public_arg_lens = lens.empty() ? nullptr : lens.data();
        job.n_public_args = lens.size();
        lig_verify_info local;
        const int rc = lig_rows_verify_begin(ctx_, &job, proof, len, &vt_, stage1_seed, info ? info : &local);
        if (rc != LIG_OK) throw std::runtime_error(std::string("lig_rows_verify_begin: ") + lig_last_error(ctx_));
        if (vt_ && linear_.is_set() && lig_rows_verify_set_linear(vt_, linear_.get()) != LIG_OK)
            throw std::runtime_error(std::string("lig_rows_verify_set_linear: ") + lig_last_error(ctx_));
        if (vt_ && program_ && lig_rows_verify_attach_linear(vt_, program_) != LIG_OK)
            throw std::runtime_error(std::string("lig_rows_verify_attach_linear: ") + lig_last_error(ctx_));
        if (vt_ && has_linear() && values_set_) apply_values();
        if (!has_linear()) rands_.assign(kinds_.size() * (size_t)k_ * 4, 0);
        next_ = 0;
        return vt_ != nullptr;
    }
    void linear_callback(const uint64_t* rand) { row(LIG_ROW_LINEAR, rand); }
    void quadratic_callback(const uint64_t* x_rand, const uint64_t* y_rand, const uint64_t* z_rand) { row(LIG_ROW_QX, x_rand); row(LIG_ROW_QY, y_rand); row(LIG_ROW_QZ, z_rand); }
    void on_batch_init() { row(LIG_ROW_INIT, nullptr); }
    void on_batch_bit() { row(LIG_ROW_BIT, nullptr); }
    void on_batch_equal() { row(LIG_ROW_EQX, nullptr); row(LIG_ROW_EQY, nullptr); }
    void on_batch_quadratic() { row(LIG_ROW_BQX, nullptr); row(LIG_ROW_BQY, nullptr); row(LIG_ROW_BQZ, nullptr); }
    // the seven predicates of webgpu_verifier.cpp:412-442; returns accept
    bool finish(const uint8_t const_sum[32], lig_verify_info* info = nullptr) {
        if (!vt_) throw std::logic_error("hip_row_verifier::finish without a successful begin");
        const bool linear = has_linear();
        if (!linear && next_ != kinds_.size()) throw std::logic_error("hip_row_verifier::finish: fewer rows replayed than expected");
        lig_verify_info local;
        lig_verify_info* o = info ? info : &local;
        lig_vtrace* vt = vt_;
        vt_ = nullptr;                                        // finish frees the trace
        if (lig_rows_verify_finish(vt, linear ? nullptr : rands_.data(), 0, const_sum, o) != LIG_OK) throw std::runtime_error(std::string("lig_rows_verify_finish: ") + lig_last_error(ctx_));
        return o->accept != 0;
    }

private:
    bool has_linear() const { return linear_.is_set() || program_ != nullptr; }
    void apply_values() {
        if (lig_rows_verify_set_linear_values(vt_, values_set_ ? values_.data() : nullptr, values_.size() / 32) != LIG_OK)
            throw std::runtime_error(std::string("lig_rows_verify_set_linear_values: ") + lig_last_error(ctx_));
    }
    void row(uint8_t kind, const uint64_t* rand) {
        if (next_ >= kinds_.size() || (kinds_[next_] & 0x7f) != kind) throw std::logic_error("hip_row_verifier: the guest diverges from the expected row kinds");
        if (rand && !has_linear()) std::memcpy(rands_.data() + next_ * (size_t)k_ * 4, rand, (size_t)k_ * 32);
        next_++;
    }
    lig_ctx* ctx_;
    hip_proof_meta meta_;
    uint32_t k_;
    size_t next_ = 0;
    std::vector<uint8_t> kinds_;
    std::vector<uint64_t> rands_;
    hip_linear_system_copy linear_;
    const lig_linear_program* program_ = nullptr;
    std::vector<uint8_t> values_;
    bool values_set_ = false;
    lig_vtrace* vt_ = nullptr;
};

}  // namespace ligero
