// prover.hip -- batched three-stage Ligero prover over a resident witness matrix, host side.
//
// MI355X-native counterpart of the orchestration in src/webgpu_prover.cpp:226-494 and the stage contexts of
// include/zkp/nonbatch_context.hpp (stage 1 :445-558, stage 2 :654-780, stage 3 :924-1000).  The reference
// streams one row at a time through the executor and re-runs the guest program (and therefore re-encodes every
// row) three times because a WebGPU device cannot hold the witness matrix.  With 288 GB of HBM the matrix is at
// rest: every message row is encoded ONCE in stage 1, the codewords (1 MiB per row) stay resident and are re-used
// by the stage-2 accumulators and the stage-3 column gather; only the dense stage-2 randomness rows need a second
// encode.  Transcript bytes (seeds, sample indices, Merkle decommitment, protobuf envelope) follow the reference
// byte for byte, so an unmodified verifier accepts the proof.
//
// The guest interpreter / constraint generator is out of scope; rows come from the synthetic
// constraint stream of BASELINE.md 3: n_linear witness slots + n_quad slots of x*y=z, one dense linear-test
// coefficient per witness.
#include "prover_common.hpp"
#include "upload.hpp"
#include <cerrno>
#include <functional>

struct lig_trace {
    lig_ctx* c = nullptr;
    lig_synth_job job;                  // synthetic jobs only (n_linear / n_quad / witness_key); pointers cleared
    bool from_rows = false;             // rows supplied by the caller (lig_rows_*): no witness generation here
    bool loaded = false, committed = false;   // lig_rows_*: rows for the next commit are loaded / stage 1 done, proof pending
    bool dense_rands = false;           // lig_rows_job.dense_rands_per_row given: randomness rows may be generated here
    bool diag_ok = false;               // `msgs` holds a committed trace (lig_rows_diagnose): from lig_rows_commit until the matrix is replaced
    fr* msgs_alt = nullptr;             // second message matrix: the next trace is uploaded while the current one is proved
    bool alt_pending = false;           // the rows for the next commit are (arriving) in msgs_alt
    JobHeader hdr;
    std::vector<RowDesc> rows;          // committed non-mask rows in commit order
    std::vector<PadRun> pad_runs;       // pads drawn at commit time (pad_encoding_random), runs of consecutive rows
    uint64_t mask_pos = 0;              // encoding-stream position of the first mask element
    std::vector<std::pair<size_t, size_t>> sched1;     // stage-1 chunk schedule
    const uint8_t* host_msgs = nullptr; // lig_rows_begin with host memory: uploaded chunk by chunk under the encodes
    std::vector<hipEvent_t> ev_up;      // one per stage-1 chunk: its rows have arrived (per-context copy stream, LIG_UPLOAD_MODE=1)
    FlagPage flags;                     // pinned: word ci = sequence number of the last upload whose chunk ci has arrived; then the words of flag_layout()
    UploadLane up, rand;                // witness rows (what stage 1 waits for) | randomness rows, kept apart: a restart between commit and prove must not move what
                                        // the next commit waits for, and lig_rows_prove must not wait for (or swallow the error of) the NEXT trace's witness prefetch
    bool up_by_thread = false;
    fr* rands_full = nullptr;           // lig_rows_push_rands / lig_rows_set_linear: R x k, device resident
    lig_linear* linear = nullptr;       // lig_rows_set_linear: the sparse linear system, regrouped by slot (linear.hip); survives lig_rows_restart
    lig_derive* derive = nullptr;       // lig_rows_set_derived: the slots stage 1 forms from their defining constraints (derive.hip); survives lig_rows_restart
    uint64_t rands_pushed = 0;          // rows handed to the uploader so far (the page's push word counts the rows that have ARRIVED)
    bool push_sync = false;             // lig_rows_push_rands without an uploader thread: the pushed rows were copied synchronously
    std::vector<UploadJob> push_log;    // the pushes of the committed trace (their host rows stay valid until lig_rows_prove returns): what a retry copies again
    bool up_retry = false;              // prove_stage1 failed because a witness-rows transfer timed out (LIG_UPLOAD_TIMEOUT_S): lig_rows_commit makes the upload again
    bool leak = false;                  // an abandoned transfer of this trace is still pending and cannot be cancelled: its buffers are never freed or reused
    std::atomic<int> up_abort{0};       // a failed lig_rows_prove: the uploader drops the randomness-row copies it still holds
    // narrow row format (lig_rows_job.elem_bytes): packed byte offset of every row (+1 entry), the device staging
    // area the packed rows are uploaded to (expanded into `msgs` chunk by chunk in stage 1)
    bool narrow = false;
    std::vector<uint64_t> src_off;
    std::vector<uint8_t> widths;        // elem_bytes of every row (32 for a full-width row): what lig_rows_set_derived checks its list against
    uint64_t* src_off_dev = nullptr; uint8_t* widths_dev = nullptr; uint8_t* packed_dev = nullptr;
    ProductRows prod;                   // derived rows (LIG_ELEM_PRODUCT): formed next to the expansion from the packed x and y rows
    WideRows wide;                      // mixed rows (lig_rows_job.wide_per_row): their records are written behind the expansion
    uint32_t* h_wide_flag = nullptr;    // pinned: the flag word of the records of DEVICE rows, read by lig_rows_commit with the root
    lig_proof_info info1;               // stage-1 results kept between lig_rows_commit and lig_rows_prove
    size_t R = 0, RB = 0, n_init = 0;   // all rows, leading rows committed by the batch program, of those: init rows
    fr* msgs = nullptr;                 // R x k witness matrix (pads are re-drawn by every prove)
    // [stage-1 chunks: rows arrived | stage-2 chunks: randomness rows arrived | ... consumed]; n_chunks of the stage-2 schedule
    lig::FlagLayout flag_layout(size_t n_chunks = 0) const { return lig::trace_flags(sched1.size(), R, lig_tune::CHUNK, n_chunks); }
    bool zres = false;                  // LIG_ZRES: `cw` holds the encoder's Z tiles (lig::ENC_ZRES) instead of planes -- K3 runs inside the column hash,
                                        // stage 2 / 3 take single radix-8 outputs from the tiles (linear rows only: a trace with quadratic triples keeps planes)
    fr* cw = nullptr;                   // R x 3k: cosets 1..3 of every codeword as planes (lig::ENC_PLANAR), resident across the stages;
                                        // coset 0 of a codeword is its message row reversed and is read from `msgs` (lig::CwView)
    fr* maskcw = nullptr;               // 3 x n: the mask rows' codewords, reference layout
    fr* randb = nullptr;                // chunk x k randomness rows
    fr* rcw = nullptr;                  // chunk x n their codewords
    fr* acc = nullptr;                  // code | lin | quad | tmp   (4 x n)
    fr* parts = nullptr;                // 2 x groups x n partial accumulators
    fr* dots = nullptr;                 // one element: a device-side sum (mask closing slot, linear-test constant)
    fr* samples = nullptr;              // (R+3) x t
    uint32_t* sha_state = nullptr; uint32_t* leaves = nullptr; uint32_t* nodes = nullptr;
    uint32_t* tri_dev = nullptr;
    lig::f29s* coef_dev = nullptr;      // rc (R) | rq2 (T) | rq1 (T)
    std::vector<uint32_t> triples;
    uint8_t* h_proof = nullptr; size_t h_proof_cap = 0;   // pinned: the envelope is assembled here (owned by the trace)
    uint8_t* h_enc = nullptr;                              // pinned: 3 x n accumulators
    uint8_t* h_nodes = nullptr;                            // pinned: Merkle nodes
    hipEvent_t ev_ready[2] = {nullptr, nullptr}, ev_used[2] = {nullptr, nullptr};   // double-buffered randomness rows
    hipEvent_t ev_gate = nullptr, ev_k1 = nullptr, ev_acc[3] = {nullptr, nullptr, nullptr};
    uint8_t* h_small = nullptr;                            // pinned: the device-side sum (32 B) | 3 decoded accumulators (3 x n x 32)
};

// Host waits of a proof (root of stage 1, the three accumulators, the decodes, the envelope).  The runtime's blocking waits sleep on an
// interrupt: every wake-up costs tens of microseconds during which the GPU has nothing of this proof to run.  LIG_SPIN_WAIT=1 (default)
// polls instead (the calling thread yields between polls for LIG_SPIN_WAIT_MS, then falls back on the blocking wait): A/B in
// profiles/r05_spin_wait_ab.md.
template <class Query, class Sync> static hipError_t spin_wait(Query query, Sync sync) {
    if (!lig::knobs().spin_wait) return sync();
    const auto t0 = clk::now();
    for (unsigned spins = 0;; spins++) {
        const hipError_t e = query();
        if (e != hipErrorNotReady) return e;
        std::this_thread::yield();
        if ((spins & 255) == 255 && ms_since(t0) > (double)lig::knobs().spin_wait_ms) return sync();
    }
}
static hipError_t wait_stream(hipStream_t st) { return spin_wait([st] { return hipStreamQuery(st); }, [st] { return hipStreamSynchronize(st); }); }
static hipError_t wait_event(hipEvent_t ev) { return spin_wait([ev] { return hipEventQuery(ev); }, [ev] { return hipEventSynchronize(ev); }); }
hipError_t lig_internal_wait_stream(hipStream_t st) { return wait_stream(st); }      // (diagnose.hip waits the way a proof does)

// The batch program on the device (lig_hip.h, lig_batch_op): k-element variables in a slab, every operation one eltwise
// kernel into a temporary + a copy (as vbn254fr_module does), every hook a device-to-device copy of the rows it names
// into the witness matrix.  The padding of an initialised variable comes from the encoding stream, 192 draws per init
// in program order (pad_encoding_random, nonbatch_context.hpp:497-510).
int lig_run_batch_program(lig_ctx* c, const lig_synth_job& job, fr* rows_out) {
    const uint32_t l = c->l, k = c->k, pad = k - l;
    hipStream_t s = c->stream;
    uint32_t nvars = 1;
    for (uint64_t i = 0; i < job.n_batch_ops; i++) {
        const lig_batch_op& o = job.batch_ops[i];
        nvars = std::max(nvars, std::max(o.out, std::max(o.x, o.y)) + 1);
        if (o.op == LIG_BOP_BIT_DECOMPOSE)
            for (uint32_t b = 0; b < o.len; b++) { uint32_t slot; std::memcpy(&slot, job.batch_data + o.data_off + 4ull * b, 4); nvars = std::max(nvars, (slot & 511u) + 1); }
    }
    fr* vars = nullptr; fr* tmp = nullptr;
    HIP_TRY(c, hipMalloc((void**)&vars, (size_t)nvars * k * sizeof(fr)));
    struct Free { fr*& a; fr*& b; lig_ctx* c; ~Free() { (void)hipStreamSynchronize(c->stream); (void)hipFree(a); (void)hipFree(b); } } guard{vars, tmp, c};
    HIP_TRY(c, hipMalloc((void**)&tmp, (size_t)k * sizeof(fr)));
    HIP_TRY(c, hipMemsetAsync(vars, 0, (size_t)nvars * k * sizeof(fr), s));
    uint32_t rk[60];
    lig::aes256_expand_host(job.encoding_seed, rk);
    HIP_TRY(c, hipMemcpyAsync(c->rk_dev, rk, sizeof rk, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const size_t vb = (size_t)k * sizeof(fr);
    size_t r = 0, inits = 0;
    auto var = [&](uint32_t i) { return vars + (size_t)i * k; };
    auto commit = [&](const fr* src) -> int { HIP_TRY(c, hipMemcpyAsync(rows_out + (r++) * (size_t)k, src, vb, hipMemcpyDeviceToDevice, s)); return LIG_OK; };
    auto to_out = [&](uint32_t out) -> int { HIP_TRY(c, hipMemcpyAsync(var(out), tmp, vb, hipMemcpyDeviceToDevice, s)); return LIG_OK; };
    std::vector<uint8_t> stage;
    bool compat = false;                 // LIG_BOP_UPSTREAM_COMPAT seen: slices as upstream defines them (lig_hip.h)
    for (uint64_t i = 0; i < job.n_batch_ops; i++) {
        const lig_batch_op& o = job.batch_ops[i];
        const uint8_t* data = job.batch_data ? job.batch_data + o.data_off : nullptr;
        switch (o.op) {
            case LIG_BOP_UPSTREAM_COMPAT: compat = true; break;
            case LIG_BOP_SET: case LIG_BOP_SET_SCALAR: {
                const bool limbs = (o.reserved & LIG_BOP_F_WRITE_LIMBS) != 0;           // write_limbs family: write_buffer only
                const uint32_t len = o.op == LIG_BOP_SET ? o.len : l;
                stage.assign(32ull * len, 0);
                if (o.op == LIG_BOP_SET) std::memcpy(stage.data(), data, 32ull * o.len);
                else for (uint32_t e = 0; e < l; e++) std::memcpy(stage.data() + 32ull * e, data, 32);
                if (!limbs && !compat) HIP_TRY(c, hipMemsetAsync(var(o.x), 0, vb, s));  // write_buffer_clear, declared slice: the rest of x
                if (len) HIP_TRY(c, hipMemcpyAsync(var(o.x), stage.data(), 32ull * len, hipMemcpyHostToDevice, s));
                HIP_TRY(c, hipStreamSynchronize(s));                                    // `stage` is reused
                // write_buffer_clear as upstream runs it: clear_buffer(x.slice(len * 32)) after the write, the slice being
                // {offset len*32, size X + k*32 - len*32} of the slab: elements [len, x*k + k)
                if (!limbs && compat) HIP_TRY(c, hipMemsetAsync(vars + len, 0, ((size_t)o.x * k + k - len) * sizeof(fr), s));
                // on_batch_init's pad: x's own pad slots (declared) / slab element l = variable 0's pad slots (upstream)
                lig::launch_rng_fill_rows(s, c->rk_dev, (uint64_t)(inits++) * pad, compat ? vars : var(o.x), 1, pad, k, l, 1, pad);
                TRY(commit(var(o.x)));
                break;
            }
            case LIG_BOP_COPY:
                if (o.out != o.x) HIP_TRY(c, hipMemcpyAsync(var(o.out), var(o.x), vb, hipMemcpyDeviceToDevice, s));
                TRY(commit(var(o.out))); TRY(commit(var(o.x)));
                break;
            case LIG_BOP_ADD: TRY(lig_eltwise(c, LIG_OP_ADD, var(o.x), var(o.y), tmp, k, nullptr, 0)); TRY(to_out(o.out)); break;
            case LIG_BOP_SUB: TRY(lig_eltwise(c, LIG_OP_SUB, var(o.x), var(o.y), tmp, k, nullptr, 0)); TRY(to_out(o.out)); break;
            case LIG_BOP_MUL:
                TRY(lig_eltwise(c, LIG_OP_MUL, var(o.x), var(o.y), tmp, k, nullptr, 0));
                TRY(commit(var(o.x))); TRY(commit(var(o.y))); TRY(commit(tmp));
                TRY(to_out(o.out));
                break;
            case LIG_BOP_DIV:
                TRY(lig_eltwise(c, LIG_OP_DIV, var(o.x), var(o.y), tmp, k, nullptr, 0));
                TRY(commit(tmp)); TRY(commit(var(o.y))); TRY(commit(var(o.x)));
                TRY(to_out(o.out));
                break;
            case LIG_BOP_ADD_CONST: case LIG_BOP_SUB_CONST: case LIG_BOP_CONST_SUB: case LIG_BOP_MUL_CONST: case LIG_BOP_MONTMUL_CONST: {
                static const int map[5] = {LIG_OP_ADD_CONST, LIG_OP_SUB_CONST, LIG_OP_CONST_SUB, LIG_OP_MUL_CONST, LIG_OP_MONTMUL_CONST};
                TRY(lig_eltwise(c, map[o.op - LIG_BOP_ADD_CONST], var(o.x), nullptr, tmp, k, data, 0));
                TRY(to_out(o.out));
                break;
            }
            case LIG_BOP_ASSERT_EQUAL: TRY(commit(var(o.x))); TRY(commit(var(o.y))); break;
            case LIG_BOP_BIT_DECOMPOSE:
                for (uint32_t b = 0; b < o.len; b++) {
                    uint32_t slot;
                    std::memcpy(&slot, data + 4ull * b, 4);
                    slot &= 511u;
                    TRY(lig_eltwise(c, LIG_OP_BIT_DECOMPOSE, var(o.x), nullptr, tmp, k, nullptr, b));
                    TRY(to_out(slot));
                    TRY(commit(var(slot)));
                }
                break;
            case LIG_BOP_FREE: HIP_TRY(c, hipMemsetAsync(var(o.x), 0, vb, s)); break;
            default: break;
        }
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    return LIG_OK;
}

int lig_internal_synth_witness(lig_ctx* c, const uint8_t witness_key[32], const std::vector<RowDesc>& rows, size_t first, fr* msgs) {
    const uint32_t k = c->k;
    uint32_t rk[60];
    lig::aes256_expand_host(witness_key, rk);
    TRY(lig_internal_upload_small(c, c->rk_dev, rk, sizeof rk, c->stream));
    uint64_t pos = 0;
    const size_t R = rows.size();
    for (size_t r = first; r < R;) {
        const RowDesc d = rows[r];
        if (d.kind == 0) {                      // run of linear rows with the same fill
            size_t run = 1;
            while (r + run < R && rows[r + run].kind == 0 && rows[r + run].data == d.data) run++;
            lig::launch_rng_fill_rows(c->stream, c->rk_dev, pos, msgs + r * k, run, d.data, k, 0, 1, d.data);
            pos += (uint64_t)run * d.data; r += run;
        } else {                                 // x, y, z triple
            lig::launch_rng_fill_rows(c->stream, c->rk_dev, pos, msgs + r * k, 2, d.data, k, 0, 1, d.data);
            pos += 2ull * d.data;
            lig::launch_eltwise(c->stream, LIG_OP_MUL, msgs + r * k, msgs + (r + 1) * k, msgs + (r + 2) * k, d.data, fr{}, 0);
            r += 3;
        }
    }
    HIP_TRY(c, hipGetLastError());
    return LIG_OK;
}

int lig_internal_form_mask_rows(lig_ctx* c, hipStream_t s, uint64_t epos, fr* mask, fr* dots) {
    const uint32_t l = c->l, n = c->n, pad = c->k - l;
    HIP_TRY(c, hipMemsetAsync(mask, 0, 3 * (size_t)n * 32, s));
    lig::launch_rng_fill_rows(s, c->rk_dev, epos, mask, 1, l, 0, 0, 1, 0); epos += l;               // code mask: l randoms, zeros to k
    fr* mlin = mask + n; fr* mquad = mask + 2 * (size_t)n;
    lig::launch_rng_fill_rows(s, c->rk_dev, epos, mlin, 1, l - 1, 0, 1, 2, 0); epos += l - 1;       // (0, r) x (l-1)
    // last odd slot = -(sum of the others) (witness_manager.hpp:283-297), on the device: no host round trip
    lig::launch_sum_elems(s, mlin + 1, l - 1, 2, dots, mlin + 2 * (size_t)(l - 1) + 1);
    lig::launch_rng_fill_rows(s, c->rk_dev, epos, mlin, 1, 2 * pad, 0, 2 * l, 1, 0); epos += 2 * pad;
    lig::launch_rng_fill_rows(s, c->rk_dev, epos, mquad, 1, l, 0, 1, 2, 0); epos += l;              // (0, r) x l
    lig::launch_rng_fill_rows(s, c->rk_dev, epos, mquad, 1, 2 * pad, 0, 2 * l, 1, 0);
    return LIG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// shared by lig_synth_* and lig_rows_*: buffers of a trace whose row plan (T->rows) is known
static int trace_alloc(lig_ctx* c, lig_trace* T) {
    const uint32_t k = c->k, n = c->n, t = 192;
    const size_t R = T->R = T->rows.size();
    T->triples = quad_terms(T->rows);
    T->zres = lig::knobs().zres && c->fast && T->triples.empty();
    const size_t chunk = lig_tune::CHUNK, groups = (chunk + lig_tune::GROUP - 1) / lig_tune::GROUP;
    auto dm = [&](void** p, size_t bytes) -> int { HIP_TRY(c, hipMalloc(p, bytes ? bytes : 16)); HIP_TRY(c, hipMemsetAsync(*p, 0, bytes, c->stream)); return LIG_OK; };
    TRY(dm((void**)&T->msgs, (R ? R : 1) * (size_t)k * 32));
    TRY(dm((void**)&T->cw, (R ? R : 1) * 3 * (size_t)k * 32));
    TRY(dm((void**)&T->maskcw, 3 * (size_t)n * 32));
    TRY(dm((void**)&T->randb, 2 * chunk * (size_t)k * 32));          // double-buffered
    TRY(dm((void**)&T->rcw, chunk * (size_t)n * 32));
    TRY(dm((void**)&T->acc, 4 * (size_t)n * 32));
    TRY(dm((void**)&T->parts, (2 * groups * (size_t)n + (chunk + lig_tune::DOT_GROUP - 1) / lig_tune::DOT_GROUP * k) * 32));
    TRY(dm((void**)&T->dots, 32));
    TRY(dm((void**)&T->samples, (R + 3) * (size_t)t * 32));
    TRY(dm((void**)&T->sha_state, lig_sha_state_bytes(n)));
    TRY(dm((void**)&T->leaves, (size_t)n * 32));
    TRY(dm((void**)&T->nodes, lig_merkle_nodes(n) * 32));
    TRY(dm((void**)&T->tri_dev, (T->triples.size() ? T->triples.size() : 1) * sizeof(uint32_t)));
    TRY(dm((void**)&T->coef_dev, (R + 2 * T->triples.size() / 3 + 1) * sizeof(lig::f29s)));
    T->h_proof_cap = (size_t)1 << 19;
    T->h_proof_cap += 3 * (size_t)n * 32 + (R + 3) * (size_t)t * 32;
    HIP_TRY(c, hipHostMalloc((void**)&T->h_proof, T->h_proof_cap, hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc((void**)&T->h_enc, 3 * (size_t)n * 32, hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc((void**)&T->h_nodes, lig_merkle_nodes(n) * 32, hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc((void**)&T->h_small, (1 + 3 * (size_t)n) * 32, hipHostMallocDefault));
    for (int i = 0; i < 2; i++) {
        HIP_TRY(c, hipEventCreateWithFlags(&T->ev_ready[i], hipEventDisableTiming));
        HIP_TRY(c, hipEventCreateWithFlags(&T->ev_used[i], hipEventDisableTiming));
    }
    HIP_TRY(c, hipEventCreateWithFlags(&T->ev_gate, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&T->ev_k1, hipEventDisableTiming));
    for (int a3 = 0; a3 < 3; a3++) HIP_TRY(c, hipEventCreateWithFlags(&T->ev_acc[a3], hipEventDisableTiming));
    if (!T->triples.empty()) HIP_TRY(c, hipMemcpyAsync(T->tri_dev, T->triples.data(), T->triples.size() * 4, hipMemcpyHostToDevice, c->stream));
    {   // a short first chunk (the column hash -- the longest chain of stage 1 -- starts after 128 rows instead of 512) and a short
        // last one (the hash tail after the last encode); LIG_S1_HEAD / LIG_S1_TAIL override for experiments
        // (profiles/r02_stage1_schedule_ab.md: head 128 is +3 % proofs/s with two proofs in flight; one stage 1 at a time -- a
        // process-wide lock around this stage -- measured 3-5 % slower)
        T->sched1 = chunk_schedule(R, lig_tune::CHUNK, lig::knobs().s1_head, lig::knobs().s1_tail);
    }
    TRY(lig_internal_reserve_scratch(c, R < lig_tune::CHUNK ? (R ? R : 1) : lig_tune::CHUNK));     // sized once: never re-allocated under a running stream
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return LIG_OK;
}

// (the brackets of lig_profile_*, lig_capi.hip, for a launch this file makes)
int lig_internal_profile_bracket(lig_ctx* c, uint32_t rows, hipEvent_t* e0, hipEvent_t* e1) {
    *e0 = *e1 = nullptr;
    if (!c->prof_on) return LIG_OK;
    if (c->prof_used == c->prof_events.size()) {
        hipEvent_t a, b;
        HIP_TRY(c, hipEventCreate(&a)); HIP_TRY(c, hipEventCreate(&b));
        c->prof_events.push_back({a, b});
    }
    *e0 = c->prof_events[c->prof_used].first; *e1 = c->prof_events[c->prof_used].second;
    if (c->prof_launch_rows.size() < c->prof_used + 1) c->prof_launch_rows.resize(c->prof_used + 1);
    c->prof_launch_rows[c->prof_used] = rows;
    c->prof_used++; c->prof_rows += rows;
    return LIG_OK;
}
// ================= stage 1: row forming (pads + masks from the encoding stream), encode, column hash, Merkle root
static int prove_stage1(lig_trace* T, lig_proof_info* info, const std::function<void(const char*)>& mark) {
    lig_ctx* c = T->c;
    const uint32_t l = c->l, k = c->k, n = c->n, pad = k - l;
    const size_t k3 = 3 * (size_t)k;
    hipStream_t s = c->stream;
    uint32_t rk[60];
    lig::aes256_expand_host(T->hdr.encoding_seed, rk);
    TRY(lig_internal_upload_small(c, c->rk_dev, rk, sizeof rk, s));
    const bool streamed = T->host_msgs != nullptr;       // rows arrive chunk by chunk: their pads are drawn per chunk below
    if (!streamed)
        for (const PadRun& pr : T->pad_runs)             // pad_encoding_random of every row that draws at commit time
            lig::launch_rng_fill_rows(s, c->rk_dev, pr.pos, T->msgs + pr.first * (size_t)k, pr.count, pad, k, l, 1, pad);
    mark("  pads");
    fr* mask = T->maskcw; fr* mlin = mask + n;                                                      // the 3 mask rows are formed in place
    TRY(lig_internal_form_mask_rows(c, s, T->mask_pos, mask, T->dots));
    mark("row forming (pads, masks)");
    // Encode chunk by chunk on the main stream; the column hash of chunk b runs on the side stream while chunk
    // b+1 is being encoded (the hash has only n = 32768 lanes of parallelism -- 512 waves -- and would otherwise
    // leave most of the chip idle for its whole duration).  Row order = hash order is preserved by stream order.
    hipStream_t s2 = c->stream2;
    // (dedicated CUs for the hash via CU-masked streams were measured with one proof: no gain, profiles/r01_overlap_experiments.md;
    // LIG_SHA_CUMASK: disjoint halves for the hashes of two proofs in flight, profiles/r04_sha_cumask_ab.md)
    hipStream_t s_sha = c->stream_sha ? c->stream_sha : s2, s_enc = s;
    TRY(lig_sha_init(c, T->sha_state, n));
    HIP_TRY(c, hipEventRecord(c->ev_fork, s));
    HIP_TRY(c, hipStreamWaitEvent(s_sha, c->ev_fork, 0));
    // The three mask rows do not depend on the witness: their transforms run on the side stream under the
    // first chunk's encode (the hash of chunk 0 is queued behind them and has to wait for that encode anyway).
    TRY(lig_internal_encode_generic(c, mask, s_sha));
    TRY(lig_internal_encode_2k_rows(c, mlin, 2, s_sha));      // mlin and mquad are adjacent rows: one pass
    uint64_t absorbed = 0;
    size_t pr_i = 0;
    // what has to be on the encode stream in front of chunk ci's first kernel: its rows have arrived, are expanded, have their pads
    auto pre = [&](size_t ci, hipStream_t s_enc) -> int {
        const size_t b = T->sched1[ci].first, nb = T->sched1[ci].second - b;
        if (streamed) {
            if (T->up_by_thread) HIP_TRY(c, hipStreamWaitValue32(s_enc, T->flags.dev + ci, T->up.seq, hipStreamWaitValueGte, 0xffffffffu));
            else HIP_TRY(c, hipStreamWaitEvent(s_enc, T->ev_up[ci], 0));                   // this chunk's rows have arrived
            // (a derived row whose x / y rows belong to the previous chunk reads them from the staging area: that chunk's arrival was waited for earlier on this stream)
            if (T->narrow) lig::launch_expand_rows(s_enc, T->packed_dev, T->src_off_dev, T->widths_dev, b, nb, l, k, T->msgs, T->prod.first(b), T->prod.count(b, b + nb), T->wide.args(b, b + nb));
            for (; pr_i < T->pad_runs.size() && T->pad_runs[pr_i].first < b + nb; pr_i++) {      // runs never straddle chunks (split in begin)
                const PadRun& pr = T->pad_runs[pr_i];
                lig::launch_rng_fill_rows(s_enc, c->rk_dev, pr.pos, T->msgs + pr.first * (size_t)k, pr.count, pad, k, l, 1, pad);
            }
        }
        return LIG_OK;
    };
    const int enc_mode = T->zres ? lig::ENC_ZRES : lig::ENC_PLANAR;
    const int gate = lig::knobs().sha_gate;
    // Derived slots (lig_rows_set_derived): their waves read slots of ANY row, so every row of the trace has to be expanded first.  Rows that
    // arrive chunk by chunk: the arrival wait, expansion and pads of all chunks, then the waves, then the encodes -- such a trace gives up the
    // upload / encode overlap.  Device rows were expanded by rows_load on this stream.  Without a list nothing below differs.
    const bool derive = T->derive != nullptr;
    if (derive) {
        if (streamed) for (size_t ci = 0; ci < T->sched1.size(); ci++) TRY(pre(ci, s_enc));
        hipEvent_t e0 = nullptr, e1 = nullptr;                    // lig_profile_read_launches(rows_in_launch = 0): the waves of this commit
        TRY(lig_internal_profile_bracket(c, 0, &e0, &e1));
        if (e0) HIP_TRY(c, hipEventRecord(e0, s_enc));
        TRY(lig_internal_derive_run(c, T->derive, T->msgs, s_enc));
        if (e1) HIP_TRY(c, hipEventRecord(e1, s_enc));
    }
    // LIG_SHA_GATE=2 (round 6): K1 of chunk ci+1 is queued BEHIND the last kernel of chunk ci and runs alone -- the hash of chunk ci
    // waits for it (K1 is latency-bound: next to the hash waves it takes 2.2x as long, on the critical path of a lone proof) --
    // then the hash is placed, then the tile kernel of chunk ci+1 goes on.  (One Y scratch: K1 of ci+1 starts after chunk ci is done with it.)
    const bool k1_ahead = gate == 2 && c->fast && lig_tune::CHUNK <= lig::knobs().encode_chunk && !derive;
    if (k1_ahead && !T->sched1.empty()) {
        TRY(pre(0, s_enc));
        TRY(lig_internal_encode_rows(c, T->msgs, T->cw, T->sched1[0].second - T->sched1[0].first, enc_mode, s_enc, 1));
    }
    for (size_t ci = 0; ci < T->sched1.size(); ci++) {
        const size_t b = T->sched1[ci].first, nb = T->sched1[ci].second - b;
        if (!k1_ahead && !derive) TRY(pre(ci, s_enc));
        TRY(lig_internal_encode_rows(c, T->msgs + b * k, T->cw + b * k3, nb, enc_mode, s_enc, k1_ahead ? 14 : 15));
        HIP_TRY(c, hipEventRecord(c->ev_fork, s_enc));
        HIP_TRY(c, hipStreamWaitEvent(s_sha, c->ev_fork, 0));
        if (k1_ahead && ci + 1 < T->sched1.size()) {
            const size_t b1 = T->sched1[ci + 1].first, nb1 = T->sched1[ci + 1].second - b1;
            TRY(pre(ci + 1, s_enc));
            TRY(lig_internal_encode_rows(c, T->msgs + b1 * k, T->cw + b1 * k3, nb1, enc_mode, s_enc, 1));
            HIP_TRY(c, hipEventRecord(T->ev_k1, s_enc));
            HIP_TRY(c, hipStreamWaitEvent(s_sha, T->ev_k1, 0));
        }
        const size_t g = lig::knobs().sha_gate_rows;
        if (T->zres) {
            // (same placement rule as below; the gate is a whole batch of the in-hash butterflies: 8 rows)
            const size_t gz = g < 8 ? 8 : g;
            if (gate && nb > 2 * gz) {
                lig::launch_sha_update_rows_z(s_sha, T->sha_state, c->ep, T->cw + b * k3, gz, absorbed, T->msgs + b * k);
                HIP_TRY(c, hipEventRecord(T->ev_gate, s_sha));
                lig::launch_sha_update_rows_z(s_sha, T->sha_state, c->ep, T->cw + (b + gz) * k3, nb - gz, absorbed + gz, T->msgs + (b + gz) * k);
                HIP_TRY(c, hipStreamWaitEvent(s_enc, T->ev_gate, 0));
            } else {
                lig::launch_sha_update_rows_z(s_sha, T->sha_state, c->ep, T->cw + b * k3, nb, absorbed, T->msgs + b * k);
            }
        } else if (gate && nb > 2 * g) {
            // the hash waves must be placed while the chip is idle (one per SIMD, evenly): hash the first two rows, let the
            // encode stream wait for that, and queue the rest of the chunk right behind it on the hash stream
            lig::launch_sha_update_rows(s_sha, T->sha_state, n, T->cw + b * k3, 0, g, absorbed, k, T->msgs + b * k);
            HIP_TRY(c, hipEventRecord(T->ev_gate, s_sha));
            lig::launch_sha_update_rows(s_sha, T->sha_state, n, T->cw + (b + g) * k3, 0, nb - g, absorbed + g, k, T->msgs + (b + g) * k);
            HIP_TRY(c, hipStreamWaitEvent(s_enc, T->ev_gate, 0));
        } else {
            lig::launch_sha_update_rows(s_sha, T->sha_state, n, T->cw + b * k3, 0, nb, absorbed, k, T->msgs + b * k);
        }
        absorbed += nb;
    }
    mark("encode message rows");
    HIP_TRY(c, hipEventRecord(c->ev_fork, s));
    HIP_TRY(c, hipStreamWaitEvent(s_sha, c->ev_fork, 0));
    lig::launch_sha_update_rows(s_sha, T->sha_state, n, mask, n, 3, absorbed, k, nullptr);     // same plane-major instances, interleaved rows
    absorbed += 3;
    c->sha[T->sha_state].second = absorbed;
    HIP_TRY(c, hipEventRecord(c->ev_join, s_sha));
    HIP_TRY(c, hipStreamWaitEvent(s, c->ev_join, 0));
    mark("encode mask rows + column sha tail");
    uint32_t* leaf_level = T->nodes + 8 * ((size_t)n - 1);                    // n = 4k is a power of two: the leaves ARE the last level of the heap
    lig::launch_sha_final(s, T->sha_state, n, absorbed, leaf_level, k);      // plane-major instances -> leaves in column order, written in place
    TRY(lig_merkle_build(c, leaf_level, n, T->nodes));
    TRY(lig_internal_download(c, T->h_nodes, T->nodes, 32, s));              // the root now ...
    // (mixed DEVICE rows: the host has not seen their records -- rows_load expanded them on this stream -- so the flag word comes with the root)
    const bool wide_flag = !streamed && T->wide.any();
    if (wide_flag) HIP_TRY(c, hipMemcpyAsync(T->h_wide_flag, T->wide.flag_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, wait_stream(s));
    if (wide_flag && *T->h_wide_flag) FAIL(c, LIG_E_ARG, "lig_rows_commit: a wide slot of the device rows names a column >= l (lig_rows_job.wide_per_row); lig_rows_restart with good rows");
    if (streamed && T->up_by_thread) {
        // every chunk has been waited for by now; a copy the uploader thread could not make leaves garbage rows behind
        if (const int e = T->up.take_error()) {
            T->up_retry = e == (int)hipErrorLaunchTimeOut;
            FAIL(c, LIG_E_HIP, std::string("rows upload failed: ") + hipGetErrorString((hipError_t)e));
        }
    }
    std::memcpy(info->root, T->h_nodes, 32);
    TRY(lig_internal_download(c, T->h_nodes, T->nodes, lig_merkle_nodes(n) * 32, s));      // ... the tree for the decommitment (stage 3) under stage 2
    stage1_seed(info->root, T->hdr.ih, info->stage1_seed);
    mark("merkle + seed");
    return LIG_OK;
}

// where the stage-2 randomness rows come from: generated (dense rows of the synthetic stream, from the linear stream
// keyed by the stage-1 seed) or supplied by the caller (device pointer used in place / host rows uploaded chunk-wise)
struct RandSource { const fr* dev = nullptr; const uint8_t* host = nullptr; bool pushed = false;
                    lig_linear* linear = nullptr; };      // linear: `dev` (= T->rands_full) is formed from the sparse linear system on the side stream

// ================= stage 2 + 3
static int prove_stage23(lig_trace* T, const RandSource& rs, const uint8_t* const_sum_given, const uint8_t** proof, size_t* proof_len,
                         lig_proof_info* info, const std::function<void(const char*)>& mark) {
    lig_ctx* c = T->c;
    const uint32_t l = c->l, k = c->k, n = c->n, t = 192;
    const size_t R = T->R;
    hipStream_t s = c->stream, s2 = c->stream2;
    auto t0 = clk::now();
    uint32_t rk[60];
    // ================= stage 2: code / linear / quadratic accumulators over the resident codewords
    const size_t NT = T->triples.size() / 3;
    lig::aes256_expand_host(info->stage1_seed, rk);           // key of the code / linear / quadratic streams (three engines, same key)
    TRY(lig_internal_upload_small(c, c->rk_dev, rk, sizeof rk, s));
    // Accumulators.  All three tests are sums of low-degree polynomials, so they are accumulated where they are
    // cheapest and extended to the n evaluation points once per proof (exact field arithmetic => same values as the
    // reference's per-row n-point updates, nonbatch_context.hpp:756-780):
    //   code  = sum_r rc_r * U_r          degree < k : combine the MESSAGE rows (k values per row), encode once;
    //   lin   = sum_r U_r o R_r           degree < 2k: accumulate on the order-2k subgroup <w_n^2> (the even codeword
    //   quad  = sum_t rq_t (X o Y - Z)                 positions), then INTT_2k + NTT_n once.
    // Half of <w_n^2> is the message domain itself (w_n^4 = w_k^-1), where U_r and R_r are the message and randomness rows
    // as given; so a randomness row is only ever evaluated on ONE extra coset (w_n^2 <w_n^4>, k points): linH accumulates
    // msg_r o rand_r in message order (fused with the code test, same pass over the message rows), linC accumulates
    // codeword coset 2 against the coset-2 values of the randomness rows, and the two are interleaved once per proof.
    fr* code = T->acc; fr* lin = T->acc + n; fr* quad = T->acc + 2 * (size_t)n; fr* tmp = T->acc + 3 * (size_t)n;
    fr* linH = lin + 2 * (size_t)k; fr* linC = lin + 3 * (size_t)k;
    // group partials of the three k-column accumulators: group g of every chunk adds into slot g, combined once at the end
    const size_t groups = (lig_tune::CHUNK + lig_tune::GROUP - 1) / lig_tune::GROUP;
    fr* p_code = T->parts; fr* p_linH = T->parts + groups * (size_t)n; fr* p_linC = T->parts + 2 * groups * (size_t)n;
    const size_t dot_groups = (lig_tune::CHUNK + lig_tune::DOT_GROUP - 1) / lig_tune::DOT_GROUP;      // p_linC: dot_groups x k
    HIP_TRY(c, hipMemsetAsync(T->parts, 0, (2 * groups * (size_t)n + dot_groups * k) * 32, s));
    HIP_TRY(c, hipMemsetAsync(T->acc, 0, 4 * (size_t)n * 32, s));
    fr* rhalf = T->rcw;                                   // chunk x 2k
    // The randomness rows of chunk b+1 (AES sampling: LDS-bound; or the upload of the caller's rows) are formed on the side
    // stream, double-buffered, while the main stream encodes / accumulates chunk b (VALU-bound).
    // first chunk 192 rows (the encode stream waits for the first randomness rows); LIG_S2_HEAD overrides for experiments
    // (profiles/r02_stage1_schedule_ab.md: 192-256 rows +3 % proofs/s over 96 with two proofs in flight)
    const size_t s2_head = lig::knobs().s2_head;
    const std::vector<std::pair<size_t, size_t>> sched2 = chunk_schedule(R, lig_tune::CHUNK, s2_head, 0);
    const size_t n_chunks = sched2.size();
    std::vector<uint64_t> chunk_pos(n_chunks + 1, 0);
    for (size_t ci = 0; ci < n_chunks; ci++) {
        uint64_t cnt = 0;
        for (size_t r = sched2[ci].first; r < sched2[ci].second; r++) cnt += T->rows[r].data;
        chunk_pos[ci + 1] = chunk_pos[ci] + cnt;
    }
    auto rand_buf = [&](size_t ci) -> fr* { return rs.dev ? const_cast<fr*>(rs.dev) + sched2[ci].first * (size_t)k : T->randb + (ci & 1) * lig_tune::CHUNK * (size_t)k; };
    // Generated (dense) randomness rows: the sampler also accumulates the message-domain halves of the code and linear tests
    // while the elements are in registers (aes.hip: k_rand_rlc) -- all of it on the side stream; the main stream only encodes.
    const bool fused_rlc = !rs.dev && !rs.host && (k % 256 == 0) && lig::knobs().fused_rlc;
    const bool early_code = lig::knobs().early_code;      // (see below)
    const lig::f29s* rc_loop = early_code ? nullptr : T->coef_dev;      // code coefficients of the row loop (null: accumulated up front)
    // Caller rows in HOST memory (what a constraint generator delivers, nonbatch_context.hpp:654-780 / mpz_vector.hpp:108-127) take
    // the road of the witness rows (rows_load): the uploader thread copies chunk after chunk into the double buffer and
    // publishes each arrival in pinned host memory, the main stream waits for that word in its own queue and writes a second word
    // when it has consumed a chunk -- which is what the uploader waits for before it overwrites that half of the buffer.  No copy,
    // event or barrier packet of this transfer ever sits in a queue of the proof (the event-chained copy
    // on the side stream that this replaces is LIG_UPLOAD_MODE=1, profiles/r04_caller_rands_ab.md).
    const bool rands_by_thread = rs.host && lig::knobs().upload_mode == 2 && lig::knobs().rands_upload_mode == 2 && lig_internal_uploader_available(c) && n_chunks;
    uint32_t rseq = 0;
    const lig::FlagLayout fl = T->flag_layout(n_chunks);
    if (rands_by_thread) {
        TRY(T->flags.ensure(c, fl.words));
        if (fl.consumed + n_chunks > fl.words) FAIL(c, LIG_E_STATE, "rows job: flag page too small for the stage-2 schedule");
        rseq = ++T->rand.seq;
        T->up_abort.store(0, std::memory_order_release);
        std::vector<lig::UploadChunk> chunks;
        for (size_t ci = 0; ci < n_chunks; ci++) chunks.push_back({(uint8_t*)rand_buf(ci), rs.host + sched2[ci].first * (size_t)k * 32, (sched2[ci].second - sched2[ci].first) * (size_t)k * 32});
        lig_internal_uploader_submit(c->device, lig::chunk_jobs(chunks, T->flags.host + fl.rands, rseq, &T->rand.failed, T->flags.host + fl.consumed, &T->up_abort, 1), &T->rand.pending);
    }
    auto form_rand_chunk = [&](size_t ci) -> int {        // enqueued on the side stream
        const size_t b = sched2[ci].first, nb = sched2[ci].second - sched2[ci].first;
        fr* rb = rand_buf(ci);
        if (rs.pushed) return LIG_OK;                                                           // arriving in T->rands_full (lig_rows_push_rands)
        if (rs.dev) { HIP_TRY(c, hipEventRecord(T->ev_ready[ci & 1], s2)); return LIG_OK; }     // used in place
        if (rands_by_thread) return LIG_OK;                                                     // the uploader thread brings them
        if (ci >= 2) HIP_TRY(c, hipStreamWaitEvent(s2, T->ev_used[ci & 1], 0));      // buffer free again
        if (rs.host) {
            HIP_TRY(c, hipMemcpyAsync(rb, rs.host + b * (size_t)k * 32, nb * (size_t)k * 32, hipMemcpyHostToDevice, s2));
        } else {
            uint64_t lpos = chunk_pos[ci];
            for (size_t r = 0; r < nb;) {          // dense linear-test coefficients: one draw per witness slot, commit order; zeros after
                size_t run = 1;
                const uint32_t d = T->rows[b + r].data;
                while (r + run < nb && T->rows[b + r + run].data == d) run++;
                if (fused_rlc) lig::launch_rand_rlc(s2, c->rk_dev, lpos, rb + r * k, T->msgs + (b + r) * k, run, d, k, rc_loop ? rc_loop + b + r : nullptr, lig_tune::GROUP / 4, p_code, p_linH);
                else lig::launch_rng_fill_rows_dense(s2, c->rk_dev, lpos, rb + r * k, run, d, k);
                lpos += (uint64_t)run * d; r += run;
            }
        }
        HIP_TRY(c, hipEventRecord(T->ev_ready[ci & 1], s2));
        return LIG_OK;
    };
    {   // coefficients: one code-stream draw per row, one quadratic-stream draw per triple (the sampler's fused pass reads them)
        const std::vector<lig::f29s> coef = coef_table(draw_coefficients(info->stage1_seed, T->rows), nullptr, nullptr);
        TRY(lig_internal_upload_small(c, T->coef_dev, coef.data(), coef.size() * sizeof(lig::f29s), s));
    }
    HIP_TRY(c, hipEventRecord(c->ev_fork, s));            // the side stream starts after the key / coefficient uploads and the memsets above
    HIP_TRY(c, hipStreamWaitEvent(s2, c->ev_fork, 0));
    // sparse linear system: the whole randomness matrix is formed on the side stream (r_c from the linear stream, one pass in slot
    // order: linear.hip) while the main stream accumulates the code test below; stage 2 then finds it where an uploaded matrix would be
    if (rs.linear) TRY(lig_internal_linear_form(c, rs.linear, c->rk_dev, const_cast<fr*>(rs.dev), s2));
    if (n_chunks) TRY(form_rand_chunk(0));
    // (the side stream is already sampling the first randomness rows while the main stream does this)
    // The code-test accumulator does not depend on the randomness rows: it is formed FIRST (one pass over the message rows, one
    // encode, mask, download), so that the host can absorb it into the stage-2 seed hash -- 1 MiB of the 3 MiB sequential
    // SHA-256 that is the longest host step of a proof -- while the GPU is still busy with the row loop below.
    // LIG_EARLY_CODE=0: accumulate it inside the row loop as before (profiles/r03_early_code_ab.md).
    fr* mask = T->maskcw; fr* mlin = mask + n; fr* mquad = mask + 2 * (size_t)n;
    uint8_t* enc = T->h_enc;
    const size_t vec_bytes = (size_t)n * 32;
    if (early_code) {
        for (size_t b = 0; b < R; b += lig_tune::CHUNK) {
            const size_t nb = std::min<size_t>(lig_tune::CHUNK, R - b);
            lig::launch_rlc_accumulate29(s, T->msgs + b * k, k, 1, nullptr, 0, nb, k, T->coef_dev + b, p_code, nullptr, lig_tune::GROUP / 4);
        }
        lig::launch_rlc_combine(s, tmp, p_code, (uint32_t)((lig_tune::CHUNK + lig_tune::GROUP / 4 - 1) / (lig_tune::GROUP / 4)), k);
        TRY(lig_internal_encode_rows(c, tmp, code, 1, false));      // out of place: no device-to-device staging copy
        lig::launch_eltwise(s, LIG_OP_ADD_ASSIGN, mask, nullptr, code, n, fr{}, 0);
        TRY(lig_internal_download(c, enc, code, vec_bytes, s));
        HIP_TRY(c, hipEventRecord(T->ev_acc[0], s));
    }
    for (size_t ci = 0; ci < n_chunks; ci++) {
        const size_t b = sched2[ci].first, nb = sched2[ci].second - sched2[ci].first;
        fr* rb = rand_buf(ci);
        if (ci + 1 < n_chunks) TRY(form_rand_chunk(ci + 1));
        if (rs.pushed && !T->push_sync) HIP_TRY(c, hipStreamWaitValue32(s, T->flags.dev + fl.push, (uint32_t)sched2[ci].second, hipStreamWaitValueGte, 0xffffffffu));
        else if (rands_by_thread) HIP_TRY(c, hipStreamWaitValue32(s, T->flags.dev + fl.rands + ci, rseq, hipStreamWaitValueGte, 0xffffffffu));
        else HIP_TRY(c, hipStreamWaitEvent(s, T->ev_ready[ci & 1], 0));
        if (c->fast) {
            // coset-2 values of the randomness rows times the coset-2 plane of the codewords, summed per group of rows inside the
            // encoder's output kernel: the values themselves are never written
            TRY(lig_internal_encode_dot(c, rb, nb, T->cw + b * 3 * (size_t)k + k, 3 * (size_t)k, lig_tune::DOT_GROUP, p_linC, nullptr, T->zres));
        } else {
            TRY(lig_internal_encode_rows(c, rb, rhalf, nb, lig::ENC_HALF));
            lig::launch_rlc_accumulate29(s, T->cw + b * 3 * (size_t)k + k, 3 * (size_t)k, 1, rhalf, k, nb, k, nullptr, nullptr, p_linC, lig_tune::DOT_GROUP);
        }
        // k columns per pass: groups of 16 rows (4x more workgroups than the n-column grouping; same partial-sum space)
        if (!fused_rlc) lig::launch_rlc_accumulate29(s, T->msgs + b * k, k, 1, rb, k, nb, k, rc_loop ? rc_loop + b : nullptr, p_code, p_linH, lig_tune::GROUP / 4);
        if (rands_by_thread) HIP_TRY(c, hipStreamWriteValue32(s, T->flags.dev + fl.consumed + ci, rseq, 0));      // chunk consumed: its half of the buffer is free
        else HIP_TRY(c, hipEventRecord(T->ev_used[ci & 1], s));
    }
    {   // one combine per accumulator and proof
        const uint32_t pg = (uint32_t)((lig_tune::CHUNK + lig_tune::GROUP / 4 - 1) / (lig_tune::GROUP / 4));
        if (!early_code) lig::launch_rlc_combine(s, tmp, p_code, pg, k);         // the code test's k message values (tmp was zeroed with acc)
        lig::launch_rlc_combine(s, linH, p_linH, pg, k);
        lig::launch_rlc_combine(s, linC, p_linC, (uint32_t)dot_groups, k);
    }
    mark("stage2 rows (rng+dot+encode+rlc)");
    lig::launch_sum_elems(s, linH, k, 1, T->dots, nullptr);       // sum of all <witness row, randomness row> (prover_kernels.hip)
    lig::launch_lin_interleave(s, lin, linH, linC, k);
    HIP_TRY(c, hipMemsetAsync(lin + 2 * (size_t)k, 0, (size_t)(n - 2 * k) * 32, s));
    const lig::CwView view{T->msgs, T->cw, k};
    // (the group partials of the row loop have been combined above: their space holds the quadratic test's group sums now)
    lig::launch_quad_rows29_view(s, view, 2 * k, T->tri_dev, T->coef_dev + R, T->coef_dev + R + NT, NT, quad, T->parts, 2 * groups * (size_t)n);
    // Each accumulator is extended to the n evaluation points, masked (nonbatch_context.hpp:739-753) and sent to the host
    // as soon as it is final; the host absorbs it into the stage-2 seed hash (a sequential SHA-256 over 3 MiB, the longest
    // host step of the proof) while the GPU extends the next one.
    const H::Fr* dots = reinterpret_cast<const H::Fr*>(T->h_small);
    TRY(lig_internal_download(c, T->h_small, T->dots, 32, s));
    if (!early_code) {
        TRY(lig_internal_encode_rows(c, tmp, code, 1, false));      // out of place: no device-to-device staging copy
        lig::launch_eltwise(s, LIG_OP_ADD_ASSIGN, mask, nullptr, code, n, fr{}, 0);
        TRY(lig_internal_download(c, enc, code, vec_bytes, s));
        HIP_TRY(c, hipEventRecord(T->ev_acc[0], s));
    }
    TRY(lig_internal_extend_2k(c, lin));
    lig::launch_eltwise(s, LIG_OP_ADD_ASSIGN, mlin, nullptr, lin, n, fr{}, 0);
    TRY(lig_internal_download(c, enc + vec_bytes, lin, vec_bytes, s));
    HIP_TRY(c, hipEventRecord(T->ev_acc[1], s));
    TRY(lig_internal_extend_2k(c, quad));
    lig::launch_eltwise(s, LIG_OP_ADD_ASSIGN, mquad, nullptr, quad, n, fr{}, 0);
    TRY(lig_internal_download(c, enc + 2 * vec_bytes, quad, vec_bytes, s));
    HIP_TRY(c, hipEventRecord(T->ev_acc[2], s));
    // prover self-check (src/webgpu_prover.cpp:355-386,465-469): the three decodes run on the GPU while the host hashes
    H::Fr* dec = reinterpret_cast<H::Fr*>(T->h_small + 32);    // 3 x n
    const fr* accs[3] = {code, lin, quad};
    for (int a3 = 0; a3 < 3; a3++) {
        TRY(lig_internal_decode_to(c, accs[a3], tmp));
        TRY(lig_internal_download(c, dec + (size_t)a3 * n, tmp, vec_bytes, s));
    }
    HIP_TRY(c, hipEventRecord(c->ev_join, s));
    {
        Sha256 h2;
        h2.add("LigetronStage2", 15).add(info->root, 32);
        for (int a3 = 0; a3 < 3; a3++) {
            HIP_TRY(c, wait_event(T->ev_acc[a3]));
            h2.add(enc + (size_t)a3 * vec_bytes, vec_bytes);
        }
        h2.finish(info->stage2_seed);
    }
    if (const_sum_given) std::memcpy(info->const_sum, const_sum_given, 32);     // the caller's public constant (linear_sums)
    else if (rs.linear) {
        // the statement's own constant -sum_c b_c r_c, formed on the side stream (in host memory since the first chunk's event)
        if (n_chunks) HIP_TRY(c, wait_event(T->ev_ready[0])); else HIP_TRY(c, wait_stream(s2));      // (every record of that event follows the form on the side stream)
        std::memcpy(info->const_sum, lig_internal_linear_const(rs.linear), 32);
    } else {
        // synthetic stream: every witness slot carries the constraint w_i = b_i with b public (derived from witness_key), so
        // the constant is minus the sum of all inner products <witness row, randomness row> = minus the sum of linH
        const H::Fr sum = H::neg(dots[0]);
        std::memcpy(info->const_sum, sum.v, 32);
    }
    const std::vector<uint32_t> idx = sample_columns(info->stage2_seed, n, t);
    mark("accumulators to host, seed hash, sampling, decodes");
    info->ms_stage2 = ms_since(t0);
    t0 = clk::now();

    // ================= stage 3: open the sampled columns of every committed row, assemble the envelope.  The gather
    // runs while the host derives the decommitment (the Merkle nodes were downloaded in stage 1) and lays out the envelope;
    // the opened columns then land in place while the host evaluates the self-check predicates.
    TRY(lig_sample_init(c, idx.data(), idx.size()));
    if (T->zres) lig::launch_gather_rows_z(s, c->ep, view, R, c->sample_idx, t, T->samples);
    else lig::launch_gather_rows_planar(s, view, R, c->sample_idx, t, T->samples);
    lig::launch_gather_rows(s, T->maskcw, n, 3, c->sample_idx, t, T->samples + R * (size_t)t);
    const size_t n_nodes = lig_merkle_nodes(n);
    const std::vector<uint8_t> sib = decommit(T->h_nodes, (n_nodes + 1) / 2, idx);
    const size_t smp_bytes = (R + 3) * (size_t)t * 32;
    const EnvelopeLayout lay = write_envelope(T->h_proof, T->h_proof_cap, T->hdr.version, T->hdr.program_hash, T->hdr.generated_at, k, n, t,
                                              info->root, sib, idx, nullptr, smp_bytes);       // framing only: the layout is known now
    if (lay.total > T->h_proof_cap) FAIL(c, LIG_E_NOMEM, "proof buffer too small");
    TRY(lig_internal_download(c, T->h_proof + lay.samples_off, T->samples, smp_bytes, s));   // opened columns land in place (any byte offset)
    for (int a3 = 0; a3 < 3; a3++) std::memcpy(T->h_proof + lay.vec_off[a3], enc + (size_t)a3 * vec_bytes, vec_bytes);     // 3 MiB, under the 13 MB download
    HIP_TRY(c, wait_event(c->ev_join));          // decoded accumulators are on the host
    const SelfCheck ok = self_check(dec, info->const_sum, l, k, n);
    info->valid_code = ok.valid_code; info->valid_linear = ok.valid_linear; info->valid_quad = ok.valid_quad;
    HIP_TRY(c, wait_stream(s));
    *proof = T->h_proof;
    *proof_len = lay.total;
    mark("serialize");
    info->ms_stage3 = ms_since(t0);
    HIP_TRY(c, hipGetLastError());
    return LIG_OK;
}

// LIG_TRACE=1: print a synchronised timeline of the prove call to stderr (debug aid, off by default)
static std::function<void(const char*)> make_mark(lig_ctx* c) {
    const bool trace_on = lig::knobs().trace;
    auto t_mark = std::make_shared<clk::time_point>(clk::now());
    return [c, trace_on, t_mark](const char* what) {
        if (!trace_on) return;
        (void)hipStreamSynchronize(c->stream);
        std::fprintf(stderr, "[lig_trace] %-28s %8.3f ms\n", what, ms_since(*t_mark));
        *t_mark = clk::now();
    };
}

extern "C" {

// plan_rows: commit order of witness_manager (witness_manager.hpp:497-503): full linear rows, full quadratic
// triples, partial linear row, partial quadratic triple
static int synth_prepare_impl(lig_ctx* c, const lig_synth_job* job, lig_trace* T);
int lig_synth_prepare(lig_ctx* c, const lig_synth_job* job, lig_trace** out) {
    CHECK_CTX(c);
    if (!job || !out) return LIG_E_ARG;
    *out = nullptr;
    lig_trace* T = new lig_trace();
    T->c = c; T->job = *job;
    T->job.batch_ops = nullptr; T->job.batch_data = nullptr;       // the program is consumed here; the caller's memory is not kept
    T->job.public_args = nullptr; T->job.public_arg_lens = nullptr;
    const int rc = synth_prepare_impl(c, job, T);
    if (rc != LIG_OK) { lig_trace_destroy(T); return rc; }         // nothing is handed out on failure
    *out = T;
    return LIG_OK;
}
static int synth_prepare_impl(lig_ctx* c, const lig_synth_job* job, lig_trace* T) {
    const uint32_t l = c->l, k = c->k, n = c->n, t = 192;
    // k - l = sample_size upstream (include/params.hpp:24-32); with fewer random pads than opened columns the proof
    // would silently stop being zero-knowledge
    if (l >= k || l < 2 || t > n || k - l < t) FAIL(c, LIG_E_ARG, "synthetic trace: need 2 <= l <= k - 192 (k - l random pads cover the 192 opened columns)");
    if (!plan_rows(*job, l, T->rows, T->n_init)) FAIL(c, LIG_E_ARG, "malformed batch program");
    if (T->n_init && k - l != 192) FAIL(c, LIG_E_ARG, "batch program: on_batch_init draws params::sample_size = 192 pads, k - l must be 192");
    if (!fill_job_header(*job, T->hdr)) FAIL(c, LIG_E_ARG, "public arguments: null pointer");
    const size_t R = T->rows.size();
    for (T->RB = 0; T->RB < R && T->rows[T->RB].kind >= RK_INIT; T->RB++) {}
    TRY(trace_alloc(c, T));
    // pads: init rows of the batch program drew theirs while the program ran (prepare); every stream row draws at commit time
    if (R > T->RB) T->pad_runs.push_back({T->RB, R - T->RB, (uint64_t)T->n_init * (k - l)});
    T->mask_pos = (uint64_t)(T->n_init + (R - T->RB)) * (k - l);
    // witness values: one draw per data slot of every linear / x / y row, in commit order; z = x*y
    if (T->RB) TRY(lig_run_batch_program(c, *job, T->msgs));
    TRY(lig_internal_synth_witness(c, job->witness_key, T->rows, T->RB, T->msgs));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    return LIG_OK;
}

void lig_trace_destroy(lig_trace* T) {
    if (!T) return;
    (void)hipSetDevice(T->c->device);
    sync_all_streams(T->c);
    T->up_abort.store(1, std::memory_order_release);      // (copies that wait for a buffer of a proof that never ran)
    T->up.drain();                                        // an upload still in flight
    T->rand.drain();
    lig_internal_linear_destroy(T->linear);
    lig_internal_derive_destroy(T->derive);
    T->c->sha.erase(T->sha_state);
    if (T->leak) {      // destinations of a transfer that was given up on and has never completed (upload_settled): they outlive the trace
        T->rands_full = nullptr; T->msgs_alt = nullptr; T->msgs = nullptr; T->randb = nullptr; T->packed_dev = nullptr;
    }
    for (void* p : {(void*)T->rands_full, (void*)T->msgs_alt, (void*)T->msgs, (void*)T->cw, (void*)T->maskcw, (void*)T->randb, (void*)T->rcw, (void*)T->acc, (void*)T->parts, (void*)T->dots,
                    (void*)T->samples, (void*)T->sha_state, (void*)T->leaves, (void*)T->nodes, (void*)T->tri_dev,
                    (void*)T->coef_dev})
        (void)hipFree(p);
    for (int i = 0; i < 2; i++) { if (T->ev_ready[i]) (void)hipEventDestroy(T->ev_ready[i]); if (T->ev_used[i]) (void)hipEventDestroy(T->ev_used[i]); }
    if (T->ev_gate) (void)hipEventDestroy(T->ev_gate);
    if (T->ev_k1) (void)hipEventDestroy(T->ev_k1);
    for (int a3 = 0; a3 < 3; a3++) if (T->ev_acc[a3]) (void)hipEventDestroy(T->ev_acc[a3]);
    for (hipEvent_t e : T->ev_up) (void)hipEventDestroy(e);
    T->flags.release();
    (void)hipFree(T->src_off_dev); (void)hipFree(T->widths_dev); (void)hipFree(T->packed_dev); (void)hipFree(T->prod.dev);
    T->wide.release(); (void)hipHostFree(T->h_wide_flag);
    (void)hipHostFree(T->h_proof); (void)hipHostFree(T->h_enc); (void)hipHostFree(T->h_nodes); (void)hipHostFree(T->h_small);
    delete T;
}
uint64_t lig_trace_rows(const lig_trace* T) { return T ? T->R + 3 : 0; }

int lig_synth_prove(lig_trace* T, const uint8_t** proof, size_t* proof_len, lig_proof_info* info) {
    if (!T || !proof || !proof_len || !info) return LIG_E_ARG;
    lig_ctx* c = T->c;
    CHECK_CTX(c);
    if (T->from_rows) FAIL(c, LIG_E_STATE, "lig_synth_prove on a trace made by lig_rows_begin (use lig_rows_commit / lig_rows_prove)");
    std::memset(info, 0, sizeof *info);
    info->rows = T->R + 3;
    const auto t_begin = clk::now();
    const auto mark = make_mark(c);
    TRY(prove_stage1(T, info, mark));
    info->ms_stage1 = ms_since(t_begin);
    TRY(prove_stage23(T, RandSource{}, nullptr, proof, proof_len, info, mark));
    info->ms_total = ms_since(t_begin);
    return LIG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Host rows -> device: through the uploader thread (upload.hip: why, and what it guarantees) or by stream-ordered copies.
// the byte range of every stage-1 chunk in the caller's matrix (T->host_msgs) and the destination of its copy
static std::vector<lig::UploadChunk> stage1_chunks(const lig_trace* T, uint8_t* up_dst) {
    auto chunk_src = [&](size_t b) -> size_t { return T->narrow ? (size_t)T->src_off[b] : b * (size_t)T->c->k * 32; };
    std::vector<lig::UploadChunk> chunks;
    for (const auto& ch : T->sched1) chunks.push_back({up_dst + chunk_src(ch.first), T->host_msgs + chunk_src(ch.first), chunk_src(ch.second) - chunk_src(ch.first)});
    return chunks;
}
// witness rows by stream-ordered copies on the context's copy stream, one event per stage-1 chunk (LIG_UPLOAD_MODE=1, devices without
// stream memory operations, and the second attempt after a transfer of the uploader thread has timed out)
static int rows_copy_by_stream(lig_ctx* c, lig_trace* T, uint8_t* up_dst) {
    const std::vector<lig::UploadChunk> chunks = stage1_chunks(T, up_dst);
    T->up_by_thread = false;
    if (T->ev_up.empty()) {
        T->ev_up.resize(T->sched1.size(), nullptr);
        for (auto& e : T->ev_up) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    for (size_t ci = 0; ci < chunks.size(); ci++) {
        if (chunks[ci].bytes) HIP_TRY(c, hipMemcpyAsync(chunks[ci].dst, chunks[ci].src, chunks[ci].bytes, hipMemcpyHostToDevice, lig_internal_copy_stream(c)));
        HIP_TRY(c, hipEventRecord(T->ev_up[ci], lig_internal_copy_stream(c)));
    }
    HIP_TRY(c, hipGetLastError());
    return LIG_OK;
}
// A transfer of the uploader thread timed out (Uploader::run): the waiting streams were released and drain here.  The copy itself is
// still queued on the uploader's stream and cannot be cancelled.  Bounded wait for it to leave the bus: true = it has (its bytes are where
// they belong or will be overwritten by the second attempt, which is counted); false = it is still pending -- what it reads (the caller's rows)
// and writes (this trace's buffers) must stay alive: the trace is marked, its buffers are never freed or reused, lig_upload_health() reports it.
static bool upload_settled(lig_ctx* c, lig_trace* T) {
    sync_all_streams(c);
    if (lig_internal_upload_settle(c->device, (double)lig::knobs().upload_timeout_s)) { lig_internal_upload_count_retry(c->device); return true; }
    T->leak = true;
    return false;
}
static const char* const UPLOAD_PENDING_MSG = "; the transfer is still pending and cannot be cancelled: keep the rows alive until lig_upload_health reports no unsettled "
                                              "transfer (the trace's device buffers are kept for the life of the process)";
// message rows of a rows job -> T->msgs.  Device rows: one copy on the main stream.  Host rows: the upload starts now, on
// the copy stream, one event per stage-1 chunk: lig_rows_commit encodes chunk b while chunk b+1 is still on the bus.
static int rows_load(lig_ctx* c, lig_trace* T, const void* msgs, bool on_device) {
    const uint32_t k = c->k;
    const size_t R = T->R;
    T->host_msgs = nullptr;
    T->loaded = true;
    T->alt_pending = false;
    if (!R) return LIG_OK;
    fr* dst = T->msgs;
    // narrow host rows land in the packed staging area and are expanded into `msgs` by lig_rows_commit (after the previous
    // proof has finished with it): no second matrix needed
    if (T->committed && !(T->narrow && !on_device)) {
        // the committed trace still needs its rows for stage 2: the next trace goes to the second matrix and is swapped in
        // by lig_rows_commit -- its upload runs under lig_rows_prove of the current one
        if (!T->msgs_alt) HIP_TRY(c, hipMalloc((void**)&T->msgs_alt, R * (size_t)k * 32));
        dst = T->msgs_alt;
        T->alt_pending = true;
    }
    if (on_device) {
        if (T->wide.any()) HIP_TRY(c, hipMemsetAsync(T->wide.flag_dev, 0, sizeof(uint32_t), c->stream));      // raised by a record with a column >= l: lig_rows_commit
        if (T->narrow) lig::launch_expand_rows(c->stream, (const uint8_t*)msgs, T->src_off_dev, T->widths_dev, 0, R, c->l, k, dst, T->prod.dev, T->prod.rows.size(), T->wide.args(0, R));
        else HIP_TRY(c, hipMemcpyAsync(dst, msgs, R * (size_t)k * 32, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipGetLastError());
        return LIG_OK;
    }
    T->host_msgs = (const uint8_t*)msgs;
    if (T->narrow && !T->packed_dev) HIP_TRY(c, hipMalloc((void**)&T->packed_dev, T->src_off[R] ? T->src_off[R] : 16));   // (the job began with device rows)
    uint8_t* up_dst = T->narrow ? T->packed_dev : (uint8_t*)dst;
    // (every earlier reader of `dst` has finished: lig_rows_prove returns only after its stream work is done)
    // (A copy kernel reading the pinned rows over PCIe instead of the DMA engine was measured: 37 GB/s against 56 GB/s, and
    // the long-running kernel serialises with the proof's kernels whenever both streams share a hardware queue:
    // stage 2 5.6 -> 13.8 ms.  The DMA engine it is.)
    if (lig::knobs().upload_mode == 2 && lig_internal_uploader_available(c)) {      // 2: uploader thread (default), 1: per-context copy stream + events
        TRY(T->flags.ensure(c, T->flag_layout().words));
        T->up.seq++;
        lig_internal_uploader_submit(c->device, lig::chunk_jobs(stage1_chunks(T, up_dst), T->flags.host, T->up.seq, &T->up.failed), &T->up.pending);
        T->up_by_thread = true;
        return LIG_OK;
    }
    return rows_copy_by_stream(c, T, up_dst);
}

// ---------------------------------------------------------------------------------------------------------------------
// rows supplied by the caller (include/lig_hip.h, lig_rows_*)
static int rows_begin_impl(lig_ctx* c, const lig_rows_job* job, lig_trace* T) {
    const uint32_t l = c->l, k = c->k, n = c->n, t = 192, pad = k - l;
    if (l >= k || l < 2 || t > n || k - l < t) FAIL(c, LIG_E_ARG, "rows job: need 2 <= l <= k - 192");
    if (job->rows && (!job->kinds || !job->msgs)) FAIL(c, LIG_E_ARG, "rows job: null kinds / msgs");
    if (!fill_job_header(*job, T->hdr)) FAIL(c, LIG_E_ARG, "public arguments: null pointer");
    T->from_rows = true;
    const size_t R = job->rows;
    std::vector<uint8_t> draw;
    std::vector<uint64_t> pos;
    if (const char* why = lig::parse_row_kinds(*job, l, k, true, T->rows, draw, pos)) FAIL(c, LIG_E_ARG, std::string("rows job: ") + why);
    T->dense_rands = job->dense_rands_per_row != nullptr;
    T->mask_pos = pos[R];
    lig::NarrowPlan np;
    if (job->elem_bytes || lig::job_wide_per_row(*job)) {            // the narrow row format; every row is local
        std::vector<size_t> all(R);
        for (size_t r = 0; r < R; r++) all[r] = r;
        if (const char* why = lig::plan_narrow_rows(job->elem_bytes, T->rows, draw, l, k, all, np, lig::job_wide_per_row(*job))) FAIL(c, LIG_E_ARG, std::string("rows job: ") + why);
        // mixed host rows: their records are read here, before anything is allocated, copied or launched
        if (!job->msgs_on_device && !np.mixed_rows.empty())
            if (const char* why = lig::wide_records_refusal((const uint8_t*)job->msgs, np.src_off, np.mixed_rows, np.wide, l)) FAIL(c, LIG_E_ARG, std::string("rows job: ") + why);
    }
    T->narrow = np.packed;
    TRY(trace_alloc(c, T));
    if (T->narrow) {
        TRY(lig_internal_upload_narrow_plan(c, np, &T->src_off_dev, &T->widths_dev, &T->prod, &T->wide));
        T->src_off = std::move(np.src_off);
        T->widths = np.widths;
        if (T->wide.any()) HIP_TRY(c, hipHostMalloc((void**)&T->h_wide_flag, sizeof(uint32_t)));
        if (!job->msgs_on_device) HIP_TRY(c, hipMalloc((void**)&T->packed_dev, T->src_off[R] ? T->src_off[R] : 16));
    }
    // pad runs: consecutive flagged rows whose stream positions are consecutive, never straddling a stage-1 chunk
    for (const auto& ch : T->sched1)
        for (size_t r = ch.first; r < ch.second;) {
            if (!draw[r]) { r++; continue; }
            size_t e = r + 1;
            while (e < ch.second && draw[e] && pos[e] == pos[e - 1] + pad) e++;
            T->pad_runs.push_back({r, e - r, pos[r]});
            r = e;
        }
    return rows_load(c, T, job->msgs, job->msgs_on_device != 0);
}
int lig_rows_begin(lig_ctx* c, const lig_rows_job* job, lig_trace** out) {
    CHECK_CTX(c);
    if (!job || !out) return LIG_E_ARG;
    *out = nullptr;
    lig_trace* T = new lig_trace();
    T->c = c;
    std::memset(&T->job, 0, sizeof T->job);
    const int rc = rows_begin_impl(c, job, T);
    if (rc != LIG_OK) { lig_trace_destroy(T); return rc; }
    *out = T;
    return LIG_OK;
}
int lig_rows_restart(lig_trace* T, const void* msgs, int msgs_on_device) {
    if (!T) return LIG_E_ARG;
    lig_ctx* c = T->c;
    CHECK_CTX(c);
    if (!T->from_rows) FAIL(c, LIG_E_STATE, "lig_rows_restart: not a rows trace");
    if (T->R && !msgs) FAIL(c, LIG_E_ARG, "lig_rows_restart: null rows");
    if (T->leak) FAIL(c, LIG_E_STATE, "lig_rows_restart: a transfer into this trace's buffers never completed (lig_upload_health): destroy the trace");
    if (T->loaded && T->host_msgs) { T->up.drain(); if (c->stream3) HIP_TRY(c, hipStreamSynchronize(c->stream3)); }      // an upload nobody committed: let it finish first
    if (!msgs_on_device && T->wide.any())                 // mixed host rows: the records are read before any copy starts
        if (const char* why = lig::wide_records_refusal((const uint8_t*)msgs, T->src_off, T->wide.mixed.rows, T->wide.wide, c->l)) FAIL(c, LIG_E_ARG, std::string("lig_rows_restart: ") + why);
    if (!T->committed) T->diag_ok = false;                // the rows go straight into the matrix: the window of lig_rows_diagnose ends
    return rows_load(c, T, msgs, msgs_on_device != 0);
}
int lig_rows_commit(lig_trace* T, uint8_t root[32], uint8_t stage1_seed[32]) {
    if (!T) return LIG_E_ARG;
    lig_ctx* c = T->c;
    CHECK_CTX(c);
    if (!T->from_rows || !T->loaded) FAIL(c, LIG_E_STATE, "lig_rows_commit: no rows loaded (lig_rows_begin / lig_rows_restart)");
    if (T->committed) FAIL(c, LIG_E_STATE, "lig_rows_commit: the committed trace has not been proved yet");
    T->diag_ok = false;
    if (T->alt_pending) { std::swap(T->msgs, T->msgs_alt); T->alt_pending = false; }
    std::memset(&T->info1, 0, sizeof T->info1);
    T->info1.rows = T->R + 3;
    const auto t_begin = clk::now();
    {
        if (T->leak) FAIL(c, LIG_E_STATE, "lig_rows_commit: a transfer into this trace's buffers never completed (lig_upload_health): destroy the trace");
        T->up_retry = false;
        int rc = prove_stage1(T, &T->info1, make_mark(c));
        if (rc != LIG_OK && T->up_retry) {
            // a chunk of the rows did not arrive within LIG_UPLOAD_TIMEOUT_S (the uploader thread has released the streams, stage 1 ran over
            // garbage and is discarded): once the abandoned copy has left the bus the same rows are brought by stream-ordered copies and
            // stage 1 runs again -- the caller sees a slow commit, not an error
            T->up_retry = false;
            const std::string why = c->err;
            T->up.drain();
            if (upload_settled(c, T)) {
                rc = rows_copy_by_stream(c, T, T->narrow ? T->packed_dev : (uint8_t*)T->msgs);
                if (rc == LIG_OK) rc = prove_stage1(T, &T->info1, make_mark(c));
            } else c->err = why + UPLOAD_PENDING_MSG;
        }
        if (rc != LIG_OK) {           // the caller is told it may free its rows: nothing of ours may still read them (but see T->leak)
            T->up.drain();
            sync_all_streams(c);
            T->loaded = false; T->host_msgs = nullptr;
            return rc;
        }
    }
    T->info1.ms_stage1 = ms_since(t_begin);
    T->committed = true;
    T->diag_ok = true;
    T->loaded = false;
    T->host_msgs = nullptr;                               // the caller's memory is no longer referenced
    if (root) std::memcpy(root, T->info1.root, 32);
    if (stage1_seed) std::memcpy(stage1_seed, T->info1.stage1_seed, 32);
    return LIG_OK;
}
int lig_rows_prove(lig_trace* T, const void* rands, int rands_on_device, const uint8_t const_sum[32], const uint8_t** proof,
                   size_t* proof_len, lig_proof_info* info) {
    if (!T || !proof || !proof_len || !info) return LIG_E_ARG;
    lig_ctx* c = T->c;
    CHECK_CTX(c);
    if (!T->from_rows || !T->committed) FAIL(c, LIG_E_STATE, "lig_rows_prove: lig_rows_commit has not run on this trace");
    if (T->linear && rands) FAIL(c, LIG_E_ARG, "lig_rows_prove: randomness rows given while a linear system is set (lig_rows_set_linear)");
    if (T->R && !rands && !T->dense_rands && !T->rands_pushed && !T->linear) FAIL(c, LIG_E_ARG, "lig_rows_prove: null randomness rows");
    if (const_sum) {
        H::Fr v;
        std::memcpy(v.v, const_sum, 32);
        if (H::geq(v, H::P)) FAIL(c, LIG_E_ARG, "lig_rows_prove: constant not reduced mod p");
    }
    *info = T->info1;
    const auto t_begin = clk::now();
    RandSource rs;                                        // default: generated from the dense counts of the job
    if (rands && T->rands_pushed) {                       // explicit rows win over rows pushed earlier: drop what the uploader still holds of those
        T->up_abort.store(1, std::memory_order_release);
        T->rand.drain();
        T->up_abort.store(0, std::memory_order_release);
        (void)T->rand.take_error();
        T->rands_pushed = 0;
    }
    if (rands && rands_on_device) rs.dev = (const fr*)rands; else if (rands) rs.host = (const uint8_t*)rands;
    else if (T->linear) { rs.dev = T->rands_full; rs.linear = T->linear; }
    else if (T->rands_pushed) {
        if (T->rands_pushed != T->R) FAIL(c, LIG_E_STATE, "lig_rows_prove: lig_rows_push_rands has not delivered every row");
        rs.dev = T->rands_full; rs.pushed = true;
    }
    for (int attempt = 0;; attempt++) {
        int rc = prove_stage23(T, rs, const_sum, proof, proof_len, info, make_mark(c));
        if (rc != LIG_OK) {           // randomness-row copies the uploader thread still holds read the caller's memory: drop them, wait
            T->rands_pushed = 0; T->push_log.clear();
            T->up_abort.store(1, std::memory_order_release);
            T->rand.drain();
            sync_all_streams(c);
            return rc;
        }
        if (!(rs.host || rs.pushed)) break;
        T->rand.drain();
        const int e = T->rand.take_error();
        if (!e) break;
        // a randomness-row transfer timed out: stages 2 / 3 ran over garbage and are discarded.  Same second attempt as in
        // lig_rows_commit: host rows come by stream-ordered copies now (the uploader is out of service), pushed rows are copied again
        // from the pushes' host memory (valid until this call returns)
        const bool again = e == (int)hipErrorLaunchTimeOut && attempt == 0;
        if (again && upload_settled(c, T)) {
            if (rs.pushed) {
                for (const UploadJob& j : T->push_log) HIP_TRY(c, lig_internal_copy_job(j, lig_internal_copy_stream(c)));
                if (c->stream3) HIP_TRY(c, hipStreamSynchronize(c->stream3));
                T->push_sync = true;          // every row is there: stage 2 has no arrival word to wait for
            }
            *info = T->info1;
            continue;
        }
        T->rands_pushed = 0; T->push_log.clear();
        FAIL(c, LIG_E_HIP, std::string("randomness rows upload failed: ") + hipGetErrorString((hipError_t)e) + (again ? UPLOAD_PENDING_MSG : ""));
    }
    T->rands_pushed = 0; T->push_log.clear();
    info->ms_total = info->ms_stage1 + ms_since(t_begin);
    T->committed = false;
    return LIG_OK;
}

// the shared end of lig_rows_set_linear / lig_rows_attach_linear (fn, for the error text): the randomness matrix the forms write, then L
// takes the place of the trace's system
static int trace_take_linear(lig_trace* T, lig_linear* L, const char* fn) {
    lig_ctx* c = T->c;
    if (!T->rands_full) {
        const hipError_t e = hipMalloc((void**)&T->rands_full, (T->R ? T->R : 1) * (size_t)c->k * 32);
        if (e != hipSuccess) { lig_internal_linear_destroy(L); FAIL(c, LIG_E_NOMEM, std::string(fn) + ": randomness matrix: " + hipGetErrorString(e)); }
    }
    lig_internal_linear_destroy(T->linear);
    T->linear = L;
    return LIG_OK;
}
int lig_rows_set_linear(lig_trace* T, const lig_linear_system* sys) {
    if (!T) return LIG_E_ARG;
    lig_ctx* c = T->c;
    CHECK_CTX(c);
    if (!T->from_rows || !(T->loaded || T->committed)) FAIL(c, LIG_E_STATE, "lig_rows_set_linear: between lig_rows_begin and lig_rows_prove");
    if (T->rands_pushed) FAIL(c, LIG_E_STATE, "lig_rows_set_linear: randomness rows have already been pushed");
    if (!sys) {
        lig_internal_linear_destroy(T->linear);
        T->linear = nullptr;
        return LIG_OK;
    }
    if (T->dense_rands) FAIL(c, LIG_E_ARG, "lig_rows_set_linear: the job has dense_rands_per_row");
    lig_linear* L = nullptr;
    TRY(lig_internal_linear_create(c, sys, kinds_of(T->rows).data(), T->R, &L));       // lig_linear_check first: nothing is launched for a system it rejects
    return trace_take_linear(T, L, "lig_rows_set_linear");
}

// derived slots (derive.hip): checked against the trace's kinds and widths, copied, in force from the next lig_rows_commit on.  A refused
// list changes nothing.  (No derive kernel is in flight here: lig_rows_commit returns only after stage 1 has drained.)
int lig_rows_set_derived(lig_trace* T, const lig_linear_system* sys, const lig_derived_slot* d, uint64_t n, lig_derived_info* info) {
    if (!T) return LIG_E_ARG;
    lig_ctx* c = T->c;
    CHECK_CTX(c);
    if (!T->from_rows) FAIL(c, LIG_E_STATE, "lig_rows_set_derived: not a rows trace");
    if (!d || !n) {
        if (info && info->struct_bytes < sizeof(lig_derived_info)) FAIL(c, LIG_E_ARG, "lig_rows_set_derived: lig_derived_info.struct_bytes too small");
        lig_internal_derive_destroy(T->derive);
        T->derive = nullptr;
        if (info) { const uint32_t sb = info->struct_bytes; std::memset(info, 0, sizeof *info); info->struct_bytes = sb; }
        return LIG_OK;
    }
    lig_derive* D = nullptr;
    TRY(lig_internal_derive_create(c, sys, kinds_of(T->rows).data(), T->R, T->narrow ? T->widths.data() : nullptr, d, n, &D, info));
    lig_internal_derive_destroy(T->derive);
    T->derive = D;
    return LIG_OK;
}

int lig_rows_attach_linear(lig_trace* T, const lig_linear_program* p) {
    if (!T) return LIG_E_ARG;
    lig_ctx* c = T->c;
    CHECK_CTX(c);
    if (!T->from_rows || !(T->loaded || T->committed)) FAIL(c, LIG_E_STATE, "lig_rows_attach_linear: between lig_rows_begin and lig_rows_prove");
    if (T->rands_pushed) FAIL(c, LIG_E_STATE, "lig_rows_attach_linear: randomness rows have already been pushed");
    if (!p) {
        lig_internal_linear_destroy(T->linear);
        T->linear = nullptr;
        return LIG_OK;
    }
    if (T->dense_rands) FAIL(c, LIG_E_ARG, "lig_rows_attach_linear: the job has dense_rands_per_row");
    if (!lig_internal_linear_fits(c, p, kinds_of(T->rows).data(), T->R)) FAIL(c, LIG_E_ARG, "lig_rows_attach_linear: the program was prepared for another device, (l, k), row count or row kinds");
    lig_linear* L = nullptr;
    TRY(lig_internal_linear_attach(c, p, &L));
    return trace_take_linear(T, L, "lig_rows_attach_linear");
}
int lig_rows_set_linear_values(lig_trace* T, const uint8_t* coefs, uint64_t n_coefs) {
    if (!T) return LIG_E_ARG;
    lig_ctx* c = T->c;
    CHECK_CTX(c);
    if (!T->from_rows || !T->linear) FAIL(c, LIG_E_STATE, "lig_rows_set_linear_values: no linear program is attached (lig_rows_attach_linear)");
    return lig_internal_linear_set_values(c, T->linear, coefs, n_coefs, c->stream2);      // the stream lig_rows_prove forms on
}

// which constraints does the committed witness violate (diagnose.hip); blocking, reads T->msgs only, main stream only
int lig_rows_diagnose(lig_trace* T, const lig_linear_system* sys, lig_diag_linear* lin_out, uint64_t lin_cap, lig_diag_quad* quad_out, uint64_t quad_cap,
                      lig_diag_info* info) {
    if (!T || !info || info->struct_bytes < sizeof(lig_diag_info)) return LIG_E_ARG;
    if ((lin_cap && !lin_out) || (quad_cap && !quad_out)) return LIG_E_ARG;
    const auto t_begin = clk::now();                      // ms_total is the whole call: the host check of the system included
    lig_ctx* c = T->c;
    CHECK_CTX(c);
    if (!T->from_rows) FAIL(c, LIG_E_STATE, "lig_rows_diagnose: not a rows trace");
    if (!T->diag_ok) FAIL(c, LIG_E_STATE, "lig_rows_diagnose: no committed matrix (between lig_rows_commit and the next commit, or a lig_rows_restart after lig_rows_prove)");
    if (sys && lig_linear_check(sys, kinds_of(T->rows).data(), T->R, c->l) != LIG_OK) FAIL(c, LIG_E_ARG, "lig_rows_diagnose: linear system rejected by lig_linear_check");
    const uint32_t struct_bytes = info->struct_bytes;
    std::memset(info, 0, sizeof *info);
    info->struct_bytes = struct_bytes;
    TRY(lig_internal_rows_diagnose(c, T->msgs, T->R, T->tri_dev, T->triples.size() / 3, sys, lin_out, lin_cap, quad_out, quad_cap, info));
    info->ms_total = ms_since(t_begin);
    return LIG_OK;
}

// the same passes over the statement attached to the trace (lig_rows_set_linear / lig_rows_attach_linear, the values in force): nothing of
// the program or the attachment is written
int lig_rows_diagnose_attached(lig_trace* T, lig_diag_linear* lin_out, uint64_t lin_cap, lig_diag_quad* quad_out, uint64_t quad_cap, lig_diag_info* info) {
    if (!T || !info || info->struct_bytes < sizeof(lig_diag_info)) return LIG_E_ARG;
    if ((lin_cap && !lin_out) || (quad_cap && !quad_out)) return LIG_E_ARG;
    const auto t_begin = clk::now();
    lig_ctx* c = T->c;
    CHECK_CTX(c);
    if (!T->from_rows) FAIL(c, LIG_E_STATE, "lig_rows_diagnose_attached: not a rows trace");
    if (!T->diag_ok) FAIL(c, LIG_E_STATE, "lig_rows_diagnose_attached: no committed matrix (between lig_rows_commit and the next commit, or a lig_rows_restart after lig_rows_prove)");
    if (!T->linear) FAIL(c, LIG_E_STATE, "lig_rows_diagnose_attached: nothing is attached (lig_rows_set_linear, lig_rows_attach_linear)");
    const uint32_t struct_bytes = info->struct_bytes;
    std::memset(info, 0, sizeof *info);
    info->struct_bytes = struct_bytes;
    TRY(lig_internal_rows_diagnose_attached(c, T->msgs, T->R, T->tri_dev, T->triples.size() / 3, T->linear, lin_out, lin_cap, quad_out, quad_cap, info));
    info->ms_total = ms_since(t_begin);
    return LIG_OK;
}

// the asked constraints as the library holds them: terms, coefficient values, committed witness values, b_c, residual (diagnose.hip); the
// window, blocking and streams of lig_rows_diagnose.  which: the C name, for the messages; att: the attached statement instead of sys
static int rows_explain(const char* which, bool att, lig_trace* T, const lig_linear_system* sys, const uint32_t* asked, uint64_t n_asked,
                        lig_explain_constraint* con_out, lig_explain_term* terms_out, uint64_t term_cap, lig_explain_info* info) {
    if (!T || !info || info->struct_bytes < sizeof(lig_explain_info)) return LIG_E_ARG;
    if ((n_asked && (!con_out || !asked)) || (term_cap && !terms_out)) return LIG_E_ARG;
    const auto t_begin = clk::now();
    lig_ctx* c = T->c;
    CHECK_CTX(c);
    const std::string w(which);
    if (!T->from_rows) FAIL(c, LIG_E_STATE, w + ": not a rows trace");
    if (!T->diag_ok) FAIL(c, LIG_E_STATE, w + ": no committed matrix (between lig_rows_commit and the next commit, or a lig_rows_restart after lig_rows_prove)");
    if (att && !T->linear) FAIL(c, LIG_E_STATE, w + ": nothing is attached (lig_rows_set_linear, lig_rows_attach_linear)");
    if (!att && !sys) FAIL(c, LIG_E_ARG, w + ": null linear system");
    if (!att && lig_linear_check(sys, kinds_of(T->rows).data(), T->R, c->l) != LIG_OK) FAIL(c, LIG_E_ARG, w + ": linear system rejected by lig_linear_check");
    const uint32_t struct_bytes = info->struct_bytes;
    std::memset(info, 0, sizeof *info);
    info->struct_bytes = struct_bytes;
    if (att) TRY(lig_internal_rows_explain_attached(c, T->msgs, T->linear, asked, n_asked, con_out, terms_out, term_cap, info));
    else TRY(lig_internal_rows_explain(c, T->msgs, sys, asked, n_asked, con_out, terms_out, term_cap, info));
    info->ms_total = ms_since(t_begin);
    return LIG_OK;
}
int lig_rows_explain(lig_trace* T, const lig_linear_system* sys, const uint32_t* constraints, uint64_t n_asked, lig_explain_constraint* con_out,
                     lig_explain_term* terms_out, uint64_t term_cap, lig_explain_info* info) {
    return rows_explain("lig_rows_explain", false, T, sys, constraints, n_asked, con_out, terms_out, term_cap, info);
}
int lig_rows_explain_attached(lig_trace* T, const uint32_t* constraints, uint64_t n_asked, lig_explain_constraint* con_out, lig_explain_term* terms_out,
                              uint64_t term_cap, lig_explain_info* info) {
    return rows_explain("lig_rows_explain_attached", true, T, nullptr, constraints, n_asked, con_out, terms_out, term_cap, info);
}
// the committed w[slot] of any row kind, canonical (diagnose.hip); the window, blocking and streams of lig_rows_diagnose
int lig_rows_read_slots(lig_trace* T, const uint32_t* slots, uint64_t n_slots, uint8_t* values) {
    if (!T || (n_slots && (!slots || !values))) return LIG_E_ARG;
    lig_ctx* c = T->c;
    CHECK_CTX(c);
    if (!T->from_rows) FAIL(c, LIG_E_STATE, "lig_rows_read_slots: not a rows trace");
    if (!T->diag_ok) FAIL(c, LIG_E_STATE, "lig_rows_read_slots: no committed matrix (between lig_rows_commit and the next commit, or a lig_rows_restart after lig_rows_prove)");
    return lig_internal_rows_read_slots(c, T->msgs, T->R, slots, n_slots, values);
}

// the constraints through the asked slots, and the witness slots no term touches (diagnose.hip); the window, blocking and streams of
// lig_rows_diagnose.  Both read the slot-major index of a program: the one attached to the trace (att), or a temporary one prepared from
// sys -- lig_linear_check first, nothing is launched for a system it rejects -- and released before the call returns.
struct TempProgram {
    lig_linear_program* P = nullptr;
    ~TempProgram() { lig_linear_program_release(P); }
};
using SlotsRun = std::function<int(lig_ctx*, const uint8_t*, const lig_linear_view&)>;
// the checks the four entries share (args_ok: the entry's own host check of its arguments), then `run` on the view of the statement
static int rows_slots_call(const char* which, bool att, lig_trace* T, const lig_linear_system* sys, const std::function<bool()>& args_ok, bool nothing_to_do,
                           const SlotsRun& run) {
    lig_ctx* c = T->c;
    CHECK_CTX(c);
    const std::string w(which);
    if (!T->from_rows) FAIL(c, LIG_E_STATE, w + ": not a rows trace");
    if (!T->diag_ok) FAIL(c, LIG_E_STATE, w + ": no committed matrix (between lig_rows_commit and the next commit, or a lig_rows_restart after lig_rows_prove)");
    if (att && !T->linear) FAIL(c, LIG_E_STATE, w + ": nothing is attached (lig_rows_set_linear, lig_rows_attach_linear)");
    if (!att && !sys) FAIL(c, LIG_E_ARG, w + ": null linear system");
    const std::vector<uint8_t> kinds = kinds_of(T->rows);
    // (the prepare below runs lig_linear_check itself)
    if (!att && nothing_to_do && lig_linear_check(sys, kinds.data(), T->R, c->l) != LIG_OK) FAIL(c, LIG_E_ARG, w + ": linear system rejected by lig_linear_check");
    if (!args_ok()) FAIL(c, LIG_E_ARG, w + ": the asked slots must be strictly ascending and below rows * l");
    if (nothing_to_do) return LIG_OK;      // (an empty request launches nothing: no prepare either)
    if (att) return run(c, kinds.data(), lig_internal_linear_view(T->linear));
    TempProgram tmp;
    TRY(lig_internal_linear_prepare(c, sys, kinds.data(), T->R, &tmp.P));
    return run(c, kinds.data(), lig_internal_linear_program_view(tmp.P));
}
static int rows_explain_slots(const char* which, bool att, lig_trace* T, const lig_linear_system* sys, const uint32_t* slots, uint64_t n_asked, lig_slot_record* slot_out,
                              lig_slot_term* terms_out, uint64_t term_cap, lig_slot_info* info) {
    if (!T || !info || info->struct_bytes < sizeof(lig_slot_info)) return LIG_E_ARG;
    if ((n_asked && (!slot_out || !slots)) || (term_cap && !terms_out)) return LIG_E_ARG;
    const auto t_begin = clk::now();
    const uint32_t struct_bytes = info->struct_bytes;
    // (the asked list before the prepare of the term-list entry: a refused list launches nothing)
    const auto args_ok = [&]() -> bool {
        for (uint64_t i = 0; i < n_asked; i++) if (slots[i] >= T->R * (uint64_t)T->c->l || (i && slots[i] <= slots[i - 1])) return false;
        return true;
    };
    TRY(rows_slots_call(which, att, T, sys, args_ok, !n_asked, [&](lig_ctx* c, const uint8_t* kinds, const lig_linear_view& v) -> int {
        std::memset(info, 0, sizeof *info);
        info->struct_bytes = struct_bytes;
        return lig_internal_rows_explain_slots(c, T->msgs, kinds, T->R, v, slots, n_asked, slot_out, terms_out, term_cap, info);
    }));
    if (!n_asked) { std::memset(info, 0, sizeof *info); info->struct_bytes = struct_bytes; }
    info->ms_total = ms_since(t_begin);
    return LIG_OK;
}
static int rows_untouched_slots(const char* which, bool att, lig_trace* T, const lig_linear_system* sys, int nonzero_only, lig_slot_value* out, uint64_t cap,
                                lig_untouched_info* info) {
    if (!T || !info || info->struct_bytes < sizeof(lig_untouched_info)) return LIG_E_ARG;
    if (cap && !out) return LIG_E_ARG;
    const auto t_begin = clk::now();
    const uint32_t struct_bytes = info->struct_bytes;
    TRY(rows_slots_call(which, att, T, sys, []() -> bool { return true; }, false, [&](lig_ctx* c, const uint8_t* kinds, const lig_linear_view& v) -> int {
        std::memset(info, 0, sizeof *info);
        info->struct_bytes = struct_bytes;
        return lig_internal_rows_untouched_slots(c, T->msgs, kinds, T->R, v, nonzero_only, out, cap, info);
    }));
    info->ms_total = ms_since(t_begin);
    return LIG_OK;
}
int lig_rows_explain_slots_attached(lig_trace* T, const uint32_t* slots, uint64_t n_asked, lig_slot_record* slot_out, lig_slot_term* terms_out, uint64_t term_cap,
                                    lig_slot_info* info) {
    return rows_explain_slots("lig_rows_explain_slots_attached", true, T, nullptr, slots, n_asked, slot_out, terms_out, term_cap, info);
}
int lig_rows_explain_slots(lig_trace* T, const lig_linear_system* sys, const uint32_t* slots, uint64_t n_asked, lig_slot_record* slot_out, lig_slot_term* terms_out,
                           uint64_t term_cap, lig_slot_info* info) {
    return rows_explain_slots("lig_rows_explain_slots", false, T, sys, slots, n_asked, slot_out, terms_out, term_cap, info);
}
int lig_rows_untouched_slots_attached(lig_trace* T, int nonzero_only, lig_slot_value* out, uint64_t cap, lig_untouched_info* info) {
    return rows_untouched_slots("lig_rows_untouched_slots_attached", true, T, nullptr, nonzero_only, out, cap, info);
}
int lig_rows_untouched_slots(lig_trace* T, const lig_linear_system* sys, int nonzero_only, lig_slot_value* out, uint64_t cap, lig_untouched_info* info) {
    return rows_untouched_slots("lig_rows_untouched_slots", false, T, sys, nonzero_only, out, cap, info);
}

int lig_rows_push_rands(lig_trace* T, uint64_t first_row, uint64_t n_rows, const void* host_rows) {
    return lig_rows_push_rands_sparse(T, first_row, n_rows, nullptr, host_rows);
}
int lig_rows_push_rands_sparse(lig_trace* T, uint64_t first_row, uint64_t n_rows, const uint8_t* present, const void* host_rows) {
    if (!T) return LIG_E_ARG;
    lig_ctx* c = T->c;
    CHECK_CTX(c);
    if (!T->from_rows || !T->committed) FAIL(c, LIG_E_STATE, "lig_rows_push_rands: lig_rows_commit has not run on this trace");
    if (T->linear) FAIL(c, LIG_E_STATE, "lig_rows_push_rands: a linear system is set (lig_rows_set_linear): the library forms the randomness rows");
    if (first_row != T->rands_pushed || first_row + n_rows > T->R) FAIL(c, LIG_E_ARG, "lig_rows_push_rands: rows must arrive in order, without gaps, inside the trace");
    if (!n_rows) return LIG_OK;
    size_t n_present = n_rows;
    if (present) { n_present = 0; for (uint64_t i = 0; i < n_rows; i++) n_present += present[i] != 0; }
    if (n_present && !host_rows) FAIL(c, LIG_E_ARG, "lig_rows_push_rands: null rows");
    const size_t row_bytes = (size_t)c->k * 32;
    if (!T->rands_full) HIP_TRY(c, hipMalloc((void**)&T->rands_full, T->R * row_bytes));
    // one job per push: the uploader publishes the number of rows that have arrived in the page's push word (jobs of a trace are taken in order)
    UploadJob j{(uint8_t*)T->rands_full + first_row * row_bytes, (const uint8_t*)host_rows, n_rows * row_bytes, nullptr, (uint32_t)(first_row + n_rows), &T->rand.failed};
    // runs of present rows are copied from where they follow each other in host_rows, the others zero-filled on the device
    if (present && n_present != n_rows) j.segs = std::make_shared<std::vector<UploadSeg>>(lig::presence_runs(present, n_rows, row_bytes, j.dst, j.src));
    j.abort = &T->up_abort; j.prio = 1;
    if (lig::knobs().upload_mode != 2 || !lig_internal_uploader_available(c)) {
        // no uploader thread (LIG_UPLOAD_MODE=1, or a device without stream memory operations): the same rows by plain copies on the
        // copy stream, waited for here -- slower (the transfer sits in a HIP queue of the context) but every caller of the push
        // interface (include/lig_hip_row_batcher.hpp) keeps working.  ADVICE r4.
        if (first_row == 0) T->push_sync = true;
        if (!T->push_sync) FAIL(c, LIG_E_STATE, "lig_rows_push_rands: the uploader became unavailable in the middle of a trace");
        HIP_TRY(c, lig_internal_copy_job(j, lig_internal_copy_stream(c)));
        if (c->stream3) HIP_TRY(c, hipStreamSynchronize(c->stream3));
        T->rands_pushed = first_row + n_rows;
        return LIG_OK;
    }
    TRY(T->flags.ensure(c, T->flag_layout().words));
    j.flag = T->flags.host + T->flag_layout().push;
    if (first_row == 0) { T->push_sync = false; __atomic_store_n(j.flag, 0u, __ATOMIC_RELEASE); T->up_abort.store(0, std::memory_order_release); T->push_log.clear(); }
    T->push_log.push_back(j);
    lig_internal_uploader_submit(c->device, {j}, &T->rand.pending);
    T->rands_pushed = first_row + n_rows;
    return LIG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// host-only transcript helpers
int lig_public_arg_bytes(int kind, const char* text, uint8_t* out, size_t cap, size_t* len) {
    if (!text || !len) return LIG_E_ARG;
    std::vector<uint8_t> b;
    if (kind == LIG_ARG_I64) {
        char* end = nullptr;
        errno = 0;
        const long long v = std::strtoll(text, &end, 10);
        if (errno || end == text || *end) return LIG_E_ARG;
        const int64_t i = (int64_t)v;
        b.resize(8);
        std::memcpy(b.data(), &i, 8);                      // (u8*)&i .. + sizeof(int64_t), little-endian host as upstream
    } else if (kind == LIG_ARG_STR) {
        b.assign(text, text + std::strlen(text) + 1);      // c_str() .. + size() + 1: the NUL is part of the argument
    } else if (kind == LIG_ARG_HEX) {
        std::string h(text);
        if (h.rfind("0x", 0) == 0) h = h.substr(2);
        if (h.size() % 2) h.insert(h.begin(), '0');
        auto nib = [](char ch) -> int { return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1; };
        for (size_t i = 0; i < h.size(); i += 2) {
            const int hi = nib(h[i]), lo = nib(h[i + 1]);
            if (hi < 0 || lo < 0) return LIG_E_ARG;        // boost::algorithm::unhex throws on a non-hex character
            b.push_back((uint8_t)(hi * 16 + lo));
        }
    } else return LIG_E_ARG;
    *len = b.size();
    if (!out || cap < b.size()) return LIG_E_ARG;
    if (!b.empty()) std::memcpy(out, b.data(), b.size());
    return LIG_OK;
}
int lig_instance_hash(const uint8_t* args, const uint64_t* lens, size_t n_args, uint8_t out[32]) {
    if (!out || !instance_hash(args, lens, n_args, out)) return LIG_E_ARG;
    return LIG_OK;
}
int lig_sample_columns(const uint8_t seed[32], uint32_t n, uint32_t t, uint32_t* out_sorted) {
    if (!seed || !out_sorted || !n) return LIG_E_ARG;
    const std::vector<uint32_t> idx = sample_columns(seed, n, t);
    std::memcpy(out_sorted, idx.data(), idx.size() * sizeof(uint32_t));
    return LIG_OK;
}

}  // extern "C"
