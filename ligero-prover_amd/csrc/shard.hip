// shard.hip -- one trace sharded over the GPUs of a node (lig_shard_*).
#include "explain_plan.hpp"
#include "prover_common.hpp"
#include "upload.hpp"
#include <unistd.h>
#include <functional>

// =====================================================================================================================
// One trace sharded over the GPUs of a node (BASELINE.json configs[3]).
//
// The committed rows are cut into G = W * rounds global chunks (<= 512 rows, equal sizes, never splitting an x,y,z
// triple or an equality pair) and dealt block-cyclically: chunk g belongs to rank g mod W, so the local rows of a rank are
// its chunks r, r+W, r+2W, ...; every rank forms, encodes and keeps only those (codewords as three coset planes + the message
// rows, like the single-GPU prover: lig::CwView).  leaf_j hashes ALL rows in commit order, so
// the hash is column-partitioned (rank h owns columns [h*n/W, (h+1)*n/W), i.e. positions q in [h*k/W, (h+1)*k/W) of all four
// cosets): in round c every rank sends the column slices
// of its c-th chunk to their owners -- ONE all-to-all per round -- and receives the W consecutive global chunks
// cW .. cW+W-1 restricted to its columns, in rank order = commit order.  The column hash therefore runs in commit order
// from the first round on, on the side stream, while the main stream encodes round c+1 and the copy stream exchanges it:
//     main:  encode(c)   pack(c)   encode(c+1)  pack(c+1)  ...
//     comm:                        exchange(c)             exchange(c+1)
//     hash:                                     hash(c)                 hash(c+1)
// n/W leaves per rank are all-gathered, the Merkle tree is built redundantly.  The stage-2 tests are sums over rows: every
// rank accumulates its rows on the low-degree domains (k + 2k + 2k values), the partial sums are all-gathered and added
// mod p locally (RCCL has no modular reduction).  Opened columns are all-gathered and laid out in commit order.
// Collectives: lig_comm (include/lig_hip.h) -- RCCL over xGMI from comm_rccl.hip (stream-ordered), or host-synchronous
// callbacks (tests over gloo).  Every rank ends with the same envelope, byte-identical to lig_synth_prove.
struct lig_shard {
    lig_ctx* c = nullptr;
    lig_synth_job job;
    lig_comm comm;
    uint32_t rank = 0, world = 1;
    std::atomic<const char*> dbg_wait{nullptr}; std::atomic<uint64_t> dbg_wait_since_ms{0};     // what shard_bounded_wait is polling for, since when (shard_debug)
    bool poisoned = false;                     // work queued behind a failed collective never drained (shard_quiesce): no further calls, buffers outlive the shard
    std::vector<RowDesc> rows;                 // global plan
    std::vector<size_t> gb;                    // G + 1 global chunk boundaries
    std::vector<size_t> lrow0;                 // local row offset of my c-th chunk (rounds + 1 entries)
    std::vector<size_t> grow;                  // global row of every local row
    std::vector<uint64_t> wit_pos, lin_pos;    // stream position of every global row (+1 entry)
    std::vector<uint8_t> draw;                 // per global row: its k-l pads are drawn here at commit time (pad_encoding_random)
    std::vector<uint64_t> enc_pos;             // encoding-stream position of every global row's pads (+1 entry = the masks' position)
    bool from_rows = false;                    // lig_shard_rows_*: the local rows and their randomness rows come from the caller
    bool dense_rands = false, committed = false;
    bool diag_ok = false;                      // `msgs` holds a committed trace (lig_shard_rows_diagnose): from lig_shard_rows_commit until the next load
    lig_proof_info info1;                      // stage-1 results kept between lig_shard_rows_commit and lig_shard_rows_prove
    JobHeader hdr;
    size_t RB = 0, n_init = 0;                 // leading rows committed by the batch program, of those: init rows
    size_t R = 0, Rl = 0, rows_max = 0, ncol = 0, rounds = 0, G = 0, ch_cap = 0;
    fr *msgs = nullptr, *cw = nullptr, *maskcw = nullptr, *send = nullptr, *recv = nullptr, *randb = nullptr, *rhalf = nullptr, *acc = nullptr,
       *parts = nullptr, *accp = nullptr, *accg = nullptr, *dots = nullptr, *smp = nullptr, *smpg = nullptr;
    uint32_t *sha_state = nullptr, *leaves_slice = nullptr, *leaves = nullptr, *nodes = nullptr, *tri_dev = nullptr;
    lig::f29s* coef_dev = nullptr;
    std::vector<uint32_t> triples;             // local row indices
    std::vector<size_t> triple_ord;            // global ordinal of each local triple
    uint8_t *h_proof = nullptr, *h_enc = nullptr, *h_nodes = nullptr, *h_small = nullptr;
    size_t h_proof_cap = 0;
    hipEvent_t ev_enc[2] = {nullptr, nullptr}, ev_comm[2] = {nullptr, nullptr}, ev_hash[2] = {nullptr, nullptr};
    // caller rows in host memory (lig_shard_rows_*): uploaded by the library's uploader thread, as in lig_rows_* (prover.hip).  Flag words
    // in pinned host memory (lig::shard_flags): [round c: local rows of my c-th chunk arrived | round c: randomness rows arrived | ... consumed]
    FlagPage flags;
    UploadLane up;                             // one lane for the local rows and their randomness rows; the latter count in rand_seq
    uint32_t rand_seq = 0;
    bool rows_by_thread = false;               // the local rows of the trace being committed are arriving through the uploader
    std::atomic<int> up_abort{0};
    // narrow row format (lig_rows_job.elem_bytes): packed byte offset of every LOCAL row (+1 entry) and its width, on the device; the
    // staging buffer host rows are copied to (device rows are expanded from where they are)
    bool narrow = false;
    std::vector<uint64_t> src_off;
    uint64_t* src_off_dev = nullptr; uint8_t* widths_dev = nullptr; uint8_t* packed_dev = nullptr;
    ProductRows prod;                          // derived LOCAL rows (LIG_ELEM_PRODUCT)
    WideRows wide;                             // mixed LOCAL rows (lig_rows_job.wide_per_row)
    // sparse linear system (lig_shard_rows_set_linear): this rank's share of it, regrouped by local slot (linear.hip), and the local rows x k
    // randomness matrix it is formed into per proof; both survive lig_shard_rows_restart
    lig_linear* linear = nullptr;
    fr* rands_lin = nullptr;
    // derived slots (lig_shard_rows_set_derived): this rank's program (derive.hip), the send block of a wave's all-gather and the import
    // buffer of a commit; survive lig_shard_rows_restart.  The buffers only grow: one a peer may still have mapped is never freed before
    // lig_shard_destroy has told the communicator (derive_retired).
    lig_derive_shard* derive = nullptr;
    fr *derive_send = nullptr, *derive_import = nullptr;
    uint64_t derive_send_cap = 0, derive_import_cap = 0;
    std::vector<void*> derive_retired;
    std::vector<uint8_t> elem_bytes_all;       // lig_rows_job.elem_bytes of ALL rows (empty: none given): what a list of derived slots is checked against
    bool used_comm = false;                    // a collective has been issued with buffers of this shard as send buffers
    bool exchange_even_alone = false;          // LIG_SHARD_FORCE_EXCHANGE: run pack + all-to-all with world == 1 too (tests)
    size_t chunk_rows(size_t g) const { return g < G ? gb[g + 1] - gb[g] : 0; }
};

namespace lig {
// The column slices of `rows` codewords, one block of cap_rows x ncol per destination rank h.  Inside a row of a block the
// ncol = 4*kq columns of rank h are PLANE-MAJOR: element c*kq + ql = codeword column 4*(h*kq + ql) + c, so that both sides
// move contiguous runs (reads: runs of kq elements of one plane / of the message row; the receiver's column hash then reads
// 32-byte neighbours) and instance j of the receiver's hash state is simply element j of every received row.
__global__ void __launch_bounds__(256) k_pack_slices(CwView cw, fr* __restrict__ out, size_t rows, size_t kq, size_t cap_rows) {
    const size_t n = 4 * (size_t)cw.k, ncol = 4 * kq, total = rows * n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / n, j = i - r * n;                  // j: position in the row of blocks = h*ncol + c*kq + ql
        const size_t h = j / ncol, e = j - h * ncol, c = e / kq, ql = e - c * kq;
        fr_store(out + (h * cap_rows + r) * ncol + e, fr_load(cw.at(r, (uint32_t)(4 * (h * kq + ql) + c))));
    }
}
}  // namespace lig

// The block-cyclic deal: rounds = ceil(R / (W * CHUNK)), G = W * rounds global chunks of (nearly) equal size whose boundaries
// never fall inside an x,y,z triple or an equality pair; chunk g belongs to rank g mod W.  gb: G + 1 boundaries.
static void shard_chunks(const std::vector<RowDesc>& rows, uint32_t W, size_t& rounds, std::vector<size_t>& gb) {
    const size_t R = rows.size();
    rounds = std::max<size_t>(1, (R + W * lig_tune::CHUNK - 1) / (W * lig_tune::CHUNK));
    const size_t G = rounds * W;
    const size_t target = std::max<size_t>(1, (R + G - 1) / G);
    gb.assign(G + 1, R);
    gb[0] = 0;
    auto inside_group = [&](uint8_t kd) { return kd == 2 || kd == 3 || kd == RK_EQY || kd == RK_BQY || kd == RK_BQZ; };
    for (size_t g = 1; g < G; g++) {
        size_t b = std::min(R, gb[g - 1] + target);
        while (b < R && inside_group(rows[b].kind)) b++;                       // never split a triple / an equality pair
        gb[g] = b;
    }
}

extern "C" {

// host only (no GPU work): the deal of a job's committed rows over `world` ranks, for drivers and tests
int lig_shard_plan(const lig_synth_job* job, uint32_t l, uint32_t world, uint64_t* rounds_out, uint64_t* boundaries, size_t cap) {
    if (!job || !world || !rounds_out) return LIG_E_ARG;
    std::vector<RowDesc> rows;
    size_t n_init = 0;
    if (!plan_rows(*job, l, rows, n_init)) return LIG_E_ARG;
    size_t rounds = 0;
    std::vector<size_t> gb;
    shard_chunks(rows, world, rounds, gb);
    *rounds_out = rounds;
    if (gb.size() > cap || !boundaries) return gb.size() > cap ? LIG_E_NOMEM : LIG_E_ARG;
    for (size_t i = 0; i < gb.size(); i++) boundaries[i] = gb[i];
    return LIG_OK;
}

static int shard_prepare_impl(lig_ctx* c, const lig_synth_job* job, uint32_t rank, uint32_t world, lig_shard* S);
int lig_shard_prepare(lig_ctx* c, const lig_synth_job* job, uint32_t rank, uint32_t world, const lig_comm* comm, lig_shard** out) {
    CHECK_CTX(c);
    if (!job || !out || !comm || world == 0 || rank >= world) return LIG_E_ARG;
    if (!comm->all_to_all || !comm->all_gather) return LIG_E_ARG;
    *out = nullptr;
    lig_shard* S = new lig_shard();
    S->c = c; S->job = *job; S->comm = *comm; S->rank = rank; S->world = world;
    S->job.batch_ops = nullptr; S->job.batch_data = nullptr;
    S->job.public_args = nullptr; S->job.public_arg_lens = nullptr;
    if (!fill_job_header(*job, S->hdr)) { delete S; return LIG_E_ARG; }
    const int rc = shard_prepare_impl(c, job, rank, world, S);
    if (rc != LIG_OK) { lig_shard_destroy(S); return rc; }
    *out = S;
    return LIG_OK;
}
// the deal + every buffer of a shard whose global row plan (S->rows) is known
static int shard_alloc(lig_ctx* c, uint32_t rank, uint32_t world, lig_shard* S);
static int shard_prepare_impl(lig_ctx* c, const lig_synth_job* job, uint32_t rank, uint32_t world, lig_shard* S) {
    const uint32_t l = c->l, k = c->k, n = c->n, t = 192;
    if (l >= k || l < 2 || t > n || k - l < t || k % world) FAIL(c, LIG_E_ARG, "sharded trace: need 2 <= l <= k - 192 and world | k");
    if (!plan_rows(*job, l, S->rows, S->n_init)) FAIL(c, LIG_E_ARG, "malformed batch program");
    if (S->n_init && k - l != 192) FAIL(c, LIG_E_ARG, "batch program: on_batch_init draws params::sample_size = 192 pads, k - l must be 192");
    const size_t R = S->R = S->rows.size();
    for (S->RB = 0; S->RB < R && S->rows[S->RB].kind >= RK_INIT; S->RB++) {}
    S->wit_pos.assign(R + 1, 0); S->lin_pos.assign(R + 1, 0);
    S->draw.assign(R, 0); S->enc_pos.assign(R + 1, 0);
    for (size_t r = 0; r < R; r++) {
        const uint8_t kd = S->rows[r].kind;
        S->wit_pos[r + 1] = S->wit_pos[r] + ((kd == 3 || kd >= RK_INIT) ? 0 : S->rows[r].data);   // z rows and batch rows draw nothing
        S->lin_pos[r + 1] = S->lin_pos[r] + S->rows[r].data;
        S->draw[r] = kd <= 3;                                                                        // stream rows draw at commit time; init rows drew theirs in the program
        S->enc_pos[r + 1] = S->enc_pos[r] + ((kd <= 3 || kd == RK_INIT) ? (k - l) : 0);             // rows that draw k-l pads upstream
    }
    TRY(shard_alloc(c, rank, world, S));
    const size_t Rl = S->Rl;
    // local witness rows: same stream positions as in the single-GPU trace
    uint32_t rk[60];
    if (S->RB) {          // the batch program is small: every rank runs it and keeps the rows it owns
        fr* all = nullptr;
        HIP_TRY(c, hipMalloc((void**)&all, S->RB * (size_t)k * sizeof(fr)));
        int rc = lig_run_batch_program(c, *job, all);
        for (size_t lr = 0; lr < Rl && rc == LIG_OK; lr++)
            if (S->grow[lr] < S->RB && hipMemcpyAsync(S->msgs + lr * (size_t)k, all + S->grow[lr] * (size_t)k, (size_t)k * sizeof(fr), hipMemcpyDeviceToDevice, c->stream) != hipSuccess) rc = LIG_E_HIP;
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(all);
        if (rc != LIG_OK) return rc;
    }
    lig::aes256_expand_host(job->witness_key, rk);
    TRY(lig_internal_upload_small(c, c->rk_dev, rk, sizeof rk, c->stream));
    for (size_t lr = 0; lr < Rl;) {
        const size_t gr = S->grow[lr];
        const RowDesc d = S->rows[gr];
        if (d.kind >= RK_INIT) { lr++; continue; }
        if (d.kind == 0) {
            lig::launch_rng_fill_rows(c->stream, c->rk_dev, S->wit_pos[gr], S->msgs + lr * k, 1, d.data, k, 0, 1, d.data);
            lr += 1;
        } else {          // x, y, z are consecutive locally as well: chunks never split a triple
            lig::launch_rng_fill_rows(c->stream, c->rk_dev, S->wit_pos[gr], S->msgs + lr * k, 2, d.data, k, 0, 1, d.data);
            lig::launch_eltwise(c->stream, LIG_OP_MUL, S->msgs + lr * k, S->msgs + (lr + 1) * k, S->msgs + (lr + 2) * k, d.data, fr{}, 0);
            lr += 3;
        }
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    return LIG_OK;
}

static int shard_alloc(lig_ctx* c, uint32_t rank, uint32_t world, lig_shard* S) {
    const uint32_t k = c->k, n = c->n, t = 192, W = world;
    const size_t R = S->R;
    S->ncol = n / world;
    S->exchange_even_alone = lig::knobs().shard_force_exchange;
    shard_chunks(S->rows, W, S->rounds, S->gb);
    S->G = S->rounds * W;
    for (size_t g = 0; g < S->G; g++) S->ch_cap = std::max(S->ch_cap, S->chunk_rows(g));
    if (!S->ch_cap) S->ch_cap = 1;
    S->lrow0.assign(S->rounds + 1, 0);
    for (size_t cidx = 0; cidx < S->rounds; cidx++) {
        const size_t g = cidx * W + rank;
        for (size_t r = S->gb[g]; r < S->gb[g + 1]; r++) S->grow.push_back(r);
        S->lrow0[cidx + 1] = S->grow.size();
    }
    const size_t Rl = S->Rl = S->grow.size();
    for (uint32_t h = 0; h < W; h++) {
        size_t cnt = 0;
        for (size_t cidx = 0; cidx < S->rounds; cidx++) cnt += S->chunk_rows(cidx * W + h);
        S->rows_max = std::max(S->rows_max, cnt);
    }
    if (!S->rows_max) S->rows_max = 1;
    const size_t RM = S->rows_max;
    std::vector<size_t> local_of(R, (size_t)-1);
    for (size_t lr = 0; lr < Rl; lr++) local_of[S->grow[lr]] = lr;
    {   // quadratic-test terms whose rows are local, with local row indices; triple_ord = position in the quadratic stream
        const std::vector<uint32_t> all = quad_terms(S->rows);
        for (size_t i = 0; i < all.size() / 3; i++) {
            const size_t last = all[3 * i + 2];
            if (local_of[last] == (size_t)-1) continue;
            S->triples.push_back((uint32_t)local_of[all[3 * i]]);
            S->triples.push_back(all[3 * i + 1] == 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)local_of[all[3 * i + 1]]);
            S->triples.push_back((uint32_t)local_of[last]);
            S->triple_ord.push_back(i);
        }
    }
    const size_t chunk = S->ch_cap;
    auto dm = [&](void** p, size_t bytes) -> int { HIP_TRY(c, hipMalloc(p, bytes ? bytes : 16)); HIP_TRY(c, hipMemsetAsync(*p, 0, bytes, c->stream)); return LIG_OK; };
    TRY(dm((void**)&S->msgs, (Rl ? Rl : 1) * (size_t)k * 32));
    TRY(dm((void**)&S->cw, (Rl ? Rl : 1) * 3 * (size_t)k * 32));      // cosets 1..3 of the local codewords as planes
    TRY(dm((void**)&S->maskcw, 3 * (size_t)n * 32));                  // the mask rows' codewords, reference layout
    TRY(dm((void**)&S->send, 2 * chunk * (size_t)n * 32));          // double-buffered: W blocks of chunk x ncol each
    TRY(dm((void**)&S->recv, 2 * chunk * (size_t)n * 32));
    TRY(dm((void**)&S->randb, 2 * chunk * (size_t)k * 32));         // double-buffered
    TRY(dm((void**)&S->rhalf, chunk * 2 * (size_t)k * 32));
    TRY(dm((void**)&S->acc, 4 * (size_t)n * 32));
    TRY(dm((void**)&S->parts, (2 * ((chunk + lig_tune::GROUP / 4 - 1) / (lig_tune::GROUP / 4)) + (chunk + lig_tune::DOT_GROUP - 1) / lig_tune::DOT_GROUP) * (size_t)k * 32));
    TRY(dm((void**)&S->accp, (5 * (size_t)k + 1) * 32));               // (+ 1: a rank's share of the linear system's constant, when one is set)
    TRY(dm((void**)&S->accg, (size_t)world * (5 * (size_t)k + 1) * 32));
    TRY(dm((void**)&S->dots, 32));
    TRY(dm((void**)&S->smp, (RM + 3) * (size_t)t * 32));
    TRY(dm((void**)&S->smpg, (size_t)world * RM * t * 32));
    TRY(dm((void**)&S->sha_state, lig_sha_state_bytes(S->ncol)));
    TRY(dm((void**)&S->leaves_slice, S->ncol * 32));
    TRY(dm((void**)&S->leaves, (size_t)n * 32));
    TRY(dm((void**)&S->nodes, lig_merkle_nodes(n) * 32));
    TRY(dm((void**)&S->tri_dev, (S->triples.size() ? S->triples.size() : 1) * sizeof(uint32_t)));
    TRY(dm((void**)&S->coef_dev, (Rl + 2 * S->triple_ord.size() + 1) * sizeof(lig::f29s)));
    S->h_proof_cap = ((size_t)1 << 19) + 3 * (size_t)n * 32 + (R + 3) * (size_t)t * 32;
    HIP_TRY(c, hipHostMalloc((void**)&S->h_proof, S->h_proof_cap, hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc((void**)&S->h_enc, 3 * (size_t)n * 32, hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc((void**)&S->h_nodes, lig_merkle_nodes(n) * 32, hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc((void**)&S->h_small, (1 + 3 * (size_t)n) * 32, hipHostMallocDefault));
    for (int i = 0; i < 2; i++) {
        HIP_TRY(c, hipEventCreateWithFlags(&S->ev_enc[i], hipEventDisableTiming));
        HIP_TRY(c, hipEventCreateWithFlags(&S->ev_comm[i], hipEventDisableTiming));
        HIP_TRY(c, hipEventCreateWithFlags(&S->ev_hash[i], hipEventDisableTiming));
    }
    if (!S->triples.empty()) HIP_TRY(c, hipMemcpyAsync(S->tri_dev, S->triples.data(), S->triples.size() * 4, hipMemcpyHostToDevice, c->stream));
    TRY(lig_internal_reserve_scratch(c, chunk));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return LIG_OK;
}

// Bounded replacement for hipStreamSynchronize on the error / teardown paths: when a collective failed and neither the
// communicator's abort nor the watchdog released the kernels queued behind it, a blocking synchronize would hang exactly where
// shard_bounded_wait gave up.  Polls the context's streams for `seconds`; false = something is still queued: the shard is poisoned
// (every later call on it returns LIG_E_STATE; lig_shard_destroy keeps the device buffers the queued kernels may still touch).
static bool shard_quiesce(lig_shard* S, double seconds) {
    lig_ctx* c = S->c;
    const auto t0 = clk::now();
    for (unsigned spins = 0;; spins++) {
        bool busy = false;
        for (hipStream_t st : {c->stream, c->stream2, c->stream3}) {
            if (!st) continue;
            const hipError_t e = hipStreamQuery(st);
            if (e == hipErrorNotReady) busy = true; else if (e != hipSuccess) (void)hipGetLastError();
        }
        if (!busy) return true;
        if (spins < 4000) { std::this_thread::yield(); continue; }
        usleep(50);
        if ((spins & 63) == 0 && std::chrono::duration<double>(clk::now() - t0).count() > seconds) { S->poisoned = true; return false; }
    }
}
static constexpr double SHARD_QUIESCE_S = 20.0;
static const char* const SHARD_POISONED_MSG = "; the streams still hold work queued behind the failed collective: the shard is poisoned (rows and randomness rows of this call "
                                              "must stay alive; destroy the shard and do not reuse the context)";
// a failed call: the uploader thread is done with the caller's rows and the streams have drained -- or the shard is poisoned and says so
static void shard_settle(lig_shard* S) { S->up.drain(); if (!shard_quiesce(S, SHARD_QUIESCE_S)) S->c->err += SHARD_POISONED_MSG; }

void lig_shard_destroy(lig_shard* S) {
    if (!S) return;
    (void)hipSetDevice(S->c->device);
    if (!S->poisoned) (void)shard_quiesce(S, SHARD_QUIESCE_S);
    S->up_abort.store(1, std::memory_order_release);
    S->up.drain();                             // the uploader thread is done with our buffers
    if (S->poisoned) {
        // kernels behind a collective that never completed are still queued: they may run (and touch these buffers) whenever the queue is
        // released.  The device and pinned buffers, the events and the flag page outlive the shard; only the host object goes.  (The
        // context's streams are in the same state: destroy the context's process, or at least never reuse the context.)
        S->c->sha.erase(S->sha_state);
        delete S;
        return;
    }
    S->flags.release();
    lig_internal_linear_destroy(S->linear);
    lig_internal_derive_shard_destroy(S->derive);
    (void)hipFree(S->rands_lin);
    // the send buffers below are about to be freed.  forget() may be a host collective (comm_ipc): a shard that fails before its
    // first collective (a local error in *_begin / *_prepare) has exported nothing and must not wait for peers that are not there
    if (S->comm.forget && S->used_comm) S->comm.forget(S->comm.user);
    S->c->sha.erase(S->sha_state);
    for (void* p : {(void*)S->msgs, (void*)S->cw, (void*)S->maskcw, (void*)S->send, (void*)S->recv, (void*)S->randb, (void*)S->rhalf, (void*)S->acc,
                    (void*)S->parts, (void*)S->accp, (void*)S->accg, (void*)S->dots, (void*)S->smp, (void*)S->smpg, (void*)S->sha_state,
                    (void*)S->leaves_slice, (void*)S->leaves, (void*)S->nodes, (void*)S->tri_dev, (void*)S->coef_dev, (void*)S->src_off_dev,
                    (void*)S->widths_dev, (void*)S->packed_dev, (void*)S->prod.dev, (void*)S->wide.mixed.dev, (void*)S->wide.wide_dev, (void*)S->wide.flag_dev, (void*)S->derive_send, (void*)S->derive_import})
        (void)hipFree(p);
    for (void* p : S->derive_retired) (void)hipFree(p);
    for (int i = 0; i < 2; i++)
        for (hipEvent_t e : {S->ev_enc[i], S->ev_comm[i], S->ev_hash[i]}) if (e) (void)hipEventDestroy(e);
    (void)hipHostFree(S->h_proof); (void)hipHostFree(S->h_enc); (void)hipHostFree(S->h_nodes); (void)hipHostFree(S->h_small);
    delete S;
}

// Bounded wait for queued work that contains stream-ordered collectives (round 5: a sharded call returns an error, it never hangs).
// A collective inside a queue cannot time out or report a failure; so the host polls instead of blocking, and
//   * asks lig_comm.failed (comm_ipc: watchdog thread -- dead peer, abort word, stall timer; comm_rccl: ncclCommGetAsyncError):
//     a failed communicator releases / aborts its queued waits, the streams drain, the call returns LIG_E_STATE with the reason;
//   * after LIG_COMM_TIMEOUT_S (default 300 s -- fifty times the longest sharded proof measured) calls lig_comm.abort
//     (ncclCommAbort / poison) itself.
// Without stream-ordered forms (host-synchronous callbacks) the wait is a plain synchronize: nothing of a peer is in the queues.
static int shard_bounded_wait(lig_shard* S, const std::function<hipError_t()>& query, const char* what) {
    lig_ctx* c = S->c;
    const lig_comm& cm = S->comm;
    const auto t0 = clk::now();
    const double limit_s = (double)lig::knobs().comm_timeout_s;
    bool aborted = false, failed = false;
    auto t_fail = t0;
    std::string why;
    S->dbg_wait_since_ms.store((uint64_t)std::chrono::duration_cast<std::chrono::milliseconds>(t0.time_since_epoch()).count(), std::memory_order_release);
    S->dbg_wait.store(what, std::memory_order_release);
    struct Clear { lig_shard* S; ~Clear() { S->dbg_wait.store(nullptr, std::memory_order_release); } } clear_on_exit{S};
    for (unsigned spins = 0;; spins++) {
        const hipError_t e = query();
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) { (void)hipGetLastError(); c->err = std::string(what) + ": " + hipGetErrorString(e); return LIG_E_HIP; }
        if (spins < 4000) { std::this_thread::yield(); continue; }
        usleep(50);
        if ((spins & 63) != 0) continue;
        const auto now = clk::now();
        if (!failed && cm.failed && cm.failed(cm.user)) { failed = true; t_fail = now; why = c->err; }
        if (!failed && !aborted && std::chrono::duration<double>(now - t0).count() > limit_s) {
            aborted = failed = true; t_fail = now;
            why = std::string(what) + ": no completion after " + std::to_string((int)limit_s) + " s (LIG_COMM_TIMEOUT_S)";
            if (cm.abort) cm.abort(cm.user);
        }
        if (failed && std::chrono::duration<double>(now - t_fail).count() > 20.0) {        // the queues did not drain even so: report, leave the rest to the caller
            c->err = "collective failed and the streams did not drain: " + why;
            return LIG_E_STATE;
        }
    }
    if (failed || (cm.failed && cm.failed(cm.user))) {
        if (failed) c->err = why;
        if (c->err.find("ipc comm") == std::string::npos && c->err.find("nccl") == std::string::npos) c->err = "collective failed: " + c->err;
        return LIG_E_STATE;
    }
    return LIG_OK;
}

// where the stage-2 randomness rows of the LOCAL rows come from: generated (dense rows of the synthetic stream) or the caller's
struct ShardRands { const fr* dev = nullptr; const uint8_t* host = nullptr;
                    lig_linear* linear = nullptr; };      // linear: `dev` (= S->rands_lin) is formed from the rank's share of the sparse linear system on the side stream
#define SHARD_COMMON \
    lig_ctx* c = S->c; \
    const uint32_t l = c->l, k = c->k, n = c->n, t = 192, pad = k - l, W = S->world; \
    const size_t R = S->R, Rl = S->Rl, RM = S->rows_max, ncol = S->ncol, CAP = S->ch_cap; \
    hipStream_t s = c->stream, s_hash = c->stream2, s_comm = lig_internal_copy_stream(c); \
    const bool ordered = S->comm.all_to_all_on != nullptr && S->comm.all_gather_on != nullptr; \
    auto comm_fail = [&](const char* what) { if (c->err.find("nccl") == std::string::npos && c->err.find("ipc comm") == std::string::npos && c->err.find("injected fault") == std::string::npos) c->err = std::string("collective failed: ") + what; else c->err = std::string(what) + ": " + c->err; return (int)LIG_E_STATE; }; \
    auto all_gather = [&](const void* src, void* dst, size_t bytes, hipStream_t st, const char* what) -> int { \
        S->used_comm = true; \
        if (ordered) { if (S->comm.all_gather_on(S->comm.user, src, dst, bytes, st)) return comm_fail(what); return LIG_OK; } \
        HIP_TRY(c, hipStreamSynchronize(st)); \
        if (S->comm.all_gather(S->comm.user, src, dst, bytes)) return comm_fail(what); \
        return LIG_OK; \
    }; \
    auto drain = [&](hipStream_t st, const char* what) -> int { \
        if (!ordered) { HIP_TRY(c, hipStreamSynchronize(st)); return LIG_OK; } \
        return shard_bounded_wait(S, [&] { return hipStreamQuery(st); }, what); \
    }; \
    auto drain_event = [&](hipEvent_t ev, const char* what) -> int { \
        if (!ordered) { HIP_TRY(c, hipEventSynchronize(ev)); return LIG_OK; } \
        return shard_bounded_wait(S, [&] { return hipEventQuery(ev); }, what); \
    }; \
    (void)l; (void)pad; (void)RM; (void)t; (void)s_comm; (void)W; (void)Rl; (void)R; (void)CAP; (void)ncol; (void)s_hash; (void)all_gather; (void)drain; (void)drain_event

// what a watchdog prints when it declares the communicator dead while a sharded call is in progress
// (No HIP call in here: it runs on a communicator's watchdog thread under the context's debug mutex, in exactly the situation where the
// runtime may be wedged -- a blocked query would keep the mutex and with it the API call's return.  What the calling thread is waiting
// for is published by shard_bounded_wait in two atomics instead.  ADVICE r5.)
static std::string shard_debug(lig_shard* S, const char* stage, uint32_t rseq) {
    lig_ctx* c = S->c;
    const char* w = S->dbg_wait.load(std::memory_order_acquire);
    const uint64_t now = (uint64_t)std::chrono::duration_cast<std::chrono::milliseconds>(clk::now().time_since_epoch()).count();
    std::string o = std::string("[lig_shard] rank ") + std::to_string(S->rank) + " in " + stage + ": " +
                    (w ? std::string("the calling thread has been waiting for '") + w + "' for " + std::to_string(now - S->dbg_wait_since_ms.load(std::memory_order_acquire)) + " ms"
                       : std::string("the calling thread is enqueueing"));
    o += "; rows upload seq " + std::to_string(S->up.seq) + ", randomness seq " + std::to_string(rseq) + ", pending " + std::to_string(S->up.pending.load()) + ", flag words [arrived rows | arrived rands | consumed]:";
    if (S->flags.host && S->rounds) for (size_t i = 0; i < 3 * S->rounds && i < 24; i++) o += (i % S->rounds == 0 ? " | " : " ") + std::to_string(S->flags.host[i]);
    else o += " none";
    return o + "; " + lig_internal_uploader_state(c->device);
}
struct ShardDebugScope {
    lig_ctx* c;
    ShardDebugScope(lig_shard* S, const char* stage, const uint32_t* rseq) : c(S->c) { lig_internal_set_debug_state(c, [S, stage, rseq] { return shard_debug(S, stage, rseq ? *rseq : 0); }); }
    ~ShardDebugScope() { lig_internal_set_debug_state(c, nullptr); }
};

static int shard_stage1(lig_shard* S, lig_proof_info* info) {
    SHARD_COMMON;
    ShardDebugScope dbg(S, "stage 1", nullptr);
    // ---------------- stage 1
    uint32_t rk[60];
    lig::aes256_expand_host(S->hdr.encoding_seed, rk);
    TRY(lig_internal_upload_small(c, c->rk_dev, rk, sizeof rk, s));
    // pads of the local rows that draw them at commit time (batch init rows carry theirs from the program): the position
    // of a row's pads = number of pad-drawing rows before it in commit order; runs of consecutive rows = one launch
    // (rows that are still arriving from the host -- rows_by_thread -- get theirs round by round below, behind the arrival of the round)
    auto draw_pads = [&](size_t lr0, size_t lr1) {
        for (size_t lr = lr0; lr < lr1;) {
            const size_t gr = S->grow[lr];
            if (!S->draw[gr]) { lr++; continue; }
            size_t run = 1;
            while (lr + run < lr1 && S->grow[lr + run] == gr + run && S->draw[gr + run] && S->enc_pos[gr + run] == S->enc_pos[gr + run - 1] + pad) run++;
            lig::launch_rng_fill_rows(s, c->rk_dev, S->enc_pos[gr], S->msgs + lr * (size_t)k, run, pad, k, l, 1, pad);
            lr += run;
        }
    };
    if (!S->rows_by_thread) draw_pads(0, Rl);
    fr* mask = S->maskcw; fr* mlin = mask + n;                                                           // masks: formed by every rank
    const size_t k3 = 3 * (size_t)k, kq = ncol / 4;                                                      // kq = positions per coset of a rank's columns
    TRY(lig_internal_form_mask_rows(c, s, S->enc_pos[R], mask, S->dots));
    TRY(lig_sha_init(c, S->sha_state, ncol));
    HIP_TRY(c, hipEventRecord(c->ev_fork, s));
    HIP_TRY(c, hipStreamWaitEvent(s_hash, c->ev_fork, 0));
    HIP_TRY(c, hipStreamWaitEvent(s_comm, c->ev_fork, 0));
    // the three mask rows do not depend on the witness: encoded on the hash stream under the first round's encode
    TRY(lig_internal_encode_generic(c, mask, s_hash));
    TRY(lig_internal_encode_2k_rows(c, mlin, 2, s_hash));
    const bool exchange = W > 1 || S->exchange_even_alone;
    // Derived slots (lig_shard_rows_set_derived): the waves read slots of any local row and, through the exchange, of other ranks' rows, so
    // every local row has to be in place first.  Rows that arrive round by round: every round's arrival and pads first -- such a trace gives
    // up the upload / encode overlap.  Per wave on the main stream: export kernel, all-gather (both only when something crosses ranks in
    // that wave, on every rank alike), wave kernel.  Without a list nothing here is queued.
    const bool derive = S->derive != nullptr;
    if (derive) {
        if (S->rows_by_thread)
            for (size_t cidx = 0; cidx < S->rounds; cidx++) {
                HIP_TRY(c, hipStreamWaitValue32(s, S->flags.dev + cidx, S->up.seq, hipStreamWaitValueGte, 0xffffffffu));
                draw_pads(S->lrow0[cidx], S->lrow0[cidx + 1]);
            }
        hipEvent_t e0 = nullptr, e1 = nullptr;                    // lig_profile_read_launches(rows_in_launch = 0): the waves and exchanges of this commit
        TRY(lig_internal_profile_bracket(c, 0, &e0, &e1));
        if (e0) HIP_TRY(c, hipEventRecord(e0, s));
        TRY(lig_internal_derive_shard_run(c, S->derive, S->msgs, S->derive_send, S->derive_import, s,
                                          [&](const void* src, void* dst, size_t bytes, const char* what) -> int { return all_gather(src, dst, bytes, s, what); }));
        if (e1) HIP_TRY(c, hipEventRecord(e1, s));
    }
    const size_t blk_elems = CAP * ncol;                         // one block of the exchange buffers (per rank pair and round)
    uint64_t absorbed = 0;
    for (size_t cidx = 0; cidx < S->rounds; cidx++) {
        const int pb = (int)(cidx & 1);
        const size_t lb = S->lrow0[cidx], nb = S->lrow0[cidx + 1] - lb;
        fr* sendb = S->send + (size_t)pb * CAP * n; fr* recvb = S->recv + (size_t)pb * CAP * n;
        if (S->rows_by_thread && !derive) {                   // my c-th chunk has arrived from the host
            HIP_TRY(c, hipStreamWaitValue32(s, S->flags.dev + cidx, S->up.seq, hipStreamWaitValueGte, 0xffffffffu));
            draw_pads(lb, lb + nb);
        }
        if (nb) TRY(lig_internal_encode_rows(c, S->msgs + lb * (size_t)k, S->cw + lb * k3, nb, lig::ENC_PLANAR, s));
        if (exchange) {
            if (cidx >= 2) HIP_TRY(c, hipStreamWaitEvent(s, S->ev_comm[pb], 0));          // send buffer free again (exchange c-2 done)
            if (nb) hipLaunchKernelGGL(lig::k_pack_slices, dim3(2048), dim3(256), 0, s, lig::CwView{S->msgs + lb * (size_t)k, S->cw + lb * k3, k}, sendb, nb, kq, CAP);
        }
        HIP_TRY(c, hipEventRecord(S->ev_enc[pb], s));
        if (exchange) {
            S->used_comm = true;
            if (ordered) {
                HIP_TRY(c, hipStreamWaitEvent(s_comm, S->ev_enc[pb], 0));
                if (cidx >= 2) HIP_TRY(c, hipStreamWaitEvent(s_comm, S->ev_hash[pb], 0));   // receive buffer free again (hash c-2 done)
                if (S->comm.all_to_all_on(S->comm.user, sendb, recvb, blk_elems * 32, s_comm)) return comm_fail("all_to_all(codeword column slices)");
                HIP_TRY(c, hipEventRecord(S->ev_comm[pb], s_comm));
            } else {
                HIP_TRY(c, hipStreamSynchronize(s));
                HIP_TRY(c, hipStreamSynchronize(s_hash));                               // receive buffer free again
                if (S->comm.all_to_all(S->comm.user, sendb, recvb, blk_elems * 32)) return comm_fail("all_to_all(codeword column slices)");
                HIP_TRY(c, hipEventRecord(S->ev_comm[pb], s));
            }
            HIP_TRY(c, hipStreamWaitEvent(s_hash, S->ev_comm[pb], 0));
            for (uint32_t h = 0; h < W; h++) {               // global chunks cW .. cW+W-1 in rank order = commit order
                const size_t rg = S->chunk_rows(cidx * W + h);
                if (rg) lig::launch_sha_update_rows(s_hash, S->sha_state, ncol, recvb + (size_t)h * blk_elems, ncol, rg, absorbed);
                absorbed += rg;
            }
        } else {                                             // one rank: its codewords are the rows, all columns are its own
            HIP_TRY(c, hipStreamWaitEvent(s_hash, S->ev_enc[pb], 0));
            if (nb) lig::launch_sha_update_rows(s_hash, S->sha_state, ncol, S->cw + lb * k3, 0, nb, absorbed, k, S->msgs + lb * (size_t)k);
            absorbed += nb;
        }
        HIP_TRY(c, hipEventRecord(S->ev_hash[pb], s_hash));
    }
    lig::launch_sha_update_rows(s_hash, S->sha_state, ncol, mask + (size_t)S->rank * ncol, n, 3, absorbed, (uint32_t)kq, nullptr);   // plane-major instances over interleaved rows
    absorbed += 3;
    c->sha[S->sha_state].second = absorbed;
    HIP_TRY(c, hipEventRecord(c->ev_join, s_hash));
    HIP_TRY(c, hipStreamWaitEvent(s, c->ev_join, 0));
    if (exchange && ordered) {                                // the main stream also joins the exchange stream
        HIP_TRY(c, hipEventRecord(c->ev_fork, s_comm));
        HIP_TRY(c, hipStreamWaitEvent(s, c->ev_fork, 0));
    }
    lig::launch_sha_final(s, S->sha_state, ncol, absorbed, S->leaves_slice, (uint32_t)kq);      // plane-major instances -> the rank's leaves in column order
    uint32_t* leaf_level = S->nodes + 8 * ((size_t)n - 1);         // the gathered leaves ARE the last level of the node heap (n is a power of two)
    TRY(all_gather(S->leaves_slice, leaf_level, ncol * 32, s, "all_gather(leaves)"));
    TRY(lig_merkle_build(c, leaf_level, n, S->nodes));
    HIP_TRY(c, hipMemcpyAsync(info->root, S->nodes, 32, hipMemcpyDeviceToHost, s));
    TRY(drain(s, "stage 1 (exchange, column hash, leaves)"));
    if (S->rows_by_thread) {                                  // every round has been waited for: the caller's rows are no longer read
        S->rows_by_thread = false;
        if (const int e = S->up.take_error()) FAIL(c, LIG_E_HIP, std::string("rows upload failed: ") + hipGetErrorString((hipError_t)e));
    }
    stage1_seed(info->root, S->hdr.ih, info->stage1_seed);
    return LIG_OK;
}

static int shard_stage23(lig_shard* S, const ShardRands& rs, const uint8_t* const_sum_given, const uint8_t** proof, size_t* proof_len, lig_proof_info* info) {
    SHARD_COMMON;
    auto t0 = clk::now();
    uint32_t rk[60];
    uint32_t rseq = 0;
    ShardDebugScope dbg(S, "stages 2-3", &rseq);

    // ---------------- stage 2
    const size_t NTl = S->triple_ord.size();
    {   // the draws of the whole trace, the table of the local rows and terms
        const std::vector<lig::f29s> coef = coef_table(draw_coefficients(info->stage1_seed, S->rows), &S->grow, &S->triple_ord);
        TRY(lig_internal_upload_small(c, S->coef_dev, coef.data(), coef.size() * sizeof(lig::f29s), s));
        lig::aes256_expand_host(info->stage1_seed, rk);
        TRY(lig_internal_upload_small(c, c->rk_dev, rk, sizeof rk, s));
    }
    fr* code = S->acc; fr* lin = S->acc + n; fr* quad = S->acc + 2 * (size_t)n; fr* tmp = S->acc + 3 * (size_t)n;
    fr* linH = lin + 2 * (size_t)k; fr* linC = lin + 3 * (size_t)k;
    fr* mask = S->maskcw; fr* mlin = mask + n; fr* mquad = mask + 2 * (size_t)n;       // the mask codewords of stage 1
    const size_t kq = ncol / 4;
    (void)kq;
    HIP_TRY(c, hipMemsetAsync(S->acc, 0, 4 * (size_t)n * 32, s));
    // as in lig_synth_prove: the randomness rows of chunk c+1 are sampled on the side stream (dense rows, double-buffered)
    // while the main stream encodes / accumulates chunk c; group partials persist across chunks, one combine per accumulator
    const uint32_t pg = (uint32_t)((CAP + lig_tune::GROUP / 4 - 1) / (lig_tune::GROUP / 4));
    fr* p_code = S->parts; fr* p_linH = S->parts + (size_t)pg * k; fr* p_linC = S->parts + 2 * (size_t)pg * k;
    const uint32_t dot_groups = (uint32_t)((CAP + lig_tune::DOT_GROUP - 1) / lig_tune::DOT_GROUP);      // p_linC: dot_groups x k
    HIP_TRY(c, hipMemsetAsync(S->parts, 0, (2 * (size_t)pg + dot_groups) * k * 32, s));
    HIP_TRY(c, hipEventRecord(c->ev_fork, s));                 // key + memsets above
    HIP_TRY(c, hipStreamWaitEvent(s_hash, c->ev_fork, 0));
    // as in lig_synth_prove: the sampler also accumulates the message-domain halves of the code / linear tests (k_rand_rlc)
    const bool fused_rlc = !rs.dev && !rs.host && (k % 256 == 0) && lig::knobs().fused_rlc;
    // the caller's randomness rows (lig_shard_rows_prove): device rows are used in place, host rows go through the double buffer
    auto rand_buf = [&](size_t cidx) -> fr* { return rs.dev ? const_cast<fr*>(rs.dev) + S->lrow0[cidx] * (size_t)k : S->randb + (cidx & 1) * CAP * (size_t)k; };
    // host rows: the uploader thread fills the double buffer round by round (prover.hip, prove_stage23: same scheme -- arrival and
    // consumption are words in pinned host memory, no copy or event of the transfer in a queue of the proof)
    // (default off in the sharded entry, see shard_rows_load: event-chained copies on the side stream instead)
    const bool rands_by_thread = rs.host && lig::knobs().shard_uploader && lig::knobs().upload_mode == 2 && lig::knobs().rands_upload_mode == 2 && lig_internal_uploader_available(c) && S->rounds;
    const lig::FlagLayout fl = lig::shard_flags(S->rounds);
    if (rands_by_thread) {
        TRY(S->flags.ensure(c, fl.words));
        rseq = ++S->rand_seq;
        S->up_abort.store(0, std::memory_order_release);
        std::vector<lig::UploadChunk> chunks;
        for (size_t cidx = 0; cidx < S->rounds; cidx++) chunks.push_back({(uint8_t*)rand_buf(cidx), rs.host + S->lrow0[cidx] * (size_t)k * 32, (S->lrow0[cidx + 1] - S->lrow0[cidx]) * (size_t)k * 32});
        lig_internal_uploader_submit(c->device, lig::chunk_jobs(chunks, S->flags.host + fl.rands, rseq, &S->up.failed, S->flags.host + fl.consumed, &S->up_abort, 1), &S->up.pending);
    }
    auto form_rand_chunk = [&](size_t cidx) -> int {           // on the side stream
        const size_t lb = S->lrow0[cidx], nb = S->lrow0[cidx + 1] - lb;
        fr* rb = rand_buf(cidx);
        if (rs.dev) { HIP_TRY(c, hipEventRecord(S->ev_enc[cidx & 1], s_hash)); return LIG_OK; }
        if (rands_by_thread) return LIG_OK;
        if (cidx >= 2) HIP_TRY(c, hipStreamWaitEvent(s_hash, S->ev_comm[cidx & 1], 0));        // buffer consumed (event reused: stage 1 is over)
        if (rs.host) {
            if (nb) HIP_TRY(c, hipMemcpyAsync(rb, rs.host + lb * (size_t)k * 32, nb * (size_t)k * 32, hipMemcpyHostToDevice, s_hash));
            HIP_TRY(c, hipEventRecord(S->ev_enc[cidx & 1], s_hash));
            return LIG_OK;
        }
        for (size_t r = 0; r < nb;) {          // a chunk is a run of consecutive global rows: runs of equal fill are contiguous in the linear stream
            size_t run = 1;
            const size_t gr = S->grow[lb + r];
            const uint32_t d = S->rows[gr].data;
            while (r + run < nb && S->rows[gr + run].data == d) run++;
            if (fused_rlc) lig::launch_rand_rlc(s_hash, c->rk_dev, S->lin_pos[gr], rb + r * k, S->msgs + (lb + r) * (size_t)k, run, d, k, S->coef_dev + lb + r, lig_tune::GROUP / 4, p_code, p_linH);
            else lig::launch_rng_fill_rows_dense(s_hash, c->rk_dev, S->lin_pos[gr], rb + r * k, run, d, k);
            r += run;
        }
        HIP_TRY(c, hipEventRecord(S->ev_enc[cidx & 1], s_hash));
        return LIG_OK;
    };
    // sparse linear system: the rank's local randomness matrix is formed on the side stream (the constraints its rows need are sampled
    // through the need list, one pass in slot order: linear.hip); the row loop below then finds it where device rows of the caller would be
    if (rs.linear) {
        TRY(lig_internal_linear_form(c, rs.linear, c->rk_dev, const_cast<fr*>(rs.dev), s_hash));
        HIP_TRY(c, hipEventRecord(c->ev_fork, s_hash));       // (its wait above is queued: the event is free) -- the main stream waits for it before it reads the rank's share
    }
    if (S->rounds) TRY(form_rand_chunk(0));
    for (size_t cidx = 0; cidx < S->rounds; cidx++) {
        const size_t lb = S->lrow0[cidx], nb = S->lrow0[cidx + 1] - lb;
        fr* rb = rand_buf(cidx);
        if (cidx + 1 < S->rounds) TRY(form_rand_chunk(cidx + 1));
        if (rands_by_thread) HIP_TRY(c, hipStreamWaitValue32(s, S->flags.dev + fl.rands + cidx, rseq, hipStreamWaitValueGte, 0xffffffffu));
        else HIP_TRY(c, hipStreamWaitEvent(s, S->ev_enc[cidx & 1], 0));
        if (nb) {
            if (c->fast) {      // as in lig_synth_prove: coset-2 values times the codewords' coset-2 plane inside the encoder's output kernel
                TRY(lig_internal_encode_dot(c, rb, nb, S->cw + lb * 3 * (size_t)k + k, 3 * (size_t)k, lig_tune::DOT_GROUP, p_linC));
            } else {
                TRY(lig_internal_encode_rows(c, rb, S->rhalf, nb, lig::ENC_HALF));
                lig::launch_rlc_accumulate29(s, S->cw + lb * 3 * (size_t)k + k, 3 * (size_t)k, 1, S->rhalf, k, nb, k, nullptr, nullptr, p_linC, lig_tune::DOT_GROUP);
            }
            if (!fused_rlc) lig::launch_rlc_accumulate29(s, S->msgs + lb * (size_t)k, k, 1, rb, k, nb, k, S->coef_dev + lb, p_code, p_linH, lig_tune::GROUP / 4);
        }
        if (rands_by_thread) HIP_TRY(c, hipStreamWriteValue32(s, S->flags.dev + fl.consumed + cidx, rseq, 0));      // consumed: its half of the buffer is free
        else HIP_TRY(c, hipEventRecord(S->ev_comm[cidx & 1], s));
    }
    lig::launch_rlc_combine(s, tmp, p_code, pg, k);
    lig::launch_rlc_combine(s, linH, p_linH, pg, k);
    lig::launch_rlc_combine(s, linC, p_linC, dot_groups, k);
    lig::launch_lin_interleave(s, lin, linH, linC, k);       // see lig_synth_prove: even points of <w_n^2> = message domain
    const lig::CwView view{S->msgs, S->cw, k};
    lig::launch_quad_rows29_view(s, view, 2 * k, S->tri_dev, S->coef_dev + Rl, S->coef_dev + Rl + NTl, NTl, quad, S->parts, 2 * (size_t)pg * k);
    // partial sums [code (k message values) | lin (2k) | quad (2k)] -> every rank -> added mod p (one rank: they are the sums)
    // With a linear system the rank's share of sum_c b_c r_c travels as one more element: the W shares are added in rank order like the
    // accumulators.  Without a system the all-gather carries exactly 5k elements.
    const size_t acc_elems = 5 * (size_t)k + (rs.linear ? 1 : 0);
    if (rs.linear) HIP_TRY(c, hipStreamWaitEvent(s, c->ev_fork, 0));      // the form on the side stream has written the share
    if (W > 1 || S->exchange_even_alone) {
        HIP_TRY(c, hipMemcpyAsync(S->accp, tmp, (size_t)k * 32, hipMemcpyDeviceToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(S->accp + k, lin, 2 * (size_t)k * 32, hipMemcpyDeviceToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(S->accp + 3 * (size_t)k, quad, 2 * (size_t)k * 32, hipMemcpyDeviceToDevice, s));
        if (rs.linear) HIP_TRY(c, hipMemcpyAsync(S->accp + 5 * (size_t)k, lig_internal_linear_partial_dev(rs.linear), 32, hipMemcpyDeviceToDevice, s));
        TRY(all_gather(S->accp, S->accg, acc_elems * 32, s, "all_gather(partial accumulators)"));
        HIP_TRY(c, hipMemsetAsync(S->accp, 0, acc_elems * 32, s));
        lig::launch_rlc_combine(s, S->accp, S->accg, W, (uint32_t)acc_elems);
        if (rs.linear) HIP_TRY(c, hipMemcpyAsync(lig_internal_linear_const_buf(rs.linear), S->accp + 5 * (size_t)k, 32, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemsetAsync(S->acc, 0, 4 * (size_t)n * 32, s));
        HIP_TRY(c, hipMemcpyAsync(tmp, S->accp, (size_t)k * 32, hipMemcpyDeviceToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(lin, S->accp + k, 2 * (size_t)k * 32, hipMemcpyDeviceToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(quad, S->accp + 3 * (size_t)k, 2 * (size_t)k * 32, hipMemcpyDeviceToDevice, s));
    } else {
        HIP_TRY(c, hipMemsetAsync(lin + 2 * (size_t)k, 0, (size_t)(n - 2 * k) * 32, s));      // linH / linC scratch behind the 2k values
        if (rs.linear) HIP_TRY(c, hipMemcpyAsync(lig_internal_linear_const_buf(rs.linear), lig_internal_linear_partial_dev(rs.linear), 32, hipMemcpyDeviceToHost, s));   // one rank: its share is the sum
    }
    H::Fr* dots = reinterpret_cast<H::Fr*>(S->h_small);
    lig::launch_sum_elems(s, lin, k, 2, S->dots, nullptr);   // linear-test constant = -(sum of the message-domain half: the even points)
    HIP_TRY(c, hipMemcpyAsync(dots, S->dots, 32, hipMemcpyDeviceToHost, s));
    // as in lig_synth_prove: each accumulator is extended, masked and sent to the host as soon as it is final; the host absorbs
    // it into the stage-2 seed hash (sequential SHA-256 over 3 MiB) while the GPU extends the next one and runs the decodes
    uint8_t* enc = S->h_enc;
    const size_t vec_bytes = (size_t)n * 32, enc_bytes = 3 * vec_bytes;
    hipEvent_t ev_acc[3] = {S->ev_enc[0], S->ev_enc[1], S->ev_hash[0]};      // stage 1 is over: its events are free
    TRY(lig_internal_encode_rows(c, tmp, code, 1, false));
    lig::launch_eltwise(s, LIG_OP_ADD_ASSIGN, mask, nullptr, code, n, fr{}, 0);
    HIP_TRY(c, hipMemcpyAsync(enc, code, vec_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipEventRecord(ev_acc[0], s));
    TRY(lig_internal_extend_2k(c, lin));
    lig::launch_eltwise(s, LIG_OP_ADD_ASSIGN, mlin, nullptr, lin, n, fr{}, 0);
    HIP_TRY(c, hipMemcpyAsync(enc + vec_bytes, lin, vec_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipEventRecord(ev_acc[1], s));
    TRY(lig_internal_extend_2k(c, quad));
    lig::launch_eltwise(s, LIG_OP_ADD_ASSIGN, mquad, nullptr, quad, n, fr{}, 0);
    HIP_TRY(c, hipMemcpyAsync(enc + 2 * vec_bytes, quad, vec_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipEventRecord(ev_acc[2], s));
    H::Fr* dec = reinterpret_cast<H::Fr*>(S->h_small + 32);
    const fr* accs[3] = {code, lin, quad};
    for (int a3 = 0; a3 < 3; a3++) {
        TRY(lig_internal_decode_to(c, accs[a3], tmp));
        HIP_TRY(c, hipMemcpyAsync(dec + (size_t)a3 * n, tmp, vec_bytes, hipMemcpyDeviceToHost, s));
    }
    const size_t n_nodes = lig_merkle_nodes(n);
    HIP_TRY(c, hipMemcpyAsync(S->h_nodes, S->nodes, n_nodes * 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipEventRecord(c->ev_join, s));
    {
        Sha256 h2;
        h2.add("LigetronStage2", 15).add(info->root, 32);
        for (int a3 = 0; a3 < 3; a3++) {
            TRY(drain_event(ev_acc[a3], "stage 2 (accumulators)"));
            h2.add(enc + (size_t)a3 * vec_bytes, vec_bytes);
        }
        h2.finish(info->stage2_seed);
    }
    (void)enc_bytes;
    if (const_sum_given) std::memcpy(info->const_sum, const_sum_given, 32);     // the caller's public constant (linear_sums)
    else if (rs.linear) {                                     // the statement's own constant: minus the ranks' shares of sum_c b_c r_c (copied before ev_acc[0])
        H::Fr sum;
        std::memcpy(sum.v, lig_internal_linear_const_buf(rs.linear), 32);
        sum = H::neg(sum);
        std::memcpy(info->const_sum, sum.v, 32);
    } else {
        const H::Fr sum = H::neg(dots[0]);                    // (copied before ev_acc[0])
        std::memcpy(info->const_sum, sum.v, 32);
    }
    const std::vector<uint32_t> idx = sample_columns(info->stage2_seed, n, t);
    TRY(lig_sample_init(c, idx.data(), idx.size()));
    TRY(drain_event(c->ev_join, "stage 2 (decodes)"));     // decoded accumulators and Merkle nodes are on the host
    const SelfCheck ok = self_check(dec, info->const_sum, l, k, n);
    info->valid_code = ok.valid_code; info->valid_linear = ok.valid_linear; info->valid_quad = ok.valid_quad;
    const std::vector<uint8_t> sib = decommit(S->h_nodes, (n_nodes + 1) / 2, idx);
    info->ms_stage2 = ms_since(t0);
    t0 = clk::now();

    // ---------------- stage 3
    lig::launch_gather_rows_planar(s, view, Rl, c->sample_idx, t, S->smp);                      // local rows, then the 3 masks
    lig::launch_gather_rows(s, S->maskcw, n, 3, c->sample_idx, t, S->smp + Rl * (size_t)t);
    TRY(all_gather(S->smp, S->smpg, RM * (size_t)t * 32, s, "all_gather(opened columns)"));
    const size_t smp_bytes = (R + 3) * (size_t)t * 32;
    const EnvelopeLayout lay = write_envelope(S->h_proof, S->h_proof_cap, S->hdr.version, S->hdr.program_hash, S->hdr.generated_at, k, n, t,
                                              info->root, sib, idx, enc, smp_bytes);
    if (lay.total > S->h_proof_cap) FAIL(c, LIG_E_NOMEM, "proof buffer too small");
    // opened columns in commit order: global chunk g = the (g / W)-th chunk of rank g mod W
    std::vector<size_t> taken(W, 0);
    uint8_t* dst = S->h_proof + lay.samples_off;
    for (size_t g = 0; g < S->G; g++) {
        const uint32_t h = (uint32_t)(g % W);
        const size_t rg = S->chunk_rows(g);
        if (rg) HIP_TRY(c, hipMemcpyAsync(dst, S->smpg + ((size_t)h * RM + taken[h]) * t, rg * (size_t)t * 32, hipMemcpyDeviceToHost, s));
        taken[h] += rg;
        dst += rg * (size_t)t * 32;
    }
    HIP_TRY(c, hipMemcpyAsync(dst, S->smp + Rl * (size_t)t, 3 * (size_t)t * 32, hipMemcpyDeviceToHost, s));
    TRY(drain(s, "stage 3 (opened columns)"));
    *proof = S->h_proof;
    *proof_len = lay.total;
    info->ms_stage3 = ms_since(t0);
    HIP_TRY(c, hipGetLastError());
    return LIG_OK;
}

int lig_shard_prove(lig_shard* S, const uint8_t** proof, size_t* proof_len, lig_proof_info* info) {
    if (!S || !proof || !proof_len || !info) return LIG_E_ARG;
    lig_ctx* c = S->c;
    CHECK_CTX(c);
    if (S->poisoned) FAIL(c, LIG_E_STATE, "lig_shard_prove: the shard is poisoned (work queued behind a failed collective never drained): destroy it");
    if (S->from_rows) FAIL(c, LIG_E_STATE, "lig_shard_prove on a shard made by lig_shard_rows_begin (use lig_shard_rows_commit / _prove)");
    std::memset(info, 0, sizeof *info);
    info->rows = S->R + 3;
    const auto t_begin = clk::now();
    TRY(shard_stage1(S, info));
    info->ms_stage1 = ms_since(t_begin);
    TRY(shard_stage23(S, ShardRands{}, nullptr, proof, proof_len, info));
    info->ms_total = ms_since(t_begin);
    return LIG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The sharded prover over rows SUPPLIED BY THE CALLER (include/lig_hip.h: lig_shard_rows_*): what lig_rows_* is to
// lig_synth_*, for one trace over the GPUs of a node.  Every rank passes the kinds of ALL committed rows (the deal and the
// stream positions are global) and the message rows of ITS chunks only, in commit order; after the commit every rank's
// constraint generator derives the randomness rows of its own rows from the stage-1 seed.
// Replaces the per-row callbacks of include/zkp/nonbatch_context.hpp:445-471 (stage 1), :654-780 (stage 2), :924-970 (stage 3).

int lig_shard_rows_plan(const uint8_t* kinds, size_t n_rows, uint32_t world, uint64_t* rounds_out, uint64_t* boundaries, size_t cap) {
    if ((n_rows && !kinds) || !world || !rounds_out) return LIG_E_ARG;
    std::vector<RowDesc> rows(n_rows);
    for (size_t r = 0; r < n_rows; r++) rows[r] = RowDesc{(uint8_t)(kinds[r] & 0x7f), 0};
    size_t rounds = 0;
    std::vector<size_t> gb;
    shard_chunks(rows, world, rounds, gb);
    *rounds_out = rounds;
    if (gb.size() > cap || !boundaries) return gb.size() > cap ? LIG_E_NOMEM : LIG_E_ARG;
    for (size_t i = 0; i < gb.size(); i++) boundaries[i] = gb[i];
    return LIG_OK;
}

// local rows of a rows job -> S->msgs.  Device rows: one copy on the main stream.  Host rows: round by round through the uploader
// thread -- lig_shard_rows_commit encodes my c-th chunk as soon as it has arrived (the caller's memory must stay valid until then).
static int shard_rows_load(lig_shard* S, const void* local_msgs, bool on_device) {
    lig_ctx* c = S->c;
    if (S->Rl && !local_msgs) FAIL(c, LIG_E_ARG, "sharded rows job: null local rows");
    if (!on_device && S->wide.any())                   // mixed host rows: the records are read before any copy starts
        if (const char* why = lig::wide_records_refusal((const uint8_t*)local_msgs, S->src_off, S->wide.mixed.rows, S->wide.wide, c->l)) FAIL(c, LIG_E_ARG, std::string("sharded rows job: ") + why);
    S->up.drain();                                     // an upload nobody committed
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // the previous trace is done with S->msgs
    S->committed = false;
    S->diag_ok = false;
    S->rows_by_thread = false;
    if (!S->Rl) return LIG_OK;
    const size_t row_bytes = (size_t)c->k * 32;
    if (S->narrow) {
        // narrow rows: the packed bytes are copied to the staging buffer synchronously (the lifetime contract holds unchanged; the
        // uploader path is not taken even with LIG_SHARD_UPLOADER=1), device rows are read where they are; then expanded into
        // S->msgs on the main stream, ahead of everything lig_shard_rows_commit queues there
        const uint8_t* src = (const uint8_t*)local_msgs;
        if (!on_device) {
            if (!S->packed_dev) HIP_TRY(c, hipMalloc((void**)&S->packed_dev, S->src_off[S->Rl] ? S->src_off[S->Rl] : 16));   // first host rows
            if (S->src_off[S->Rl]) HIP_TRY(c, hipMemcpyAsync(S->packed_dev, local_msgs, S->src_off[S->Rl], hipMemcpyHostToDevice, c->stream));
            src = S->packed_dev;
        }
        const bool wide_flag = on_device && S->wide.any();      // the host has not seen the records of device rows: k_expand_wide raises a word
        if (wide_flag) HIP_TRY(c, hipMemsetAsync(S->wide.flag_dev, 0, sizeof(uint32_t), c->stream));
        lig::launch_expand_rows(c->stream, src, S->src_off_dev, S->widths_dev, 0, S->Rl, c->l, c->k, S->msgs, S->prod.dev, S->prod.rows.size(), S->wide.args(0, S->Rl));
        HIP_TRY(c, hipGetLastError());
        uint32_t raised = 0;
        if (wide_flag) HIP_TRY(c, hipMemcpyAsync(&raised, S->wide.flag_dev, sizeof raised, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));  // the caller's memory is no longer referenced
        // (refused here, before any collective is queued: no peer is left waiting)
        if (raised) FAIL(c, LIG_E_ARG, "sharded rows job: a wide slot of the device rows names a column >= l (lig_rows_job.wide_per_row)");
        return LIG_OK;
    }
    // Host rows are copied HERE, synchronously (as in round 3).  Round 4 had moved them onto the library's uploader thread with a stream
    // memory wait per round (what lig_rows_* does on ONE GPU, where it buys the link rate): with several PROCESSES on one device -- the only
    // way this entry runs on the one-GPU test box -- a DMA transfer that is started while the process's main stream holds a pending
    // hipStreamWaitValue32 sometimes never completes (profiles/r05_rows_entry_hang.md: 15 % of the runs, the GPUTEST hang of round 4).
    // LIG_SHARD_UPLOADER=1 restores the round-4 path (reproduction / a node where every rank has its own GPU).
    if (!on_device && lig::knobs().shard_uploader && lig::knobs().upload_mode == 2 && lig_internal_uploader_available(c)) {
        TRY(S->flags.ensure(c, lig::shard_flags(S->rounds).words));
        S->up.seq++;
        S->up_abort.store(0, std::memory_order_release);
        std::vector<lig::UploadChunk> chunks;
        for (size_t cidx = 0; cidx < S->rounds; cidx++) chunks.push_back({(uint8_t*)S->msgs + S->lrow0[cidx] * row_bytes, (const uint8_t*)local_msgs + S->lrow0[cidx] * row_bytes, (S->lrow0[cidx + 1] - S->lrow0[cidx]) * row_bytes});
        lig_internal_uploader_submit(c->device, lig::chunk_jobs(chunks, S->flags.host, S->up.seq, &S->up.failed), &S->up.pending);
        S->rows_by_thread = true;
        return LIG_OK;
    }
    HIP_TRY(c, hipMemcpyAsync(S->msgs, local_msgs, S->Rl * row_bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // the caller's memory is no longer referenced
    return LIG_OK;
}

int lig_shard_rows_begin(lig_ctx* c, const lig_rows_job* job, uint32_t rank, uint32_t world, const lig_comm* comm, lig_shard** out) {
    CHECK_CTX(c);
    if (!job || !out || !comm || world == 0 || rank >= world) return LIG_E_ARG;
    if (!comm->all_to_all || !comm->all_gather) return LIG_E_ARG;
    if (job->rows && !job->kinds) FAIL(c, LIG_E_ARG, "sharded rows job: null kinds");
    const uint32_t l = c->l, k = c->k, n = c->n, t = 192;
    if (l >= k || l < 2 || t > n || k - l < t || k % world) FAIL(c, LIG_E_ARG, "sharded trace: need 2 <= l <= k - 192 and world | k");
    *out = nullptr;
    lig_shard* S = new lig_shard();
    S->c = c; S->comm = *comm; S->rank = rank; S->world = world; S->from_rows = true;
    std::memset(&S->job, 0, sizeof S->job);
    S->dense_rands = job->dense_rands_per_row != nullptr;
    auto fail = [&](int rc) { lig_shard_destroy(S); return rc; };
    if (!fill_job_header(*job, S->hdr)) return fail(LIG_E_ARG);
    if (const char* why = lig::parse_row_kinds(*job, l, k, true, S->rows, S->draw, S->enc_pos)) { c->err = std::string("rows job: ") + why; return fail(LIG_E_ARG); }
    const size_t R = S->R = S->rows.size();
    S->lin_pos.assign(R + 1, 0); S->wit_pos.assign(R + 1, 0);
    for (size_t r = 0; r < R; r++) S->lin_pos[r + 1] = S->lin_pos[r] + S->rows[r].data;
    if (job->elem_bytes) S->elem_bytes_all.assign(job->elem_bytes, job->elem_bytes + R);
    int rc = shard_alloc(c, rank, world, S);
    if (rc == LIG_OK && (job->elem_bytes || lig::job_wide_per_row(*job))) {
        // the narrow row format: every row of the job is checked as lig_rows_begin does, the plan is of the local rows; the staging
        // buffer of host rows is allocated by the first load from host memory (device rows are expanded where they are)
        lig::NarrowPlan np;
        if (const char* why = lig::plan_narrow_rows(job->elem_bytes, S->rows, S->draw, l, k, S->grow, np, lig::job_wide_per_row(*job))) { c->err = std::string("sharded rows job: ") + why; rc = LIG_E_ARG; }
        else if ((S->narrow = np.packed)) {
            rc = lig_internal_upload_narrow_plan(c, np, &S->src_off_dev, &S->widths_dev, &S->prod, &S->wide);
            S->src_off = std::move(np.src_off);
        }
    }
    if (rc == LIG_OK) rc = shard_rows_load(S, job->msgs, job->msgs_on_device != 0);
    if (rc != LIG_OK) return fail(rc);
    *out = S;
    return LIG_OK;
}
// the next trace of the same shape: new local rows into the same buffers
int lig_shard_rows_restart(lig_shard* S, const void* local_msgs, int msgs_on_device) {
    if (!S) return LIG_E_ARG;
    lig_ctx* c = S->c;
    CHECK_CTX(c);
    if (S->poisoned) FAIL(c, LIG_E_STATE, "lig_shard_rows_restart: the shard is poisoned (work queued behind a failed collective never drained): destroy it");
    if (!S->from_rows) FAIL(c, LIG_E_STATE, "lig_shard_rows_restart: not a rows shard");
    // (unlike lig_rows_restart there is no second message matrix here: stage 2 of a committed trace still reads the local rows)
    if (S->committed) FAIL(c, LIG_E_STATE, "lig_shard_rows_restart: the committed trace has not been proved yet");
    return shard_rows_load(S, local_msgs, msgs_on_device != 0);
}
int lig_shard_rows_commit(lig_shard* S, uint8_t root[32], uint8_t stage1_seed[32]) {
    if (!S) return LIG_E_ARG;
    lig_ctx* c = S->c;
    CHECK_CTX(c);
    if (S->poisoned) FAIL(c, LIG_E_STATE, "lig_shard_rows_commit: the shard is poisoned (work queued behind a failed collective never drained): destroy it");
    if (!S->from_rows) FAIL(c, LIG_E_STATE, "lig_shard_rows_commit: not a rows shard");
    if (S->committed) FAIL(c, LIG_E_STATE, "lig_shard_rows_commit: the committed trace has not been proved yet");
    std::memset(&S->info1, 0, sizeof S->info1);
    S->info1.rows = S->R + 3;
    const auto t_begin = clk::now();
    {
        const int rc = shard_stage1(S, &S->info1);
        if (rc != LIG_OK) {               // the caller is told it may free its rows
            shard_settle(S);
            S->rows_by_thread = false;
            return rc;
        }
    }
    S->info1.ms_stage1 = ms_since(t_begin);
    S->committed = true;
    S->diag_ok = true;
    if (root) std::memcpy(root, S->info1.root, 32);
    if (stage1_seed) std::memcpy(stage1_seed, S->info1.stage1_seed, 32);
    return LIG_OK;
}
int lig_shard_rows_prove(lig_shard* S, const void* local_rands, int rands_on_device, const uint8_t const_sum[32], const uint8_t** proof,
                         size_t* proof_len, lig_proof_info* info) {
    if (!S || !proof || !proof_len || !info) return LIG_E_ARG;
    lig_ctx* c = S->c;
    CHECK_CTX(c);
    if (S->poisoned) FAIL(c, LIG_E_STATE, "lig_shard_rows_prove: the shard is poisoned (work queued behind a failed collective never drained): destroy it");
    if (!S->from_rows || !S->committed) FAIL(c, LIG_E_STATE, "lig_shard_rows_prove: lig_shard_rows_commit has not run on this shard");
    if (S->linear && local_rands) FAIL(c, LIG_E_ARG, "lig_shard_rows_prove: randomness rows given while a linear system is set (lig_shard_rows_set_linear)");
    if (S->Rl && !local_rands && !S->dense_rands && !S->linear) FAIL(c, LIG_E_ARG, "lig_shard_rows_prove: null randomness rows");
    if (const_sum) {
        H::Fr v;
        std::memcpy(v.v, const_sum, 32);
        if (H::geq(v, H::P)) FAIL(c, LIG_E_ARG, "lig_shard_rows_prove: constant not reduced mod p");
    }
    *info = S->info1;
    const auto t_begin = clk::now();
    ShardRands rs;
    if (local_rands && rands_on_device) rs.dev = (const fr*)local_rands; else if (local_rands) rs.host = (const uint8_t*)local_rands;
    else if (S->linear) { rs.dev = S->rands_lin; rs.linear = S->linear; }
    {
        const int rc = shard_stage23(S, rs, const_sum, proof, proof_len, info);
        if (rc != LIG_OK) {               // randomness-row copies the uploader thread still holds read the caller's memory: drop them, wait
            S->up_abort.store(1, std::memory_order_release);
            shard_settle(S);
            return rc;
        }
        if (rs.host) {
            S->up.drain();
            if (const int e = S->up.take_error()) FAIL(c, LIG_E_HIP, std::string("randomness rows upload failed: ") + hipGetErrorString((hipError_t)e));
        }
    }
    info->ms_total = info->ms_stage1 + ms_since(t_begin);
    S->committed = false;
    return LIG_OK;
}

// what diagnose.hip needs of a rows shard for a collective call (lig_diag_shard, prover_common.hpp); inside a function that began with SHARD_COMMON
#define SHARD_DIAG_VIEW(v) \
    lig_diag_shard v; \
    v.msgs = S->msgs; v.grow = &S->grow; v.rows_global = R; v.tri_dev = S->tri_dev; v.triple_ord = &S->triple_ord; \
    v.n_terms_global = quad_terms(S->rows).size() / 3; \
    v.rank = S->rank; v.world = W; v.slice = lig::knobs().diag_slice; \
    v.all_to_all = [&](const void* src, void* dst, size_t block_bytes, const char* what) -> int { \
        S->used_comm = true; \
        if (ordered) { if (S->comm.all_to_all_on(S->comm.user, src, dst, block_bytes, s)) return comm_fail(what); return LIG_OK; } \
        HIP_TRY(c, hipStreamSynchronize(s)); \
        if (S->comm.all_to_all(S->comm.user, src, dst, block_bytes)) return comm_fail(what); \
        return LIG_OK; \
    }; \
    v.all_gather = [&](const void* src, void* dst, size_t bytes, const char* what) -> int { return all_gather(src, dst, bytes, s, what); }; \
    v.drain = [&](const char* what) -> int { return drain(s, what); }; \
    v.settle_failed = [&]() -> bool { shard_settle(S); return S->poisoned; }; \
    v.forget = [&] { if (S->comm.forget) S->comm.forget(S->comm.user); };

// Which constraints does the committed witness violate, on a rows shard (diagnose.hip): collective, every rank obtains the bytes of
// lig_rows_diagnose on the whole trace.  Everything that can be refused is refused here, on the host, identically on every rank, before
// anything is launched and before any collective.
int lig_shard_rows_diagnose(lig_shard* S, const lig_linear_system* sys, lig_diag_linear* lin_out, uint64_t lin_cap, lig_diag_quad* quad_out, uint64_t quad_cap,
                            lig_diag_info* info) {
    if (!S || !info || info->struct_bytes < sizeof(lig_diag_info)) return LIG_E_ARG;
    if ((lin_cap && !lin_out) || (quad_cap && !quad_out)) return LIG_E_ARG;
    const auto t_begin = clk::now();
    SHARD_COMMON;
    (void)n;
    CHECK_CTX(c);
    if (S->poisoned) FAIL(c, LIG_E_STATE, "lig_shard_rows_diagnose: the shard is poisoned (work queued behind a failed collective never drained): destroy it");
    if (!S->from_rows) FAIL(c, LIG_E_STATE, "lig_shard_rows_diagnose: not a rows shard (lig_shard_rows_begin)");
    if (!S->diag_ok) FAIL(c, LIG_E_STATE, "lig_shard_rows_diagnose: no committed matrix (between lig_shard_rows_commit and the next lig_shard_rows_restart)");
    if (sys && lig_linear_check(sys, kinds_of(S->rows).data(), R, l) != LIG_OK) FAIL(c, LIG_E_ARG, "lig_shard_rows_diagnose: linear system rejected by lig_linear_check");
    const uint32_t struct_bytes = info->struct_bytes;
    std::memset(info, 0, sizeof *info);
    info->struct_bytes = struct_bytes;
    ShardDebugScope dbg(S, "diagnose", nullptr);
    if (W == 1 && !S->exchange_even_alone) {       // one rank holds every row in commit order: the one-GPU pass, no collective
        TRY(lig_internal_rows_diagnose(c, S->msgs, R, S->tri_dev, S->triple_ord.size(), sys, lin_out, lin_cap, quad_out, quad_cap, info));
        info->ms_total = ms_since(t_begin);
        return LIG_OK;
    }
    SHARD_DIAG_VIEW(v);
    TRY(lig_internal_shard_diagnose(c, v, sys, lin_out, lin_cap, quad_out, quad_cap, info));
    info->ms_total = ms_since(t_begin);
    return LIG_OK;
}

// lig_shard_rows_diagnose against the share of the system ATTACHED to the shard (lig_shard_rows_set_linear), with the values of
// lig_shard_rows_set_linear_values in force: no term list, no host pass, no upload (diagnose.hip).  Window, refusals and poisoning as above.
int lig_shard_rows_diagnose_attached(lig_shard* S, lig_diag_linear* lin_out, uint64_t lin_cap, lig_diag_quad* quad_out, uint64_t quad_cap, lig_diag_info* info) {
    if (!S || !info || info->struct_bytes < sizeof(lig_diag_info)) return LIG_E_ARG;
    if ((lin_cap && !lin_out) || (quad_cap && !quad_out)) return LIG_E_ARG;
    const auto t_begin = clk::now();
    SHARD_COMMON;
    (void)n;
    CHECK_CTX(c);
    if (S->poisoned) FAIL(c, LIG_E_STATE, "lig_shard_rows_diagnose_attached: the shard is poisoned (work queued behind a failed collective never drained): destroy it");
    if (!S->from_rows) FAIL(c, LIG_E_STATE, "lig_shard_rows_diagnose_attached: not a rows shard (lig_shard_rows_begin)");
    if (!S->diag_ok) FAIL(c, LIG_E_STATE, "lig_shard_rows_diagnose_attached: no committed matrix (between lig_shard_rows_commit and the next lig_shard_rows_restart)");
    if (!S->linear) FAIL(c, LIG_E_STATE, "lig_shard_rows_diagnose_attached: no linear system is set (lig_shard_rows_set_linear)");
    const uint32_t struct_bytes = info->struct_bytes;
    std::memset(info, 0, sizeof *info);
    info->struct_bytes = struct_bytes;
    ShardDebugScope dbg(S, "diagnose_attached", nullptr);
    if (W == 1 && !S->exchange_even_alone) {       // one rank holds every row in commit order: lig_rows_diagnose_attached on its matrix, no collective
        TRY(lig_internal_rows_diagnose_attached(c, S->msgs, R, S->tri_dev, S->triple_ord.size(), S->linear, lin_out, lin_cap, quad_out, quad_cap, info));
        info->ms_total = ms_since(t_begin);
        return LIG_OK;
    }
    SHARD_DIAG_VIEW(v);
    TRY(lig_internal_shard_diagnose_attached(c, v, S->linear, lin_out, lin_cap, quad_out, quad_cap, info));
    info->ms_total = ms_since(t_begin);
    return LIG_OK;
}

// lig_rows_explain / lig_rows_read_slots on a rows shard (diagnose.hip): collective, every rank obtains the bytes of the one-GPU call on the
// whole trace.  Window, state checks and refusals as lig_shard_rows_diagnose: decided here, on the host, identically on every rank, before
// anything is launched and before any collective.
int lig_shard_rows_explain(lig_shard* S, const lig_linear_system* sys, const uint32_t* asked, uint64_t n_asked, lig_explain_constraint* con_out,
                           lig_explain_term* terms_out, uint64_t term_cap, lig_explain_info* info) {
    if (!S || !info || info->struct_bytes < sizeof(lig_explain_info)) return LIG_E_ARG;
    if ((n_asked && (!con_out || !asked)) || (term_cap && !terms_out)) return LIG_E_ARG;
    const auto t_begin = clk::now();
    SHARD_COMMON;
    (void)n;
    CHECK_CTX(c);
    if (S->poisoned) FAIL(c, LIG_E_STATE, "lig_shard_rows_explain: the shard is poisoned (work queued behind a failed collective never drained): destroy it");
    if (!S->from_rows) FAIL(c, LIG_E_STATE, "lig_shard_rows_explain: not a rows shard (lig_shard_rows_begin)");
    if (!S->diag_ok) FAIL(c, LIG_E_STATE, "lig_shard_rows_explain: no committed matrix (between lig_shard_rows_commit and the next lig_shard_rows_restart)");
    if (!sys) FAIL(c, LIG_E_ARG, "lig_shard_rows_explain: null linear system");
    if (lig_linear_check(sys, kinds_of(S->rows).data(), R, l) != LIG_OK) FAIL(c, LIG_E_ARG, "lig_shard_rows_explain: linear system rejected by lig_linear_check");
    if (!lig::explain_asked_ok(asked, n_asked, sys->n_constraints))
        FAIL(c, LIG_E_ARG, "lig_shard_rows_explain: the asked constraints must be strictly ascending and below n_constraints");
    const uint32_t struct_bytes = info->struct_bytes;
    std::memset(info, 0, sizeof *info);
    info->struct_bytes = struct_bytes;
    if (!n_asked) return LIG_OK;
    ShardDebugScope dbg(S, "explain", nullptr);
    if (W == 1 && !S->exchange_even_alone) {       // one rank holds every row in commit order: the one-GPU call, no collective
        TRY(lig_internal_rows_explain(c, S->msgs, sys, asked, n_asked, con_out, terms_out, term_cap, info));
        info->ms_total = ms_since(t_begin);
        return LIG_OK;
    }
    SHARD_DIAG_VIEW(v);
    TRY(lig_internal_shard_explain(c, v, sys, asked, n_asked, con_out, terms_out, term_cap, info));
    info->ms_total = ms_since(t_begin);
    return LIG_OK;
}
// lig_shard_rows_explain against the share of the system ATTACHED to the shard (lig_shard_rows_set_linear), with the values of
// lig_shard_rows_set_linear_values in force: no term list, no host pass over it (diagnose.hip).  Window, refusals and poisoning as above;
// one rank alone runs the same passes over its share (compactly numbered through need[] all the same) without a collective.
int lig_shard_rows_explain_attached(lig_shard* S, const uint32_t* asked, uint64_t n_asked, lig_explain_constraint* con_out, lig_explain_term* terms_out,
                                    uint64_t term_cap, lig_explain_info* info) {
    if (!S || !info || info->struct_bytes < sizeof(lig_explain_info)) return LIG_E_ARG;
    if ((n_asked && (!con_out || !asked)) || (term_cap && !terms_out)) return LIG_E_ARG;
    const auto t_begin = clk::now();
    SHARD_COMMON;
    (void)n;
    CHECK_CTX(c);
    if (S->poisoned) FAIL(c, LIG_E_STATE, "lig_shard_rows_explain_attached: the shard is poisoned (work queued behind a failed collective never drained): destroy it");
    if (!S->from_rows) FAIL(c, LIG_E_STATE, "lig_shard_rows_explain_attached: not a rows shard (lig_shard_rows_begin)");
    if (!S->diag_ok) FAIL(c, LIG_E_STATE, "lig_shard_rows_explain_attached: no committed matrix (between lig_shard_rows_commit and the next lig_shard_rows_restart)");
    if (!S->linear) FAIL(c, LIG_E_STATE, "lig_shard_rows_explain_attached: no linear system is set (lig_shard_rows_set_linear)");
    if (!lig::explain_asked_ok(asked, n_asked, lig_internal_linear_view(S->linear).n_constraints))
        FAIL(c, LIG_E_ARG, "lig_shard_rows_explain_attached: the asked constraints must be strictly ascending and below n_constraints");
    const uint32_t struct_bytes = info->struct_bytes;
    std::memset(info, 0, sizeof *info);
    info->struct_bytes = struct_bytes;
    if (!n_asked) return LIG_OK;
    ShardDebugScope dbg(S, "explain_attached", nullptr);
    SHARD_DIAG_VIEW(v);
    TRY(lig_internal_shard_explain_attached(c, v, S->linear, W == 1 && !S->exchange_even_alone, asked, n_asked, con_out, terms_out, term_cap, info));
    info->ms_total = ms_since(t_begin);
    return LIG_OK;
}
int lig_shard_rows_read_slots(lig_shard* S, const uint32_t* slots, uint64_t n_slots, uint8_t* values) {
    if (!S || (n_slots && (!slots || !values))) return LIG_E_ARG;
    SHARD_COMMON;
    (void)n;
    CHECK_CTX(c);
    if (S->poisoned) FAIL(c, LIG_E_STATE, "lig_shard_rows_read_slots: the shard is poisoned (work queued behind a failed collective never drained): destroy it");
    if (!S->from_rows) FAIL(c, LIG_E_STATE, "lig_shard_rows_read_slots: not a rows shard (lig_shard_rows_begin)");
    if (!S->diag_ok) FAIL(c, LIG_E_STATE, "lig_shard_rows_read_slots: no committed matrix (between lig_shard_rows_commit and the next lig_shard_rows_restart)");
    if (!lig::explain_slots_ok(slots, n_slots, R, l)) FAIL(c, LIG_E_ARG, "lig_shard_rows_read_slots: a slot is not below rows * l of the whole trace");
    if (!n_slots) return LIG_OK;
    ShardDebugScope dbg(S, "read_slots", nullptr);
    if (W == 1 && !S->exchange_even_alone) return lig_internal_rows_read_slots(c, S->msgs, R, slots, n_slots, values);
    SHARD_DIAG_VIEW(v);
    return lig_internal_shard_read_slots(c, v, slots, n_slots, values);
}

// lig_rows_explain_slots* / lig_rows_untouched_slots* on a rows shard (diagnose.hip): collective, every rank obtains the bytes of the one-GPU
// call on the whole trace.  Both read the slot-major index of the rank's share: the one attached to the shard (att), or a temporary one made
// from sys with lig_internal_linear_create_shard and destroyed before the call returns -- one code path; what is attached is then neither
// read nor modified.  Window, state checks and refusals as lig_shard_rows_explain_attached: decided here, on the host, identically on every
// rank, before anything is launched and before any collective (args_ok: the entry's own check of its lists against the rows of the whole
// trace).  One rank alone runs the same passes over its compactly numbered share without a collective.
using ShardSlotsRun = std::function<int(lig_ctx*, const lig_diag_shard&, const lig_linear*, bool, const uint8_t*)>;
static int shard_slots_call(const char* which, const char* debug_name, bool att, lig_shard* S, const lig_linear_system* sys,
                            const std::function<bool(uint64_t, uint32_t)>& args_ok, bool nothing_to_do, const ShardSlotsRun& run) {
    SHARD_COMMON;
    (void)n;
    CHECK_CTX(c);
    const std::string w(which);
    if (S->poisoned) FAIL(c, LIG_E_STATE, w + ": the shard is poisoned (work queued behind a failed collective never drained): destroy it");
    if (!S->from_rows) FAIL(c, LIG_E_STATE, w + ": not a rows shard (lig_shard_rows_begin)");
    if (!S->diag_ok) FAIL(c, LIG_E_STATE, w + ": no committed matrix (between lig_shard_rows_commit and the next lig_shard_rows_restart)");
    if (att && !S->linear) FAIL(c, LIG_E_STATE, w + ": no linear system is set (lig_shard_rows_set_linear)");
    if (!att && !sys) FAIL(c, LIG_E_ARG, w + ": null linear system");
    const std::vector<uint8_t> kinds = kinds_of(S->rows);
    if (!att && lig_linear_check(sys, kinds.data(), R, l) != LIG_OK) FAIL(c, LIG_E_ARG, w + ": linear system rejected by lig_linear_check");
    if (!args_ok(R, l)) FAIL(c, LIG_E_ARG, w + ": the asked slots must be strictly ascending and below rows * l of the whole trace");
    if (nothing_to_do) return LIG_OK;
    ShardDebugScope dbg(S, debug_name, nullptr);
    SHARD_DIAG_VIEW(v);
    const bool alone = W == 1 && !S->exchange_even_alone;
    if (att) return run(c, v, S->linear, alone, kinds.data());
    lig_linear* tmp = nullptr;
    TRY(lig_internal_linear_create_shard(c, sys, kinds.data(), S->R, S->grow, S->rank, S->world, &tmp));
    const int rc = run(c, v, tmp, alone, kinds.data());
    if (rc != LIG_OK && S->poisoned) return rc;      // kernels that never drained may still read the temporary share: it outlives the call
    const std::string why = c->err;
    lig_internal_linear_destroy(tmp);
    c->err = why;
    return rc;
}
static int shard_explain_slots(const char* which, bool att, lig_shard* S, const lig_linear_system* sys, const uint32_t* slots, uint64_t n_asked, lig_slot_record* slot_out,
                               lig_slot_term* terms_out, uint64_t term_cap, lig_slot_info* info) {
    if (!S || !info || info->struct_bytes < sizeof(lig_slot_info)) return LIG_E_ARG;
    if ((n_asked && (!slot_out || !slots)) || (term_cap && !terms_out)) return LIG_E_ARG;
    const auto t_begin = clk::now();
    const uint32_t struct_bytes = info->struct_bytes;
    const auto args_ok = [&](uint64_t rows, uint32_t l) -> bool {
        if (!lig::explain_slots_ok(slots, n_asked, rows, l)) return false;
        for (uint64_t i = 1; i < n_asked; i++) if (slots[i] <= slots[i - 1]) return false;
        return true;
    };
    TRY(shard_slots_call(which, att ? "explain_slots_attached" : "explain_slots", att, S, sys, args_ok, !n_asked,
                         [&](lig_ctx* c, const lig_diag_shard& v, const lig_linear* L, bool alone, const uint8_t* kinds) -> int {
        std::memset(info, 0, sizeof *info);
        info->struct_bytes = struct_bytes;
        return lig_internal_shard_explain_slots(c, v, L, alone, kinds, slots, n_asked, slot_out, terms_out, term_cap, info);
    }));
    if (!n_asked) { std::memset(info, 0, sizeof *info); info->struct_bytes = struct_bytes; }
    info->ms_total = ms_since(t_begin);
    return LIG_OK;
}
static int shard_untouched_slots(const char* which, bool att, lig_shard* S, const lig_linear_system* sys, int nonzero_only, lig_slot_value* out, uint64_t cap,
                                 lig_untouched_info* info) {
    if (!S || !info || info->struct_bytes < sizeof(lig_untouched_info)) return LIG_E_ARG;
    if (cap && !out) return LIG_E_ARG;
    const auto t_begin = clk::now();
    const uint32_t struct_bytes = info->struct_bytes;
    TRY(shard_slots_call(which, att ? "untouched_slots_attached" : "untouched_slots", att, S, sys, [](uint64_t, uint32_t) -> bool { return true; }, false,
                         [&](lig_ctx* c, const lig_diag_shard& v, const lig_linear* L, bool alone, const uint8_t* kinds) -> int {
        std::memset(info, 0, sizeof *info);
        info->struct_bytes = struct_bytes;
        return lig_internal_shard_untouched_slots(c, v, L, alone, kinds, nonzero_only, out, cap, info);
    }));
    info->ms_total = ms_since(t_begin);
    return LIG_OK;
}
int lig_shard_rows_explain_slots_attached(lig_shard* S, const uint32_t* slots, uint64_t n_asked, lig_slot_record* slot_out, lig_slot_term* terms_out, uint64_t term_cap,
                                          lig_slot_info* info) {
    return shard_explain_slots("lig_shard_rows_explain_slots_attached", true, S, nullptr, slots, n_asked, slot_out, terms_out, term_cap, info);
}
int lig_shard_rows_explain_slots(lig_shard* S, const lig_linear_system* sys, const uint32_t* slots, uint64_t n_asked, lig_slot_record* slot_out, lig_slot_term* terms_out,
                                 uint64_t term_cap, lig_slot_info* info) {
    return shard_explain_slots("lig_shard_rows_explain_slots", false, S, sys, slots, n_asked, slot_out, terms_out, term_cap, info);
}
int lig_shard_rows_untouched_slots_attached(lig_shard* S, int nonzero_only, lig_slot_value* out, uint64_t cap, lig_untouched_info* info) {
    return shard_untouched_slots("lig_shard_rows_untouched_slots_attached", true, S, nullptr, nonzero_only, out, cap, info);
}
int lig_shard_rows_untouched_slots(lig_shard* S, const lig_linear_system* sys, int nonzero_only, lig_slot_value* out, uint64_t cap, lig_untouched_info* info) {
    return shard_untouched_slots("lig_shard_rows_untouched_slots", false, S, sys, nonzero_only, out, cap, info);
}

// The sparse linear system of the WHOLE trace on a rows shard: every rank passes the same system (a collective contract, like the kinds) and
// keeps its share -- the terms of the rows it was dealt, the constraints those need, its slice of the right-hand sides (linear.hip).
int lig_shard_rows_set_linear(lig_shard* S, const lig_linear_system* sys) {
    if (!S) return LIG_E_ARG;
    lig_ctx* c = S->c;
    CHECK_CTX(c);
    if (S->poisoned) FAIL(c, LIG_E_STATE, "lig_shard_rows_set_linear: the shard is poisoned (work queued behind a failed collective never drained): destroy it");
    if (!S->from_rows) FAIL(c, LIG_E_STATE, "lig_shard_rows_set_linear: not a rows shard (lig_shard_rows_begin)");
    if (!sys) {
        lig_internal_linear_destroy(S->linear);
        S->linear = nullptr;
        return LIG_OK;
    }
    if (S->dense_rands) FAIL(c, LIG_E_ARG, "lig_shard_rows_set_linear: the job has dense_rands_per_row");
    lig_linear* L = nullptr;
    TRY(lig_internal_linear_create_shard(c, sys, kinds_of(S->rows).data(), S->R, S->grow, S->rank, S->world, &L));      // lig_linear_check first: nothing is launched for a system it rejects
    if (!S->rands_lin) {
        const hipError_t e = hipMalloc((void**)&S->rands_lin, (S->Rl ? S->Rl : 1) * (size_t)c->k * 32);
        if (e != hipSuccess) { (void)hipGetLastError(); lig_internal_linear_destroy(L); FAIL(c, LIG_E_NOMEM, std::string("lig_shard_rows_set_linear: randomness matrix: ") + hipGetErrorString(e)); }
    }
    lig_internal_linear_destroy(S->linear);
    S->linear = L;
    return LIG_OK;
}
// The values of the coefficient table of the system set above, for the proofs that follow: what lig_rows_set_linear_values is on one GPU.
// They belong to the rank's attachment; host check, pinned copy, upload and k_lin_coefs_mont on the side stream -- the stream
// shard_stage23 forms on, so a form queued later reads the converted table.  No collective: every rank passes the same table (contract).
int lig_shard_rows_set_linear_values(lig_shard* S, const uint8_t* coefs, uint64_t n_coefs) {
    if (!S) return LIG_E_ARG;
    lig_ctx* c = S->c;
    CHECK_CTX(c);
    if (S->poisoned) FAIL(c, LIG_E_STATE, "lig_shard_rows_set_linear_values: the shard is poisoned (work queued behind a failed collective never drained): destroy it");
    if (!S->from_rows) FAIL(c, LIG_E_STATE, "lig_shard_rows_set_linear_values: not a rows shard (lig_shard_rows_begin)");
    if (!S->linear) FAIL(c, LIG_E_STATE, "lig_shard_rows_set_linear_values: no linear system is set (lig_shard_rows_set_linear)");
    return lig_internal_linear_set_values(c, S->linear, coefs, n_coefs, c->stream2);
}
// the rank that was dealt every row: chunk g of the deal belongs to rank g mod W
static std::vector<uint32_t> shard_owner(const std::vector<size_t>& gb, uint32_t W, size_t R) {
    std::vector<uint32_t> owner(R, 0);
    for (size_t g = 0; g + 1 < gb.size(); g++)
        for (size_t r = gb[g]; r < gb[g + 1]; r++) owner[r] = (uint32_t)(g % W);
    return owner;
}
// Derived slots on a rows shard (derive.hip): the list of the WHOLE trace; every rank passes the same one (a contract, like the system of
// lig_shard_rows_set_linear -- the exchange schedule is computed from it).  No collective here; a refused list changes nothing.  (No derive
// kernel is in flight: lig_shard_rows_commit returns only after stage 1 has drained.)
int lig_shard_rows_set_derived(lig_shard* S, const lig_linear_system* sys, const lig_derived_slot* d, uint64_t n, lig_derived_shard_info* info) {
    if (!S) return LIG_E_ARG;
    lig_ctx* c = S->c;
    CHECK_CTX(c);
    if (S->poisoned) FAIL(c, LIG_E_STATE, "lig_shard_rows_set_derived: the shard is poisoned (work queued behind a failed collective never drained): destroy it");
    if (!S->from_rows) FAIL(c, LIG_E_STATE, "lig_shard_rows_set_derived: not a rows shard (lig_shard_rows_begin)");
    if (info && info->struct_bytes < sizeof(lig_derived_shard_info)) FAIL(c, LIG_E_ARG, "lig_shard_rows_set_derived: lig_derived_shard_info.struct_bytes too small");
    if (!d || !n) {
        lig_internal_derive_shard_destroy(S->derive);
        S->derive = nullptr;
        if (info) { const uint32_t sb = info->struct_bytes; std::memset(info, 0, sizeof *info); info->struct_bytes = sb; }
        return LIG_OK;
    }
    lig_derive_shard* D = nullptr;
    uint64_t send_elems = 0, import_elems = 0;
    lig_derived_shard_info mine;
    mine.struct_bytes = sizeof mine;
    TRY(lig_internal_derive_shard_create(c, sys, kinds_of(S->rows).data(), S->R, S->elem_bytes_all.empty() ? nullptr : S->elem_bytes_all.data(), d, n,
                                         shard_owner(S->gb, S->world, S->R), S->rank, S->world, &D, &send_elems, &import_elems, &mine));
    auto grow = [&](fr** buf, uint64_t* cap, uint64_t elems) -> int {
        if (elems <= *cap) return LIG_OK;
        fr* fresh = nullptr;
        const hipError_t e = hipMalloc((void**)&fresh, elems * 32);
        if (e != hipSuccess) { (void)hipGetLastError(); FAIL(c, LIG_E_NOMEM, std::string("lig_shard_rows_set_derived: exchange buffers: ") + hipGetErrorString(e)); }
        if (*buf) S->derive_retired.push_back(*buf);
        *buf = fresh; *cap = elems;
        return LIG_OK;
    };
    int rc = grow(&S->derive_send, &S->derive_send_cap, send_elems);
    if (rc == LIG_OK) rc = grow(&S->derive_import, &S->derive_import_cap, import_elems);
    if (rc != LIG_OK) { const std::string why = c->err; lig_internal_derive_shard_destroy(D); c->err = why; return rc; }
    lig_internal_derive_shard_destroy(S->derive);
    S->derive = D;
    if (info) { const uint32_t sb = info->struct_bytes; std::memset(info, 0, sizeof *info); std::memcpy(info, &mine, sizeof mine); info->struct_bytes = sb; }
    return LIG_OK;
}
// host only: the numbers of lig_shard_rows_set_derived from the deal alone
int lig_derived_shard_count(const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, uint32_t l, const uint8_t* elem_bytes, const lig_derived_slot* d,
                            uint64_t n, uint32_t rank, uint32_t world, lig_derived_shard_info* info) {
    if (!world || rank >= world || !info || info->struct_bytes < sizeof(lig_derived_shard_info)) return LIG_E_ARG;
    if (lig_linear_check(sys, kinds, rows, l) != LIG_OK) return LIG_E_ARG;      // (kinds are read below only for a system it accepts)
    std::vector<RowDesc> rd(rows);
    for (uint64_t r = 0; r < rows; r++) rd[r] = RowDesc{(uint8_t)(kinds[r] & 0x7f), 0};
    size_t rounds = 0;
    std::vector<size_t> gb;
    shard_chunks(rd, world, rounds, gb);
    return lig_internal_derive_shard_count(sys, kinds, rows, l, elem_bytes, d, n, shard_owner(gb, world, rows), rank, world, info);
}
int lig_shard_rows_linear_stats(const lig_shard* S, uint64_t* local_terms, uint64_t* sampled_constraints) {
    if (!S || !local_terms || !sampled_constraints) return LIG_E_ARG;
    if (!S->linear) return LIG_E_STATE;
    lig_internal_linear_stats(S->linear, local_terms, sampled_constraints);
    return LIG_OK;
}
// host only: the same two numbers from the deal alone
int lig_linear_shard_count(const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, uint32_t l, uint32_t rank, uint32_t world, uint64_t* local_terms,
                           uint64_t* needed_constraints) {
    if (!world || rank >= world || !local_terms || !needed_constraints) return LIG_E_ARG;
    if (lig_linear_check(sys, kinds, rows, l) != LIG_OK) return LIG_E_ARG;
    std::vector<RowDesc> rd(rows);
    for (uint64_t r = 0; r < rows; r++) rd[r] = RowDesc{(uint8_t)(kinds[r] & 0x7f), 0};
    size_t rounds = 0;
    std::vector<size_t> gb, grow;
    shard_chunks(rd, world, rounds, gb);
    for (size_t cidx = 0; cidx < rounds; cidx++)
        for (size_t r = gb[cidx * world + rank]; r < gb[cidx * world + rank + 1]; r++) grow.push_back(r);
    lig_internal_linear_shard_count(sys, l, grow, rows, rank, world, local_terms, needed_constraints);
    return LIG_OK;
}

}  // extern "C"
