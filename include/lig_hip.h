/*
 * lig_hip.h -- C ABI of the MI355X-native Ligero prover backend (liblig_hip.so).
 *
 * This is the drop-in boundary for the reference's GPU executor `ligero::webgpu_context`
 * (include/wgpu.hpp:50-183, include/ligetron/webgpu/device_context.hpp:29-98).  In the reference the
 * executor is a C++ template parameter (`using executor_t = webgpu_context`, src/webgpu_prover.cpp:54)
 * passed into the stage contexts (include/zkp/nonbatch_context.hpp:68-80); `include/lig_hip_context.hpp`
 * wraps this ABI in a class with the same member names so those drivers compile against it.
 *
 * Conventions
 *   - plain C: opaque context, raw DEVICE pointers (hipMalloc'ed or any HIP-visible allocation, e.g. a
 *     torch tensor's data_ptr()), sizes in elements unless a name says bytes; no C++/torch types.
 *   - a field element is 32 bytes: 8 little-endian u32 limbs, canonical in [0,p) (BN254 Fr), the
 *     reference's device/host/proof format (include/ligetron/webgpu/device_bignum.hpp:76-86).
 *   - every op is asynchronous and ordered on the context's single HIP stream (the reference's single
 *     in-order WebGPU queue, src/webgpu/device_context.cpp:344-354); lig_sync() blocks.
 *   - functions return 0 on success, a negative LIG_E_* code otherwise; lig_last_error() gives text.
 *     (The reference has no error returns: device errors abort, device_context.cpp:121-127.)
 *   - thread-compatible, not thread-safe (the reference is single-threaded).
 */
#ifndef LIG_HIP_H
#define LIG_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lig_ctx lig_ctx;

enum { LIG_OK = 0, LIG_E_ARG = -1, LIG_E_HIP = -2, LIG_E_STATE = -3, LIG_E_NOMEM = -4 };
enum { LIG_ELEM_BYTES = 32, LIG_DIGEST_BYTES = 32 };

/* ---- lifecycle: webgpu_init + ntt_init (include/wgpu.hpp:71-82; src/webgpu/engine.cpp:196-260).
 * p, mu and the three roots are derived from the fixed BN254 constants (the reference's shader hard-codes
 * them too, shader/bn254fr.wgsl.in:19-45); k must be a power of two >= 512 (engine.cpp:849-850), n = 4k. */
int  lig_ctx_create(lig_ctx **out, int device, uint32_t l, uint32_t k, uint32_t n);
void lig_ctx_destroy(lig_ctx *ctx);                       /* syncs, then frees (wgpu.hpp dtor) */
int  lig_sync(lig_ctx *ctx);                              /* device_synchronize() */
const char *lig_last_error(const lig_ctx *ctx);
const char *lig_version(void);
uint32_t lig_message_size(const lig_ctx *ctx);            /* l  (wgpu.hpp:153) */
uint32_t lig_padding_size(const lig_ctx *ctx);            /* k  (wgpu.hpp:154) */
uint32_t lig_encoding_size(const lig_ctx *ctx);           /* n  (wgpu.hpp:155) */
void *lig_stream(lig_ctx *ctx);                           /* hipStream_t, for callers that enqueue their own work */
/* which physical device an ordinal is ("0000:c1:00.0") and whether it can map a peer's memory: what a multi-GPU launcher
 * records before it builds a communicator (bench.py's preflight).  No context needed. */
int lig_device_pci_bus_id(int device, char *out, size_t cap);
int lig_device_peer_access(int device, int peer, int *can);

/* ---- buffers: make_device_buffer (zero-initialised like WebGPU), write_buffer, write_buffer_clear,
 * clear_buffer, copy_buffer_to_buffer, copy_to_host (device_context.hpp:79-98, device_context.cpp:364-449) */
int lig_malloc(lig_ctx *ctx, size_t bytes, void **dptr);
int lig_free(lig_ctx *ctx, void *dptr);
int lig_write(lig_ctx *ctx, void *dst, const void *host_src, size_t bytes);
int lig_write_clear(lig_ctx *ctx, void *dst, size_t dst_bytes, const void *host_src, size_t bytes);
int lig_clear(lig_ctx *ctx, void *dst, size_t bytes);
int lig_copy(lig_ctx *ctx, void *dst, const void *src, size_t bytes);
int lig_read(lig_ctx *ctx, void *host_dst, const void *src, size_t bytes);   /* blocking */
/* page-locked host memory for rows a driver hands to lig_rows_* (uploads from it are true DMA transfers; from pageable memory
 * the runtime stages every copy).  Replaces the std::vector `limbs_` staging of include/zkp/nonbatch_context.hpp:447. */
int lig_host_alloc(lig_ctx *ctx, size_t bytes, void **host_ptr);
int lig_host_free(lig_ctx *ctx, void *host_ptr);
/* Asynchronous form of lig_write for page-locked sources (lig_host_alloc): enqueued on the context stream and NOT waited for.
 * The source must stay untouched until a fence recorded after the call has been waited for.  Fences: lig_fence_record
 * (re)records *fence at the current end of the context stream (allocating it when *fence == NULL), lig_fence_wait blocks the
 * host until that point has been reached.  Used by hip_context's deferred row mode (include/lig_hip_context.hpp): the
 * reference's per-row wgpuQueueWriteBuffer (src/webgpu/device_context.cpp:364-380) batched into one transfer per <= 512 rows
 * that runs under the caller's next rows. */
int  lig_write_async(lig_ctx *ctx, void *dst, const void *pinned_src, size_t bytes);
int  lig_fence_record(lig_ctx *ctx, void **fence);
int  lig_fence_wait(lig_ctx *ctx, void *fence);
void lig_fence_destroy(lig_ctx *ctx, void *fence);

/* ---- Reed-Solomon transforms on ONE n-element buffer, in place
 * (encode_ntt_device / decode_ntt_device / ntt_{forward,inverse}_{k,2k,n}: engine.cpp:755-968) */
enum { LIG_SIZE_K = 0, LIG_SIZE_2K = 1, LIG_SIZE_N = 2 };
int lig_encode(lig_ctx *ctx, void *buf);                  /* buf[0..k) message, buf[k..n) must be 0 */
int lig_encode_2k(lig_ctx *ctx, void *buf);               /* ntt_inverse_2k + ntt_forward_n (mask rows) */
int lig_decode(lig_ctx *ctx, void *buf);                  /* INTT_n, fold k..2k onto 0..k, NTT_k */
int lig_ntt(lig_ctx *ctx, void *buf, int which, int inverse);

/* ---- eltwise (shader/kernels.wgsl.in:326-538; wgpu.hpp:98-139).  x, y, out may alias; `scalar` is a host
 * pointer to one 32-byte element (the reference passes an mpz through a uniform buffer). */
enum {
    LIG_OP_ADD = 0,        /* out = x + y          EltwiseAddMod            */
    LIG_OP_SUB,            /* out = x - y          EltwiseSubMod            */
    LIG_OP_ADD_ASSIGN,     /* out += x             EltwiseAddAssignMod      */
    LIG_OP_ADD_CONST,      /* out = x + c          EltwiseAddMod(scalar)    */
    LIG_OP_SUB_CONST,      /* out = x - c          EltwiseSubConstMod       */
    LIG_OP_CONST_SUB,      /* out = c - x          EltwiseConstSubMod       */
    LIG_OP_MUL,            /* out = x * y          EltwiseMultMod           */
    LIG_OP_MUL_CONST,      /* out = x * c          EltwiseMultMod(scalar)   */
    LIG_OP_MONTMUL_CONST,  /* out = x * c / R      EltwiseMontMultMod       */
    LIG_OP_FMA,            /* out += x * y         EltwiseFMAMod            */
    LIG_OP_FMA_CONST,      /* out += x * c         EltwiseFMAMod(scalar)    */
    LIG_OP_DIV,            /* out = x / y (y=0->0) EltwiseDivMod            */
    LIG_OP_BIT_DECOMPOSE   /* out = bit `bit` of x EltwiseBitDecompose      */
};
int lig_eltwise(lig_ctx *ctx, int op, const void *x, const void *y, void *out, size_t count,
                const uint8_t *scalar32, uint32_t bit);
/* EltwisePowMod / EltwisePowAddMod (src/webgpu/powmod_context.cpp:178-268): out (=|+=) coeff * base^exp */
int lig_powmod(lig_ctx *ctx, const uint8_t *base32, const void *exp_u32, const void *coeff, void *out,
               size_t count, int add);

/* ---- column SHA-256 (shader/sha256.wgsl; engine.cpp:1514-1686).  `state` is a device buffer of
 * lig_sha_state_bytes(n_inst) bytes owned by the caller (the reference's sha256_context, wgpu.hpp:63-68). */
size_t lig_sha_state_bytes(size_t n_inst);
int lig_sha_init(lig_ctx *ctx, void *state, size_t n_inst);                   /* sha256_digest_init  */
int lig_sha_update(lig_ctx *ctx, void *state, const void *row);               /* sha256_digest_update: n_inst elems */
int lig_sha_final(lig_ctx *ctx, void *state, void *digests);                  /* sha256_digest_final: n_inst x 32 B */

/* ---- sampling (engine.cpp:1689-1809; kernels.wgsl.in:541-549) */
int lig_sample_init(lig_ctx *ctx, const uint32_t *host_idx, size_t count);    /* sampling_init */
int lig_sample_gather(lig_ctx *ctx, const void *from, void *to, size_t slot); /* to[slot*count + i] = from[idx[i]] */

/* ==== batched entry points (no reference counterpart: the reference pushes one row per call; these are what
 * a row-batching driver and bench.py call so the GPU sees hundreds of rows per launch) ==== */
/* msgs: rows x k elements (row-major, contiguous); codewords: rows x n elements */
int lig_encode_rows(lig_ctx *ctx, const void *msgs, void *codewords, size_t rows);
/* absorb `rows` codeword rows (rows x n_inst elements, row-major) in order */
int lig_sha_update_rows(lig_ctx *ctx, void *state, const void *codewords, size_t rows);
/* Merkle tree over n_leaves digests (merkle_tree::initialize_from_digest/build_tree, merkle_tree.hpp:344-375):
 * nodes = (2*bit_ceil(n_leaves)-1) x 32 B device buffer in heap order, root = node 0 */
size_t lig_merkle_nodes(size_t n_leaves);
int lig_merkle_build(lig_ctx *ctx, const void *leaves, size_t n_leaves, void *nodes);
/* stage-2 accumulators over a batch (check_code / check_linear / check_quadratic,
 * nonbatch_context.hpp:756-780): for r < rows
 *    code[j]  += rc[r] * U[r][j]                      (rc: rows host scalars, 32 B each)
 *    lin[j]   += U[r][j] * Rn[r][j]                   (Rn may be NULL: skipped)
 *    quad[j]  += rq[t] * (U[x_t][j]*U[y_t][j] - U[z_t][j])   for each triple t (triples: 3 row indices each)
 */
int lig_rlc_rows(lig_ctx *ctx, const void *U, const void *Rn, size_t rows,
                 const uint8_t *rc_host, void *code, void *lin,
                 const uint32_t *triples_host, const uint8_t *rq_host, size_t n_triples, void *quad);
/* out[r*count + i] = codewords[r][idx[i]]  for r < rows (stage 3, nonbatch_context.hpp:924-942) */
int lig_gather_rows(lig_ctx *ctx, const void *codewords, size_t rows, void *out);
/* AES-256-CTR field sampler on the GPU (include/util/csprng.hpp:54-107 + finite_field_gmp.hpp:66-78):
 * out[i] = element number first_elem + i of the stream keyed by key32 (IV = 0) */
int lig_rng_fill(lig_ctx *ctx, const uint8_t *key32, uint64_t first_elem, void *out, size_t count);

/* ==== batched three-stage prover over a resident witness matrix (src/webgpu_prover.cpp:226-494 restructured:
 * rows are encoded once, codewords stay in HBM for stages 2 and 3).  The guest interpreter is replaced by the
 * synthetic constraint stream of BASELINE.md: n_linear witness slots + n_quad slots of x*y=z, witnesses from the
 * AES-256-CTR field stream keyed by witness_key, one dense linear-test coefficient per witness.  The envelope
 * bytes equal the reference's LigeroProofEnvelope (proto/ligero_proof.proto) for the same rows and seeds. ==== */
typedef struct lig_trace lig_trace;
/* Optional batch ("vbn254fr") program executed before the synthetic stream: the guest-visible batch operations of
 * include/host_modules/vbn254fr.hpp:138-565 as a list.  Variables are slots 0..511 of k elements (l data + k-l padding);
 * every operation works on all k elements (the reference binds k-element windows, :64-69) and raises the constraint hook
 * the reference raises (include/zkp/nonbatch_context.hpp:497-553), whose rows are committed in program order:
 *   SET            x <- data[data_off .. +32*len), rest 0            on_batch_init(x): k-l pads drawn, 1 row
 *   SET_SCALAR     x[0..l) <- the element at data_off                on_batch_init(x)
 *   COPY           out <- x                                          on_batch_equal(out, x): 2 rows
 *   ADD, SUB       out <- x op y                                     no row
 *   MUL            out <- x*y                                        on_batch_quadratic(x, y, x*y): 3 rows
 *   DIV            out <- x/y  (x/0 = 0)                             on_batch_quadratic(x/y, y, x): 3 rows
 *   ADD_CONST, SUB_CONST, CONST_SUB (c - x), MUL_CONST, MONTMUL_CONST with the element at data_off: no row
 *   ASSERT_EQUAL                                                     on_batch_equal(x, y)
 *   BIT_DECOMPOSE  slot table of len (= 254) u32 at data_off; out_i <- bit i of x; on_batch_bit(out_i): 1 row each
 *   FREE           x <- 0
 * Stage 2 treats the rows as the reference does: check_code for init / bit / quadratic rows (not for equal rows),
 * check_quadratic for bit (x*x - x) and quadratic triples, quad += r*(x - y) for equal rows; no linear-test randomness.
 * SET / SET_SCALAR with `reserved` bit 0 set: the variable was written by the write_limbs family (vbn254fr_set_str / _set_bytes
 * and their _scalar forms, vbn254fr.hpp:200,222,251,271: write_buffer, nothing cleared): slots beyond the written ones keep
 * their content.  Bit 0 clear: the write_buffer_clear family (vbn254fr_set_ui / _set_ui_scalar, :154,:169).
 *
 * Two slicing semantics.  DECLARED (default): buffer_view::slice_bytes(from, n_bytes) as include/ligetron/webgpu/
 * buffer_view.hpp:52 declares it -- the pad of on_batch_init goes to the variable's own slots [l, k), write_buffer_clear zeroes
 * the rest of the variable.  UPSTREAM (after a LIG_BOP_UPSTREAM_COMPAT op): the definition src/webgpu/buffer_view.cpp:91-95
 * swaps the two parameters, so x.slice(B) of a variable x at slab byte offset X is the view {offset = B, size = X + size(x) - B}
 * of the SLAB: (1) on_batch_init (nonbatch_context.hpp:502-505) writes its 192 pad elements at slab byte l*32 = the pad slots
 * of VARIABLE 0, whatever x is; (2) write_buffer_clear(x, data, len) (device_context.hpp:95-98) clears slab bytes
 * [len*32, X + k*32) after the write -- for a variable other than 0 that is variable 0 from slot `len` on, every variable in
 * between and x itself, the data just written included.  An unmodified v1.5.0 build proves THAT; a proof of a vbn254fr program
 * matches / cross-verifies with it only in this mode. */
enum {
    LIG_BOP_SET = 0, LIG_BOP_SET_SCALAR, LIG_BOP_COPY, LIG_BOP_ADD, LIG_BOP_SUB, LIG_BOP_MUL, LIG_BOP_DIV, LIG_BOP_ADD_CONST,
    LIG_BOP_SUB_CONST, LIG_BOP_CONST_SUB, LIG_BOP_MUL_CONST, LIG_BOP_MONTMUL_CONST, LIG_BOP_ASSERT_EQUAL,
    LIG_BOP_BIT_DECOMPOSE, LIG_BOP_FREE,
    LIG_BOP_UPSTREAM_COMPAT,         /* no operands, no row: from here on slices behave as upstream DEFINES them (see above) */
    LIG_BOP_COUNT
};
enum { LIG_BOP_F_WRITE_LIMBS = 1 };  /* lig_batch_op.reserved, SET / SET_SCALAR */
typedef struct { uint32_t op, out, x, y, len, reserved; uint64_t data_off; } lig_batch_op;
typedef struct {
    uint64_t n_linear, n_quad;
    uint8_t  encoding_seed[32];      /* src/webgpu_prover.cpp:239-245 (there: std::random_device) */
    uint8_t  witness_key[32];
    uint8_t  program_hash[32];
    int64_t  generated_at;           /* metadata timestamp seconds (there: wall clock) */
    char     version[16];            /* "1.5.0" */
    const lig_batch_op *batch_ops; uint64_t n_batch_ops;      /* NULL / 0: no batch rows; read by prepare and verify only */
    const uint8_t *batch_data;     uint64_t batch_data_bytes;
    /* public arguments of the instance after arg0 = "Ligero\0" (src/webgpu_prover.cpp:110-168): n_public_args byte strings
     * back to back in the form the reference holds them in input_args (lig_public_arg_bytes converts the JSON forms);
     * NULL / 0: none.  They enter the proof through instance_hash -> stage1_seed.  Copied by prepare. */
    const uint8_t *public_args; const uint64_t *public_arg_lens; uint64_t n_public_args;
} lig_synth_job;
typedef struct {
    uint8_t  root[32], stage1_seed[32], stage2_seed[32], const_sum[32];
    uint64_t rows;                   /* committed rows including the 3 mask rows */
    int32_t  valid_code, valid_linear, valid_quad;   /* prover self-check, webgpu_prover.cpp:465-469 */
    int32_t  reserved;
    double   ms_stage1, ms_stage2, ms_stage3, ms_total;
} lig_proof_info;
/* untimed: plans the rows, allocates the resident buffers, generates the witness matrix on the GPU */
int  lig_synth_prepare(lig_ctx *ctx, const lig_synth_job *job, lig_trace **out);
/* the hot path: stage 1 (pads, masks, encode, column hash, Merkle), stage 2 (randomness rows, accumulators,
 * seeds, sampling, self-check), stage 3 (column gather, envelope).  *proof points into pinned host memory owned
 * by the trace: valid until the next lig_synth_prove on it or lig_trace_destroy. */
int  lig_synth_prove(lig_trace *trace, const uint8_t **proof, size_t *proof_len, lig_proof_info *info);
uint64_t lig_trace_rows(const lig_trace *trace);
void lig_trace_destroy(lig_trace *trace);

/* ==== verifier for the same synthetic stream (src/webgpu_verifier.cpp:263-452, nonbatch_verifier_context): returns
 * LIG_OK with out->accept = 1 iff the reference's seven predicates hold; a malformed envelope gives accept = 0
 * (parsed = 0), not an error.
 * The constant of the linear test is PUBLIC data upstream: the verifier re-runs the constraint stream and accumulates
 * linear_sums itself (src/webgpu_verifier.cpp:318).  The synthetic stream's public statement is "the committed witness is
 * the AES-256-CTR field stream of job->witness_key" (one linear constraint w_i = b_i per slot), so the verifier derives
 * the constant -sum_i rho_i b_i from the job alone: it regenerates b from witness_key and the coefficients rho from the
 * stage-1 seed.  const_sum == NULL selects that (the sound mode).  A non-NULL const_sum is used as given instead: the
 * hook for a caller whose own constraint generator produced the rows (lig_rows_*) and therefore the constant. ==== */
typedef struct {
    int32_t parsed, indices_match;
    int32_t valid_merkle, valid_code, valid_linear, valid_quad, code_equal, linear_equal, quad_equal;   /* webgpu_verifier.cpp:412-442 */
    int32_t accept;
    int32_t reserved;
    double  ms_total;                /* wall time of the call */
} lig_verify_info;
int lig_synth_verify(lig_ctx *ctx, const lig_synth_job *job, const uint8_t *const_sum /* NULL: derived */, const uint8_t *proof, size_t proof_len,
                     lig_verify_info *out);
/* the verifiers keep their device workspace on the context between calls (~2.5 GB after a 2^24-constraint verification: allocating it
 * per call costs milliseconds); this gives it back (it is also freed by lig_ctx_destroy) */
int lig_verify_release(lig_ctx *ctx);

/* ==== transcript helpers (host only, no GPU work): what a driver needs to stay byte-compatible with the reference ==== */
enum { LIG_ARG_I64 = 0, LIG_ARG_STR = 1, LIG_ARG_HEX = 2 };
/* one JSON "args" entry -> the bytes the reference appends to input_args (src/webgpu_prover.cpp:116-146): i64 (decimal
 * text) = 8 little-endian bytes, str = the characters plus the terminating NUL, hex (optional 0x, odd length gets a leading
 * 0) = the decoded bytes.  Returns LIG_E_ARG for malformed text or a too small buffer (*len = needed size). */
int lig_public_arg_bytes(int kind, const char *text, uint8_t *out, size_t cap, size_t *len);
/* instance_hash over arg0 = "Ligero\0" followed by the given public arguments (src/webgpu_prover.cpp:162-168) */
int lig_instance_hash(const uint8_t *args, const uint64_t *lens, size_t n_args, uint8_t out[32]);
/* hash_random_engine(seed) + portable_sample + sort (src/webgpu_prover.cpp:343-351): the t opened columns */
int lig_sample_columns(const uint8_t seed[32], uint32_t n, uint32_t t, uint32_t *out_sorted);

/* ==== the same three-stage prover over rows SUPPLIED BY THE CALLER: the entry a row-batching driver of the reference's
 * constraint generator uses.  It replaces the per-row callbacks of
 * include/zkp/nonbatch_context.hpp:445-471 (stage 1), :654-780 (stage 2) and :924-970 (stage 3); the rows are what
 * witness_manager hands to those callbacks (include/zkp/backend/witness_manager.hpp:200-269), in commit order.
 *   lig_rows_begin   takes the job: row kinds + the rows x k message matrix (host or device memory).  A host matrix is
 *                    uploaded asynchronously on a copy stream, chunk by chunk, and each chunk is encoded as soon as it has
 *                    arrived (pinned host memory makes the copy truly asynchronous; the memory must stay valid until
 *                    lig_rows_commit returns).
 *   lig_rows_commit  stage 1: pads of the rows flagged LIG_ROW_DRAW_PAD from the encoding stream (pad_encoding_random, in
 *                    commit order), the three mask rows, encode, column hash, Merkle root, stage-1 seed.  The caller now
 *                    derives its linear-test randomness from stage1_seed (the reference re-runs the guest for that).
 *   lig_rows_prove   stage 2 + 3 with the caller's randomness rows (rows x k; the row of a batch-kind row must be zero) and
 *                    the public constant of the linear test (linear_sums, src/webgpu_prover.cpp:307).
 * Encoding-stream positions follow the reference whoever draws: every LINEAR / QX / QY / QZ / INIT row owns the next k-l
 * elements of the stream keyed by encoding_seed (witness_manager pads each of them when it is formed), the three mask rows
 * take what follows; a row flagged LIG_ROW_DRAW_PAD gets exactly its own k-l elements, an unflagged one must carry them.
 * Row kinds: LINEAR rows stand alone; QX,QY,QZ / BQX,BQY,BQZ are consecutive triples (z = x*y); EQX,EQY a consecutive
 * pair; INIT and BIT stand alone.  Code-test coefficients are drawn per row (not for EQ rows), quadratic-test
 * coefficients per triple / pair / bit row, from the streams keyed by stage1_seed, exactly as lig_synth_prove does. ==== */
enum {
    LIG_ROW_LINEAR = 0, LIG_ROW_QX = 1, LIG_ROW_QY = 2, LIG_ROW_QZ = 3, LIG_ROW_INIT = 4, LIG_ROW_BIT = 5, LIG_ROW_EQX = 6,
    LIG_ROW_EQY = 7, LIG_ROW_BQX = 8, LIG_ROW_BQY = 9, LIG_ROW_BQZ = 10,
    LIG_ROW_DRAW_PAD = 0x80      /* or-ed in: slots [l, k) of this row are drawn from the encoding stream by the library */
};
/* lig_rows_job.elem_bytes values with the 0x80 prefix: the two that are not a number of bytes */
enum {
    LIG_ELEM_BIT = 0x81,         /* slot i < l = bit i % 8 of byte i / 8, LSB first (numpy.packbits(bitorder="little")) */
    LIG_ELEM_PRODUCT = 0x82      /* the QZ row of a triple, not shipped: slot i < l = x[i] * y[i] mod p, formed on the device */
};
typedef struct {
    uint64_t rows;                   /* committed rows, the 3 mask rows excluded */
    const uint8_t *kinds;            /* one byte per row (host memory) */
    const void *msgs;                /* rows x k elements, row-major */
    int32_t  msgs_on_device;         /* 0: host memory (uploaded inside the timed path), 1: device memory */
    int32_t  reserved;               /* 0, or LIG_ROWS_JOB_WIDE: this struct has the member wide_per_row (below) and the library may read it */
    uint8_t  encoding_seed[32];
    uint8_t  program_hash[32];
    int64_t  generated_at;
    char     version[16];
    const uint8_t *public_args; const uint64_t *public_arg_lens; uint64_t n_public_args;    /* as in lig_synth_job */
    /* optional (NULL: none): the linear-test randomness rows are the DENSE rows of the synthetic stream -- row r = this many
     * successive elements of the stream keyed by stage1_seed, zeros up to k -- so lig_rows_prove(rands = NULL) may
     * generate them on the device (sampled under the encodes, as lig_synth_prove does) instead of reading them */
    const uint32_t *dense_rands_per_row;
    /* optional (NULL: every row is k full 32-byte elements): the NARROW row format.  One byte per row: 0 or 32 = the row as
     * above; 1, 2, 4 or 8 = only the row's l data slots are supplied, each as a little-endian unsigned integer of that many
     * bytes; LIG_ELEM_BIT = the l data slots are bits, slot i = bit i % 8 of byte i / 8, least significant bit first (real
     * traces are mostly bits and machine words: up to 256x less to move over PCIe; the reference ships 32 bytes per slot,
     * include/util/mpz_vector.hpp:108-127).  `msgs` then holds the rows back to back in commit order, a narrow row taking
     * l * w bytes (ceil(l / 8) for bits) rounded up to a multiple of 4 -- every row starts 4-byte aligned; the padding bytes
     * are ignored -- and a full row k * 32; the library expands them on the device.  A narrow row must be LINEAR / QX / QY / QZ
     * and flagged LIG_ROW_DRAW_PAD (its k - l pad slots are drawn by the library).
     * LIG_ELEM_PRODUCT = a DERIVED row: it contributes no bytes to `msgs`; its data slots i < l are x[i] * y[i] mod p
     * (canonical), x and y being the two rows in front of it, formed on the device from their packed sources, and its pads
     * are drawn by the library.  Only on a row of kind QZ flagged LIG_ROW_DRAW_PAD (directly behind its QX and QY, which may have
     * any of the widths above, flagged or carrying their pads, but are never derived themselves; full-width operands must be
     * canonical, as every full-width row); BQZ rows are device variables and are not accepted.  The prover's own valid_quad is
     * VACUOUS for such a triple, as valid_linear is with const_sum == NULL: a caller whose z was wrong now proves a different
     * z, and a linear constraint on it fails instead.  Any other value, or a value where it is not allowed, is LIG_E_ARG
     * (decided on the host before anything is launched).
     * lig_rows_restart takes the same packed layout, as do lig_shard_rows_begin / _restart (there: one byte per row of the
     * whole trace, `msgs` = this rank's rows only, packed back to back in commit order). */
    const uint8_t *elem_bytes;
    /* optional (NULL: none); one entry per row of the job (of the WHOLE trace on the sharded entry): MIXED rows, narrow rows that
     * carry a few wide slots.  wide_per_row[r] = c > 0: the packed bytes of row r are the narrow row exactly as above (already a
     * multiple of 4 bytes), followed by c RECORDS of 36 bytes: a uint32_t column and the 8 little-endian uint32_t limbs of a
     * canonical field element.  After expansion slot `column` of the row holds the record's value; whatever the narrow part
     * carries at that column is ignored (the caller writes 0 there).  Within a row the columns are strictly ascending and < l.
     * Only on a row of width LIG_ELEM_BIT, 1, 2, 4 or 8 (whose own rules are unchanged), c <= l; c > 0 on a full-width or
     * LIG_ELEM_PRODUCT row, with elem_bytes == NULL, or c > l is LIG_E_ARG, decided on the host before anything is launched.
     * A LIG_ELEM_PRODUCT row whose QX / QY operand rows are mixed sees the records: operand slot i is the record's value where a
     * record names column i.  The counts belong to the shape: lig_rows_restart / lig_shard_rows_restart take rows in the same
     * layout with the same counts; the columns and values inside the records may differ from trace to trace.
     * HOST rows: the records are read before any copy starts (36 c bytes per mixed row); a column >= l or out of order is
     * LIG_E_ARG from lig_rows_begin / _restart / lig_shard_rows_begin / _restart and nothing is launched.  DEVICE rows: a record
     * whose column is >= l is not written and raises a flag word on the device: lig_rows_commit then returns LIG_E_ARG (the
     * trace stays usable: lig_rows_restart with good rows, then commit), lig_shard_rows_begin / _restart return it themselves,
     * before any collective is queued.  Duplicate or unordered columns in device rows are NOT detected: the slots they name
     * (and, in a derived row, the products of those slots) hold an unspecified one of the records' values -- never a write
     * outside the row.  lig_rows_verify_begin ignores the member, as it ignores msgs.
     * The member was appended to the struct: a caller compiled before it existed passes a struct that ENDS at elem_bytes (and
     * reserved = 0, as it always had to).  So the library reads wide_per_row only from a job whose `reserved` has the bit
     * LIG_ROWS_JOB_WIDE; without the bit the job is read exactly as before and nothing past elem_bytes is touched. */
    const uint32_t *wide_per_row;
} lig_rows_job;
enum { LIG_WIDE_RECORD_BYTES = 36, LIG_ROWS_JOB_WIDE = 1 };
int lig_rows_begin(lig_ctx *ctx, const lig_rows_job *job, lig_trace **out);
int lig_rows_commit(lig_trace *trace, uint8_t root[32], uint8_t stage1_seed[32]);
/* const_sum == NULL: the constant is taken to be -sum_r <row_r, rand_r> (returned in info->const_sum) -- for statements that
 * are the rows themselves, like the synthetic stream; the prover's own linear self-check is then vacuous. */
int lig_rows_prove(lig_trace *trace, const void *rands, int rands_on_device, const uint8_t *const_sum,
                   const uint8_t **proof, size_t *proof_len, lig_proof_info *info);
/* Randomness rows handed over WHILE the constraint generator is still producing them (the reference's stage-2 callbacks deliver
 * one row at a time, include/zkp/nonbatch_context.hpp:654-712): after lig_rows_commit, rows [first_row, first_row + n_rows) of the
 * rows x k randomness matrix, in order and without gaps from row 0; host memory (page-locked: lig_host_alloc), valid until
 * lig_rows_prove returns.  The upload starts at once (the library's uploader thread) into a device-resident matrix.  When all
 * rows have been pushed, lig_rows_prove(rands = NULL) uses them: stage 2 waits chunk by chunk for what is still on the bus. */
int lig_rows_push_rands(lig_trace *trace, uint64_t first_row, uint64_t n_rows, const void *host_rows);
/* The same for a generator that puts no linear constraint on many rows (the narrow format of randomness rows): present[i] != 0
 * says that row first_row + i has a randomness row; the present rows follow each other in host_rows (k x 32 bytes each), the
 * others are zero rows and are not shipped -- batch-kind rows always are (nonbatch_context.hpp:782-850 hands no randomness to the
 * vbn254fr hooks), quadratic rows often.  present == NULL: every row is present. */
int lig_rows_push_rands_sparse(lig_trace *trace, uint64_t first_row, uint64_t n_rows, const uint8_t *present, const void *host_rows);
/* the next trace of the same shape (same kinds, seeds, metadata) with new message rows, reusing every buffer of `trace`
 * (no allocation on the proving path of a service); same upload semantics as lig_rows_begin.  It may be called right
 * after lig_rows_commit, BEFORE lig_rows_prove of the committed trace: the new rows then go to a second message matrix
 * and arrive while the current trace is being proved (commit(i) -> restart(i+1) -> prove(i) -> commit(i+1) -> ...). */
int lig_rows_restart(lig_trace *trace, const void *msgs, int msgs_on_device);
/* Host rows travel through one uploader thread per device that waits for every transfer on the host.  A
 * transfer that has not completed after LIG_UPLOAD_TIMEOUT_S (default 5 s; never seen with one process per GPU) does not fail the call:
 * lig_rows_commit / lig_rows_prove discard the stage that ran over the missing rows, wait (bounded by the same time) for the abandoned
 * copy to leave the bus, bring the same rows again with stream-ordered copies and run the stage again -- the proof is the same proof.
 * Only if the abandoned copy is STILL pending after that second wait (it cannot be cancelled) do the calls return LIG_E_HIP; the
 * caller's rows and the trace's device buffers are then still referenced by a DMA transfer: keep the rows alive until
 * *unsettled == 0 here (lig_trace_destroy keeps the device side alive by itself, lig_rows_restart / _commit refuse that trace).
 * *retries = calls of this process that needed the second attempt on ctx's device.  No reference counterpart
 * (src/webgpu/device_context.cpp:364-449 blocks in wgpuQueueWriteBuffer).  Either pointer may be NULL. */
int lig_upload_health(lig_ctx *ctx, uint32_t *retries, uint32_t *unsettled);
/* The verifier's side of a rows job (src/webgpu_verifier.cpp:263-452 with the rows of nonbatch_verifier_context,
 * include/zkp/nonbatch_context.hpp:1219-1287): begin parses the envelope, re-derives both seeds and the sample indices from the
 * job's public data (kinds, public arguments; msgs is ignored) and returns the stage-1 seed; the caller's constraint generator
 * produces the randomness rows and the linear constant from it; finish recommits the 192 opened columns, encodes the
 * randomness rows, evaluates the seven predicates and frees the trace.  A malformed envelope is not an error: begin returns
 * LIG_OK with out->accept = 0 (out->parsed / out->indices_match say why) and *trace = NULL. */
typedef struct lig_vtrace lig_vtrace;
int lig_rows_verify_begin(lig_ctx *ctx, const lig_rows_job *job, const uint8_t *proof, size_t proof_len, lig_vtrace **trace,
                          uint8_t stage1_seed[32], lig_verify_info *out);
int lig_rows_verify_finish(lig_vtrace *trace, const void *rands, int rands_on_device, const uint8_t const_sum[32], lig_verify_info *out);
/* a verifier that gives up between begin and finish (its constraint generator threw) frees the trace here; NULL is a no-op */
void lig_vtrace_destroy(lig_vtrace *trace);
/* rows x k dense randomness rows on the device: row r = per_row[r] successive elements of the AES-256-CTR field stream
 * keyed by key32 (row r starts where row r-1 ended, the first at first_elem), zeros up to k -- the linear-test
 * coefficient rows of the synthetic stream, for callers that feed lig_rows_prove from the device. */
int lig_rng_fill_rows(lig_ctx *ctx, const uint8_t *key32, uint64_t first_elem, const uint32_t *per_row_host, size_t rows, void *out);

/* ==== sparse linear constraints: the linear-test randomness rows formed by the library (csrc/linear.hip).  The randomness rows a
 * caller hands to lig_rows_prove are not random data: every linear constraint c draws ONE element r_c from the linear random engine
 * (witness_manager::generate_linear_random, include/zkp/backend/witness_manager.hpp:344-348; the engine is keyed by the stage-1 seed,
 * include/zkp/nonbatch_context.hpp:105-112) and adds a * r_c to the randomness of each witness it touches (witness_add_random /
 * witness_sub_random, :356-372), b_c * r_c to the public constant (constsum_add / _sub, :374-388).  For constraints
 * sum_j a_cj * w[slot_cj] = b_c:
 *     Rn[slot s] = sum over terms (c, s, a) of a * r_c            const_sum = - sum_c b_c * r_c
 * Which constraint touches which slot with which coefficient does not depend on the seed: the caller describes it ONCE as a term
 * list of integers, the library draws r_c and forms matrix and constant on the GPU, for the prover and for the verifier.  Nothing of
 * the randomness crosses the host link per proof, and a caller whose constraint structure is fixed no longer re-runs its guest
 * between stage 1 and stage 2.  All pointers are host memory, copied before the call that takes the system returns. ==== */
enum { LIG_COEF_ONE = 0xFFFFFFFFu, LIG_COEF_NEG_ONE = 0xFFFFFFFEu };   /* coefficient "indices" that need no table entry */
typedef struct { uint32_t slot; uint32_t coef; } lig_lin_term;
/* slot = row * l + column: row = index among the job's committed rows (masks excluded), column < l;
 * coef = index into coefs[], or LIG_COEF_ONE / LIG_COEF_NEG_ONE */
typedef struct {
    uint32_t struct_bytes;              /* sizeof(lig_linear_system) as the caller sees it; smaller than the library's: LIG_E_ARG */
    uint32_t reserved;
    uint64_t n_constraints, n_terms;    /* n_terms < 2^32 */
    const uint32_t *term_begin;         /* n_constraints + 1 entries, non-decreasing, [0] = 0, [n_constraints] = n_terms */
    const lig_lin_term *terms;          /* constraint c owns terms [term_begin[c], term_begin[c+1]); may be empty; a slot may repeat */
    const uint32_t *rhs_constraint;     /* n_rhs constraint numbers, strictly ascending: the constraints with b_c != 0 */
    const uint32_t *rhs_coef;           /* n_rhs coefficient indices: b_c */
    uint64_t n_rhs;
    const uint8_t *coefs; uint64_t n_coefs;   /* n_coefs x 32 bytes, canonical elements (>= p is LIG_E_ARG) */
    uint64_t first_random;              /* constraint c draws element first_random + c of the stream keyed by stage1_seed */
} lig_linear_system;
/* host only, no context: every rule above; every slot / l < rows and on a row of kind LINEAR / QX / QY / QZ (batch-kind rows carry no
 * linear-test randomness, nonbatch_context.hpp:782-850); every coefficient index < n_coefs or one of the two specials;
 * rows * l < 2^32.  LIG_E_ARG otherwise.  Every entry below runs this before anything is launched: an index out of range never
 * reaches a kernel. */
int lig_linear_check(const lig_linear_system *sys, const uint8_t *kinds, uint64_t rows, uint32_t l);
/* any time after lig_rows_begin and before lig_rows_prove (before or after lig_rows_commit): uploads the structure and regroups it
 * by slot once; it survives lig_rows_restart (same shape, same constraints) and is freed by lig_trace_destroy; a second call
 * replaces it; sys == NULL removes it.  LIG_E_ARG for a system lig_linear_check rejects and for a job with dense_rands_per_row;
 * LIG_E_STATE when randomness rows have already been pushed (lig_rows_push_rands*).
 * With a system set, lig_rows_prove(rands = NULL) forms the randomness matrix on the device (side stream, under the first encodes of
 * stage 2) and runs stage 2 on it exactly as on an uploaded matrix.  const_sum == NULL then means the system's constant
 * -sum_c b_c r_c (returned in info->const_sum): info->valid_linear is a real check of the statement.  A non-NULL const_sum is used
 * as given.  While a system is set, lig_rows_prove(rands != NULL) is LIG_E_ARG and lig_rows_push_rands* is LIG_E_STATE. */
int lig_rows_set_linear(lig_trace *trace, const lig_linear_system *sys);
/* the verifier's side, between lig_rows_verify_begin and _finish: lig_rows_verify_finish(trace, NULL, 0, NULL, out) then forms
 * matrix and constant itself -- the sound verifier of a rows job: it needs nothing but the envelope and the public structure.
 * (A non-NULL const_sum is used as given; rands != NULL with a system set is LIG_E_ARG.)  sys == NULL removes the system. */
int lig_rows_verify_set_linear(lig_vtrace *trace, const lig_linear_system *sys);
/* stand-alone: rands_dev (rows x k x 32 bytes of device memory) <- the randomness matrix for the stream keyed by key32, const_sum <-
 * the constant; blocking.  Slots [l, k) of every row, rows no term touches and batch-kind rows come out zero, as
 * process_reset_linear_row leaves them (witness_manager.hpp:211-214).  For a caller with its own stage-2 driver. */
int lig_linear_form(lig_ctx *ctx, const lig_linear_system *sys, const uint8_t *kinds, uint64_t rows, const uint8_t key32[32],
                    void *rands_dev, uint8_t const_sum[32]);

/* ---- prepared linear systems: one resident structure for many proofs, many verifications, several contexts.
 * lig_rows_set_linear / lig_rows_verify_set_linear / lig_linear_form above prepare a structure that ONE trace owns.  The entries
 * below split that in two: the PROGRAM (the regrouped structure: immutable, reference counted, shared) and the ATTACHMENT of one
 * trace to it (what a proof writes: the sampled r_c, partial sums, the constant, an overriding coefficient table).  A verifier
 * service prepares once and attaches per envelope; two contexts proving the same guest hold one copy; a new statement of the same
 * program (other right-hand sides) is lig_rows_set_linear_values, not a new prepare.
 * On the sharded entry a rank's structure depends on its deal and nothing shares it (no program object), but a new statement is likewise
 * a call of lig_shard_rows_set_linear_values below, not a second lig_shard_rows_set_linear. */
typedef struct lig_linear_program lig_linear_program;
/* check (lig_linear_check), upload, regroup by slot -- what lig_rows_set_linear does -- into an immutable, reference-counted object
 * bound to ctx's DEVICE and (l, k), not to ctx: it may be attached to traces of any context of this process on that device, from any
 * thread, and outlives ctx.  Synchronous: every pointer of *sys may be released when it returns; nothing writes the program's device
 * memory afterwards.  The caller owns one reference.  LIG_E_ARG for a system lig_linear_check rejects (nothing is launched). */
int  lig_linear_prepare(lig_ctx *ctx, const lig_linear_system *sys, const uint8_t *kinds, uint64_t rows, lig_linear_program **out);
/* drops the caller's reference; NULL is a no-op.  Every attachment holds a reference of its own, so this may come before
 * lig_trace_destroy / lig_rows_verify_finish / lig_vtrace_destroy; device memory goes with the last reference (atomic count). */
void lig_linear_program_release(lig_linear_program *p);
/* host only: the device memory the program holds, and what EVERY attachment to it allocates on top (r and the partial sums; an
 * attachment with values of its own adds n_coefs x 32) -- the sizes of the library's own allocations */
int  lig_linear_program_bytes(const lig_linear_program *p, uint64_t *program_bytes, uint64_t *attachment_bytes);
/* lig_rows_set_linear with a prepared program: same window (after lig_rows_begin, before lig_rows_prove), same effect on
 * lig_rows_prove (rands == NULL forms the matrix; const_sum == NULL is the system's constant), survives lig_rows_restart, replaces
 * a system set with lig_rows_set_linear and is replaced by one; p == NULL detaches.  Checked on the host before anything is
 * launched: the trace has the program's device, l, k, row count and row kinds (LIG_ROW_DRAW_PAD masked off), else LIG_E_ARG;
 * LIG_E_ARG for a job with dense_rands_per_row; LIG_E_STATE after lig_rows_push_rands*.  While attached, lig_rows_prove(rands !=
 * NULL) is LIG_E_ARG and lig_rows_push_rands* is LIG_E_STATE. */
int  lig_rows_attach_linear(lig_trace *trace, const lig_linear_program *p);
/* the verifier's side (lig_rows_verify_set_linear with a prepared program); the attachment goes with lig_rows_verify_finish or
 * lig_vtrace_destroy */
int  lig_rows_verify_attach_linear(lig_vtrace *trace, const lig_linear_program *p);
/* per-proof VALUES of the coefficient table of the attached structure: coefs[] with the program's n_coefs, canonical -- the public
 * right-hand sides b_c of a new statement are the entries named by rhs_coef.  They belong to the attachment, not the program (two
 * traces on one program may carry different values), and stay over lig_rows_restart until set again; coefs == NULL: back to the
 * program's own table.  Copied before the call returns; the table is converted on the device, on the stream the forms run on.
 * LIG_E_ARG: another n_coefs, an entry >= p (decided on the host, nothing launched); LIG_E_STATE: nothing attached. */
int  lig_rows_set_linear_values(lig_trace *trace, const uint8_t *coefs, uint64_t n_coefs);
int  lig_rows_verify_set_linear_values(lig_vtrace *trace, const uint8_t *coefs, uint64_t n_coefs);
/* lig_linear_form without the prepare (blocking); coefs == NULL uses the program's table.  LIG_E_ARG when ctx is on another device
 * or has another (l, k). */
int  lig_linear_program_form(lig_ctx *ctx, const lig_linear_program *p, const uint8_t key32[32], const uint8_t *coefs, uint64_t n_coefs,
                             void *rands_dev, uint8_t const_sum[32]);

/* ---- which constraints does the committed witness violate?  (csrc/diagnose.hip)
 * Upstream a bad witness is caught while the guest runs: constrain_equal / constrain_bit assert on the values
 * (include/zkp/backend/witness_manager.hpp:418-431).  A caller of the entries above no longer runs that code, and what is left are
 * the prover's self-check bits: valid_linear is ONE bit computed from a random combination, valid_quad is vacuous for a derived
 * triple (LIG_ELEM_PRODUCT).  lig_rows_diagnose evaluates the statement itself on the committed witness matrix -- exactly, without
 * randomness -- and names the violated constraints.
 *   linear     res_c = sum_j a_cj * w[slot_cj] - b_c mod p (canonical) for every constraint c of `sys`, over the data slots of the
 *              committed trace (derived rows included); b_c = the table entry named by rhs_coef when c is in rhs_constraint, else 0.
 *              The coefficient table is sys->coefs AS PASSED HERE (a caller of lig_rows_set_linear_values passes that statement's
 *              values).  sys goes through lig_linear_check against the trace's kinds before anything is launched (LIG_E_ARG); the
 *              system or program attached to the trace is neither used nor modified.  sys == NULL: the quadratic part only.
 *   quadratic  for every quadratic-test term of the job in commit order -- a QX,QY,QZ / BQX,BQY,BQZ triple: x[i] * y[i] - z[i]; a BIT
 *              row b (row_x = row_y = row_z = that row): b[i] * b[i] - b[i]; an EQX,EQY pair: x[i] - z[i] with row_y = 0xFFFFFFFF
 *              and row_z = the EQY row -- and every column i < l.  Row numbers count the job's committed rows (masks excluded).
 *   output     the first lin_cap violated constraints in ascending constraint number, the first quad_cap violated (term, column)
 *              pairs in ascending (term, column) order: the same bytes on every run.  The counts in *info cover ALL violations,
 *              reported or not.  A cap of 0 (the array may then be NULL) gives counts only; NULL with a cap > 0 is LIG_E_ARG.
 * WHEN: from the return of lig_rows_commit until the committed matrix is replaced -- by the next lig_rows_commit on the trace, or by
 * a lig_rows_restart issued AFTER lig_rows_prove (it loads straight into the matrix); a lig_rows_restart between commit and prove
 * writes the second matrix and does not end the window.  Before or after lig_rows_prove.  Outside the window, and for a trace made
 * by lig_synth_prepare: LIG_E_STATE.  The call blocks, only reads the matrix and runs on the context stream; it changes nothing a
 * proof depends on (the envelope of a diagnosed trace is byte-identical to that of one that was not).  Scratch is allocated inside
 * the call and freed before it returns: this is not the proving path.  Its work is enqueued on the context stream alone, but freeing
 * the scratch waits for the whole device: while the rows of a lig_rows_restart are still arriving, the call returns after them.
 * info->ms_total is the whole call, the host pass of lig_linear_check over sys (one step per term) included.
 * The sharded entry has its own call, lig_shard_rows_diagnose below (a rank holds only the rows it was dealt and a constraint may span
 * ranks).  There is no verifier side: the verifier has no witness. */
typedef struct { uint32_t constraint, reserved; uint8_t residual[32]; } lig_diag_linear;          /* 40 bytes */
typedef struct { uint32_t row_x, row_y, row_z, column; uint8_t residual[32]; } lig_diag_quad;     /* 48 bytes */
typedef struct {
    uint32_t struct_bytes, reserved;     /* sizeof(lig_diag_info) as the caller sees it; smaller than the library's: LIG_E_ARG */
    uint64_t n_linear_bad;               /* constraints of sys with a nonzero residual (all of them, not only the reported ones) */
    uint64_t n_quad_bad;                 /* (quadratic term, column < l) pairs with a nonzero residual */
    uint64_t n_linear_reported, n_quad_reported;
    double   ms_total;                   /* wall time of the call */
} lig_diag_info;
int lig_rows_diagnose(lig_trace *trace, const lig_linear_system *sys, lig_diag_linear *lin_out, uint64_t lin_cap,
                      lig_diag_quad *quad_out, uint64_t quad_cap, lig_diag_info *info);
/* lig_rows_diagnose against the statement ATTACHED to the trace: the one lig_rows_prove(rands = NULL, const_sum = NULL) would prove.  For
 * the caller of lig_linear_prepare who has released the term list, and for the caller of lig_rows_set_linear_values who would otherwise
 * have to pass "the table of THIS statement" by hand.
 *   structure  what lig_rows_set_linear or lig_rows_attach_linear attached.  Nothing attached: LIG_E_STATE.
 *   values     the coefficient table in force for THIS trace: the one given to lig_rows_set_linear_values if one is set, else the
 *              program's own.  Two traces attached to one program with different values each get their own answer.
 *   output     order, counts, caps, record layouts and *info exactly as for lig_rows_diagnose: for the same statement the two calls
 *              return the same bytes.  The quadratic part is the same pass over the same trace.
 * The program keeps its terms grouped by slot; the call regroups them by constraint on the device (count, scan, scatter: the prepare run
 * the other way, csrc/diagnose.hip), reads the right-hand sides and the table where they are, and then runs the passes of
 * lig_rows_diagnose.  No host pass over the terms, no upload.  WHEN, blocking, streams and scratch as for lig_rows_diagnose (scratch:
 * 8 n_terms + 8 n_constraints for the regrouped list, on top of the residuals and records); a table lig_rows_set_linear_values is still
 * converting on the side stream is waited for with an event, not with a device-wide synchronise.  It writes nothing the program or the
 * attachment owns -- not the sampled elements, not the partial sums, not the constant, not the table -- and the envelope of a trace
 * diagnosed this way is byte-identical to that of one that was not.  LIG_E_STATE outside the window, for a lig_synth_prepare trace and
 * when nothing is attached; LIG_E_ARG for a NULL array with a cap > 0, a NULL or too small *info, a NULL trace; all decided on the host
 * before anything is launched.  info->ms_total is the whole call.
 * The sharded entry has its own call, lig_shard_rows_diagnose_attached below. */
int lig_rows_diagnose_attached(lig_trace *trace, lig_diag_linear *lin_out, uint64_t lin_cap, lig_diag_quad *quad_out, uint64_t quad_cap,
                               lig_diag_info *info);

/* ---- explain a constraint: its terms, coefficients and witness values  (csrc/diagnose.hip)
 * lig_rows_diagnose* NAME the violated constraints; these entries SHOW constraints, as the library holds them.  Upstream constrain_equal /
 * constrain_bit assert with the values in hand (witness_manager.hpp:418-431); a caller who released its term list after
 * lig_linear_prepare, or whose QZ rows are derived on the device (LIG_ELEM_PRODUCT), or whose rows are mixed (wide_per_row), has neither
 * the terms nor the witness values any more.
 *   constraints  n_asked constraint numbers of the statement, strictly ascending, each < n_constraints (else LIG_E_ARG).
 *   con_out      n_asked records (required when n_asked > 0), record i for asked constraint i:
 *                  n_terms     ALL its terms, reported or not; 0 for an empty constraint
 *                  first_term  the index of its first term in the full output order below (may be >= term_cap)
 *                  rhs         b_c, canonical: the table entry named by rhs_coef, zero when the constraint is not in rhs_constraint
 *                  residual    sum a * w - b_c over all its terms, canonical: the 32 bytes lig_rows_diagnose writes for the constraint
 *                              when it is violated, zero when it holds
 *   terms_out    the first term_cap records of the full order: ascending asked constraint, then ascending slot, then ascending
 *                coef_index as an unsigned number (LIG_COEF_NEG_ONE, LIG_COEF_ONE come last).  A term the statement holds twice appears
 *                twice.  coef = the canonical value the index stands for (1, p - 1, or the table entry IN FORCE); value = the canonical
 *                committed w[slot] -- on a derived row the product the device formed, on a record slot of a mixed row the record's
 *                value.  Records that compare equal in this order are byte-identical: no output byte depends on an atomic, on
 *                scheduling, or on which lig_linear_prepare of the same system made the program.  NULL with term_cap = 0 gives the
 *                counts and con_out only.
 *   info         n_terms_total = the terms of all asked constraints, n_terms_reported = min(n_terms_total, term_cap); ms_total = the
 *                whole call.
 * lig_rows_explain uses `sys` AS PASSED, like lig_rows_diagnose: it goes through lig_linear_check against the trace's kinds first
 * (LIG_E_ARG; sys == NULL is LIG_E_ARG here), and what is attached to the trace is neither used nor modified.
 * lig_rows_explain_attached uses what lig_rows_set_linear / lig_rows_attach_linear attached, with the table of
 * lig_rows_set_linear_values in force if one is set (a conversion still running on the side stream is waited for with its event, not
 * with a device-wide synchronise); nothing attached: LIG_E_STATE.  For the same statement the two calls return the same bytes.
 * lig_rows_read_slots: values[i] (32 bytes) = the canonical committed element of slots[i] = row * l + column, over the committed rows
 * of ANY kind (masks excluded), column < l; any order, repeats allowed; a slot >= rows * l is LIG_E_ARG; n_slots = 0 is LIG_OK and
 * launches nothing.
 * WHEN, blocking, streams as for lig_rows_diagnose: inside its window (LIG_E_STATE outside, and for a lig_synth_prepare trace), work
 * enqueued on the context stream alone, scratch allocated per call and freed before it returns.  Nothing a proof depends on is written
 * (the envelope of a trace that was explained or read is byte-identical to that of one that was not), nothing the program or the
 * attachment owns is written.  The attached entry selects the asked terms straight from the program's slot-major index (one mark
 * pass over its entries, a scan, a collect: no regrouping of the statement, no atomic); the m selected 12-byte items are ordered on the
 * host.  Scratch, attached: 8 (n_terms + 1) for marks and positions, 4 n_constraints for the right-hand-side index, 4 n_asked; term
 * list: the uploaded system as for lig_rows_diagnose, 8 n_asked; both: 20 m for the items, 88 n_asked + 84 min(m, term_cap) for the
 * records.  LIG_E_ARG: a NULL trace, a NULL or too small *info, con_out == NULL or constraints == NULL with n_asked > 0, terms_out ==
 * NULL with term_cap > 0, slots or values == NULL with n_slots > 0, and the range errors above -- all decided on the host before
 * anything is launched: an index out of range never reaches a kernel.
 * The sharded entry has its own calls, lig_shard_rows_explain / lig_shard_rows_read_slots below.  Not covered: a verifier side (the
 * verifier has no witness). */
typedef struct { uint32_t constraint, slot, coef_index, reserved; uint8_t coef[32]; uint8_t value[32]; } lig_explain_term;       /* 80 bytes */
typedef struct { uint32_t constraint, reserved; uint64_t n_terms, first_term; uint8_t rhs[32]; uint8_t residual[32]; } lig_explain_constraint; /* 88 bytes */
typedef struct {
    uint32_t struct_bytes, reserved;     /* sizeof(lig_explain_info) as the caller sees it; smaller than the library's: LIG_E_ARG */
    uint64_t n_terms_total, n_terms_reported;
    double   ms_total;                   /* wall time of the call */
} lig_explain_info;
int lig_rows_explain(lig_trace *trace, const lig_linear_system *sys, const uint32_t *constraints, uint64_t n_asked,
                     lig_explain_constraint *con_out, lig_explain_term *terms_out, uint64_t term_cap, lig_explain_info *info);
int lig_rows_explain_attached(lig_trace *trace, const uint32_t *constraints, uint64_t n_asked,
                              lig_explain_constraint *con_out, lig_explain_term *terms_out, uint64_t term_cap, lig_explain_info *info);
int lig_rows_read_slots(lig_trace *trace, const uint32_t *slots, uint64_t n_slots, uint8_t *values /* n_slots x 32 */);

/* ---- explain a slot: the constraints that touch it; and the witness slots no constraint touches  (csrc/diagnose.hip)
 * lig_rows_explain* start from a constraint and show its slots; these entries start from a SLOT.  "Constraint 17 fails and names slots 123,
 * 700 and 2500: which other constraints use slot 700, and do they hold?"  -- if all of them hold, the wrong value is elsewhere in
 * constraint 17; if several fail, slot 700 is the culprit.  The program keeps the terms grouped by slot (begin[], ent[] of
 * csrc/linear.hip), so the constraints through a slot are one contiguous segment of it and nothing is regrouped.
 *   slots        n_asked slot numbers row * l + column, STRICTLY ASCENDING, each < rows * l, over the committed rows of any kind (masks
 *                excluded); anything else is LIG_E_ARG.  A slot of a batch-kind row has no term (lig_linear_check admits none there).
 *   slot_out     n_asked records (required when n_asked > 0), record i for asked slot i:
 *                  row_kind    the kind of its row, LIG_ROW_DRAW_PAD masked off
 *                  value       the canonical committed w[slot]: the 32 bytes lig_rows_read_slots returns -- on a derived row the product
 *                              the device formed, on a record slot of a mixed row the record's value
 *                  n_terms     ALL terms of the statement on that slot, reported or not
 *                  first_term  the index of its first term in the full output order below (may be >= term_cap)
 *   terms_out    the first term_cap records of the full order: ascending asked slot, then ascending constraint, then ascending coef_index
 *                as an unsigned number (LIG_COEF_NEG_ONE, LIG_COEF_ONE come last).  A term the statement holds twice appears twice.
 *                  coef              the canonical value the index stands for: 1, p - 1, or the table entry IN FORCE
 *                  constraint_terms  the number of terms of that constraint (on all slots)
 *                  residual          sum a * w - b_c of that constraint, canonical: the 32 bytes lig_rows_explain* write for it, zero
 *                                    when it holds
 *                Records that compare equal in this order are byte-identical: no output byte depends on an atomic, on scheduling, or on
 *                which lig_linear_prepare of the same system made the program.  NULL with term_cap = 0 gives the counts and slot_out only.
 *   info         n_terms_total = the terms of all asked slots, n_terms_reported = min(n_terms_total, term_cap), n_constraints_distinct =
 *                the distinct constraints over all asked slots; ms_total = the whole call.
 * lig_rows_explain_slots_attached uses what lig_rows_set_linear / lig_rows_attach_linear attached, with the table of
 * lig_rows_set_linear_values in force if one is set (a conversion still running on the side stream is waited for with its event);
 * nothing attached: LIG_E_STATE.  lig_rows_explain_slots takes `sys` AS PASSED: it goes through lig_linear_check against the trace's
 * kinds first (LIG_E_ARG; sys == NULL is LIG_E_ARG), is regrouped by slot into a temporary program (the prepare of lig_linear_prepare:
 * 8 n_terms + 4 rows * l device bytes and as much again in scratch) that is released before the call returns; what is attached to the
 * trace is neither used nor modified.  For the same statement the two calls return the same bytes.
 * How: the segment lengths of the asked slots, an exclusive scan, one lane per (constraint, coef_index) item -- whole workgroups for a
 * slot with more than 2048 terms --, no atomic; the m 12-byte items are ordered on the host; the residuals and sizes of the distinct
 * constraints come from the selection pass of lig_rows_explain_attached itself (no second evaluator), the values from the gather of
 * lig_rows_read_slots.  Scratch on top of that pass: 8 n_asked + 36 n_asked for slots, lengths and values, 12 m for the items,
 * 88 distinct + 96 min(m, term_cap) for the records.
 *
 * lig_rows_untouched_slots*: the slots row * l + column, column < l, of the rows of kind LINEAR / QX / QY / QZ that NO term of the
 * statement touches -- an under-constrained witness, the classic defect of a statement recorded by hand --, in ascending order, the
 * first `cap` of them, each with its row kind and committed value.  nonzero_only != 0 restricts the list and n_reported to the slots
 * whose committed value is not zero (the zero fill of a short row drops out); n_untouched and n_untouched_nonzero always count all of
 * them.  cap = 0 (`out` may then be NULL) gives the counts only; NULL with cap > 0 is LIG_E_ARG.  The flags (segment empty; value
 * nonzero, read with 16-byte loads) go through one scan that carries both counts, then a compaction: no atomic.  The slots are processed
 * in slices of 2^22 (16 bytes of scratch per slot of a slice, 40 per reported record); counts and offsets are carried on the host.
 * The _attached / `sys` variants differ as above.
 *
 * WHEN, blocking, streams and scratch exactly as for lig_rows_explain*: inside the window of lig_rows_diagnose (LIG_E_STATE outside, and
 * for a lig_synth_prepare trace), work enqueued on the context stream alone, scratch allocated per call and freed before it returns.
 * Nothing a proof depends on is written (the envelope of a trace that was asked is byte-identical to that of one that was not), nothing
 * the program or the attachment owns is written.  LIG_E_ARG: a NULL trace, a NULL or too small *info, slots == NULL or slot_out == NULL
 * with n_asked > 0, terms_out == NULL with term_cap > 0, out == NULL with cap > 0, and the range and order errors above -- all decided
 * on the host before anything is launched: an index out of range never reaches a kernel.  n_asked = 0 is LIG_OK and launches nothing.
 * The new structs version themselves with struct_bytes; they are not part of lig_abi_sizes (LIG_ABI_STRUCTS stays 6).
 * The sharded entry (a rank's share numbers its slots locally and holds only the terms of its rows) has its own calls,
 * lig_shard_rows_explain_slots* / lig_shard_rows_untouched_slots* below; a share of a sharded trace attached here is LIG_E_STATE. */
typedef struct { uint32_t slot, row_kind; uint64_t n_terms, first_term; uint8_t value[32]; } lig_slot_record;                /* 56 bytes */
typedef struct { uint32_t slot, constraint, coef_index, constraint_terms; uint8_t coef[32]; uint8_t residual[32]; } lig_slot_term; /* 80 bytes */
typedef struct {
    uint32_t struct_bytes, reserved;     /* sizeof(lig_slot_info) as the caller sees it; smaller than the library's: LIG_E_ARG */
    uint64_t n_terms_total, n_terms_reported, n_constraints_distinct;
    double   ms_total;                   /* wall time of the call */
} lig_slot_info;                                                                                                                /* 40 bytes */
int lig_rows_explain_slots_attached(lig_trace *trace, const uint32_t *slots, uint64_t n_asked,
                                    lig_slot_record *slot_out, lig_slot_term *terms_out, uint64_t term_cap, lig_slot_info *info);
int lig_rows_explain_slots(lig_trace *trace, const lig_linear_system *sys, const uint32_t *slots, uint64_t n_asked,
                           lig_slot_record *slot_out, lig_slot_term *terms_out, uint64_t term_cap, lig_slot_info *info);
typedef struct { uint32_t slot, row_kind; uint8_t value[32]; } lig_slot_value;                                                 /* 40 bytes */
typedef struct {
    uint32_t struct_bytes, reserved;     /* sizeof(lig_untouched_info) as the caller sees it; smaller than the library's: LIG_E_ARG */
    uint64_t n_untouched, n_untouched_nonzero, n_reported;
    double   ms_total;                   /* wall time of the call */
} lig_untouched_info;                                                                                                           /* 40 bytes */
int lig_rows_untouched_slots_attached(lig_trace *trace, int nonzero_only, lig_slot_value *out, uint64_t cap, lig_untouched_info *info);
int lig_rows_untouched_slots(lig_trace *trace, const lig_linear_system *sys, int nonzero_only, lig_slot_value *out, uint64_t cap,
                             lig_untouched_info *info);

/* ---- derived slots: the outputs of linear constraints formed on the device  (csrc/derive.hip, csrc/derive_plan.hpp)
 * Upstream every backend.eval(expr) (include/zkp/backend/core.hpp:311) creates a NEW witness whose value is a linear expression of older
 * witnesses, tied to them by one linear constraint in which it has coefficient -1.  A caller that recorded its term list holds that
 * constraint already; with the entries below it no longer evaluates the expression per proof, and the slot needs no bytes on the link (a
 * bit row whose only wide slots are eval outputs stays a pure LIG_ELEM_BIT row, without records).  The linear counterpart of
 * LIG_ELEM_PRODUCT.
 *   A derived slot t with DEFINING constraint c of `sys`, sum_j a_j * w[s_j] = b_c: t occurs exactly once among the terms of c, with
 *   coefficient index LIG_COEF_ONE or LIG_COEF_NEG_ONE, and its committed value is
 *       w[t] = b_c - sum_{j != t} a_j * w[s_j]   (coefficient +1)        w[t] = sum_{j != t} a_j * w[s_j] - b_c   (coefficient -1)
 *   canonical, mod p.  Whatever the caller's row carries at t is IGNORED (the caller writes 0 there, as for the column of a mixed-row
 *   record).  The other terms may lie on any LINEAR / QX / QY / QZ row of the trace: rows behind t's row, LIG_ELEM_PRODUCT rows, other
 *   derived slots.  A slot derived from derived slots belongs to a later WAVE: wave = 1 + the largest wave among its derived terms (0 for
 *   a slot that is not derived), computed on the host; at most LIG_DERIVE_MAX_WAVES.
 *   A PRODUCT ENTRY {slot, LIG_DERIVED_PRODUCT} names column i < l of a LIG_ELEM_PRODUCT row r (slot = r * l + i).  Its committed value is
 *       w[r * l + i] = w[(r - 2) * l + i] * w[(r - 1) * l + i] mod p, canonical,
 *   read from the EXPANDED matrix in wave order -- so the records of mixed operand rows and operands derived in earlier waves are seen --
 *   and it overwrites what the row's own pass wrote there from the packed sources.  With it the two mechanisms compose: column i of the
 *   QX / QY row in front of a LIG_ELEM_PRODUCT row may be a derived slot IF the list also holds the product entry of column i of that
 *   row.  t = eval(a + b); u = t * c; v = eval(u + d): list t with its constraint, u as a product entry, v with its constraint -- three
 *   waves, and only a, b, c, d are shipped.  One wave numbering covers both kinds: a product entry is in wave 1 + max(wave(x_i),
 *   wave(y_i)); one whose operands are both shipped is accepted in wave 1 and re-forms the same value; a target that reads a listed
 *   product slot is in a later wave than it.
 * lig_derived_check: host only, no context.  lig_linear_check(sys, kinds, rows, l) first; then LIG_E_ARG for: a slot listed twice (two
 * entries of either kind); a constraint >= n_constraints; a target absent from its constraint or present twice; a target whose
 * coefficient is a table index (even one whose value is 1); a cycle, also one through a product entry (x_i defined by a constraint that
 * reads z_i); more than LIG_DERIVE_MAX_WAVES waves; a linear target on a LIG_ELEM_PRODUCT row; a target that is an operand slot of a
 * LIG_ELEM_PRODUCT row -- column i of the QX or QY row directly in front of one -- WITHOUT the product entry of column i of that row: the
 * row's own pass forms the product from the PACKED operand rows and would not see the derived value; a product entry on anything but a
 * data slot of a row whose elem_bytes is LIG_ELEM_PRODUCT (elem_bytes == NULL, a LINEAR row, a shipped QZ row).  elem_bytes: as in
 * lig_rows_job (one per row), NULL: no row is derived.  d may be in any order; n == 0 is accepted (no wave).  wave_out (n entries, or
 * NULL) <- the wave of d[i], product entries included; *info (or NULL; struct_bytes set by the caller) <- n_slots = n, n_terms = the
 * OTHER terms of all defining constraints + 2 per product entry, n_waves.
 * lig_rows_set_derived: runs that check against the trace's kinds and widths (LIG_E_ARG, nothing launched, the previous list stays in
 * force and the trace usable), then COPIES what it needs before it returns: the terms of the n defining constraints, their right-hand-side
 * table entries, and the table values of sys->coefs AS PASSED (converted to Montgomery form on the device once per call); the rest of sys
 * is not kept.  Any time after lig_rows_begin; the list applies from the next lig_rows_commit on and survives lig_rows_restart; a second
 * call replaces it; d == NULL or n == 0 removes it.  LIG_E_STATE for a lig_synth_prepare trace.  It is independent of what is attached for
 * proving: it works with lig_rows_set_linear, with lig_rows_attach_linear and with caller-supplied randomness rows.
 * lig_rows_set_linear_values does NOT reach it: for other right-hand sides call lig_rows_set_derived again with the new table.
 *   WHERE  in lig_rows_commit, on the encode stream, after every row of the trace has been expanded (derived product rows and the records
 *          of mixed rows included) and before the first encode: one launch per wave, written into the matrix THIS commit encodes (after a
 *          lig_rows_restart issued between commit and prove that is the second matrix); the pads are not touched (derived slots are data
 *          slots < l).  The second attempt of a commit whose upload timed out runs the pass again.  HOST rows that arrive chunk by chunk:
 *          with a list set, the arrival wait, expansion and pads of ALL chunks are queued first, then the waves, then the encodes -- the
 *          upload / encode overlap is given up for such a trace, and only for such a trace (LIG_SHA_GATE=2 is ignored while a list is
 *          set).  Without a list stage 1 queues exactly what it queued before.
 *   READERS of the committed matrix see the derived values: lig_rows_diagnose*, lig_rows_explain*, lig_rows_read_slots,
 *          lig_rows_explain_slots*.  The verifier side ignores the list, as it ignores msgs.
 *   The prover's valid_linear CANNOT fail on a defining constraint (as valid_quad is vacuous for a LIG_ELEM_PRODUCT triple): a caller whose
 *   own evaluation would have been wrong now proves a different w, and the OTHER constraints on that slot fail instead.
 *   Deterministic: one lane (a workgroup with a fixed summation tree for a constraint with more than 64 other terms) per target, no
 *   atomic on a field element: the same bytes on every run.  The product entries of a wave are one more launch, one lane per entry.
 * The sharded entry: lig_shard_rows_set_derived, below lig_shard_rows_set_linear.  Not done: per-chunk reach, so that a chunk waits only
 * for the rows its derived slots read; product entries on shipped QZ rows.
 * The new structs version themselves with struct_bytes; they are not part of lig_abi_sizes (LIG_ABI_STRUCTS stays 6). */
enum { LIG_DERIVE_MAX_WAVES = 16 };
#define LIG_DERIVED_PRODUCT 0xFFFFFFFFu   /* lig_derived_slot.constraint: a product entry */
typedef struct { uint32_t slot, constraint; } lig_derived_slot;                                                     /* 8 bytes */
typedef struct { uint32_t struct_bytes, reserved; uint64_t n_slots, n_terms; uint32_t n_waves, reserved2; } lig_derived_info;   /* 32 bytes */
int lig_derived_check(const lig_linear_system *sys, const uint8_t *kinds, uint64_t rows, uint32_t l, const uint8_t *elem_bytes /* NULL ok */,
                      const lig_derived_slot *d, uint64_t n, uint32_t *wave_out /* n entries or NULL */, lig_derived_info *info /* NULL ok */);
int lig_rows_set_derived(lig_trace *trace, const lig_linear_system *sys, const lig_derived_slot *d, uint64_t n, lig_derived_info *info /* NULL ok */);

/* ==== proof file framing (src/webgpu_prover.cpp:437-457 writes gzip(level 6) of the serialized envelope with
 * Boost.iostreams; src/webgpu_verifier.cpp:249-253 reads it back).  Host-only helpers on zlib: the output is a standard
 * gzip member that any gzip reader (the reference's gzip_decompressor included) accepts; compressed BYTES depend on the
 * zlib version and on Boost's header fields, so bit-exactness is defined on the uncompressed envelope. ==== */
size_t lig_proof_gzip_bound(size_t envelope_len);
int    lig_proof_gzip(const uint8_t *envelope, size_t len, uint8_t *out, size_t cap, size_t *out_len);
size_t lig_proof_gunzip_size(const uint8_t *gz, size_t len);           /* ISIZE trailer; 0 if not a gzip member */
int    lig_proof_gunzip(const uint8_t *gz, size_t len, uint8_t *out, size_t cap, size_t *out_len);

/* ==== one trace sharded over the GPUs of a node (configs[3]).  Rows are dealt to ranks block-cyclically
 * (global chunk g of <= 512 rows belongs to rank g mod world, chunks never split an x,y,z triple), so that after exchange
 * round c every rank holds the W consecutive global chunks cW .. cW+W-1 restricted to ITS columns: the column hash is
 * column-partitioned (rank h owns columns [h n/W, (h+1) n/W)) and absorbs the rows in global order while the next round
 * is still being encoded and exchanged.  One all-to-all of codeword column slices per round; leaves, partial stage-2 sums
 * (k + 2k + 2k values per rank, added mod p locally: RCCL has no modular reduction) and opened columns are all-gathered.
 * Every rank obtains the same envelope, byte-identical to lig_synth_prove of the same job.
 *
 * Collectives: lig_rccl_comm_create gives the RCCL communicator of the product (librccl over xGMI: grouped
 * ncclSend/ncclRecv and ncclAllGather enqueued on HIP streams of the context, nothing blocks the host).  The plain
 * callbacks exist so that tests can run the same sharded logic over gloo on CPU-staged buffers: they are called after
 * the context stream has been drained and must return 0 once the data is in place. ==== */
typedef struct lig_shard lig_shard;
/* A caller that fills in a lig_comm itself MUST zero the whole struct first (memset / = {0}): members may be appended (as
 * `forget` was), a non-NULL optional member is called.  lig_rccl_comm_create / lig_ipc_comm_create zero it themselves. */
typedef struct {
    void *user;
    /* rank g's `send` holds world blocks of block_bytes; block h goes to rank h; `recv` block g comes from rank g */
    int (*all_to_all)(void *user, const void *send_dev, void *recv_dev, size_t block_bytes);
    /* `recv` = world blocks of `bytes` in rank order */
    int (*all_gather)(void *user, const void *send_dev, void *recv_dev, size_t bytes);
    /* optional stream-ordered forms (NULL: not available): the collective is enqueued on `hip_stream`; the data is in
     * place for work enqueued on that stream afterwards */
    int (*all_to_all_on)(void *user, const void *send_dev, void *recv_dev, size_t block_bytes, void *hip_stream);
    int (*all_gather_on)(void *user, const void *send_dev, void *recv_dev, size_t bytes, void *hip_stream);
    /* optional (NULL: nothing to do): the caller is about to free device buffers it has passed as send buffers -- a
     * communicator that exports them to its peers (lig_ipc_comm_create) must not keep handles / mappings of a recycled
     * address.  Contract: call it before freeing any buffer that has been a `send_dev` (lig_shard_destroy does). */
    void (*forget)(void *user);
    /* optional (NULL: the communicator cannot tell): non-zero once the communicator has FAILED -- a peer died, left, or stopped
     * responding -- and the reason is in lig_last_error of its context.  A stream-ordered collective cannot return an error from
     * inside a queue: lig_shard_* asks this after it has drained its streams and returns LIG_E_STATE instead of an envelope made
     * of garbage.  lig_ipc_comm_create: watchdog thread (peer pids, an abort word, a stall timer; waits already queued are
     * released); lig_rccl_comm_create: ncclCommGetAsyncError. */
    int (*failed)(void *user);
    /* optional: make every collective already queued on this rank's streams give up NOW (ncclCommAbort; comm_ipc: poison).  lig_shard_*
     * calls it when queued work containing collectives has not completed LIG_COMM_TIMEOUT_S seconds (default 300) after the host
     * started to wait for it; the communicator is unusable afterwards (failed() != 0). */
    void (*abort)(void *user);
} lig_comm;
/* RCCL communicator: rank 0 calls lig_rccl_unique_id and hands the 128 bytes to every rank through the launcher's
 * rendezvous (torch.distributed / MPI / a file); every rank then calls lig_rccl_comm_create with its context. */
enum { LIG_RCCL_ID_BYTES = 128 };
int  lig_rccl_unique_id(uint8_t out[LIG_RCCL_ID_BYTES]);
int  lig_rccl_comm_create(lig_ctx *ctx, const uint8_t id[LIG_RCCL_ID_BYTES], uint32_t rank, uint32_t world, lig_comm *out);
void lig_rccl_comm_destroy(lig_comm *comm);               /* safe before or after lig_ctx_destroy of its context */
/* librccl is resolved on first use (the copy already mapped into the process wins, then the loader path, then /opt/rocm/lib;
 * LIG_RCCL_LIB overrides): LIG_OK and the library's path / ncclGetVersion, or LIG_E_STATE and the reason in path_out */
int  lig_rccl_available(char *path_out, size_t cap, int *version);
int  lig_rccl_comm_count(const lig_comm *comm, uint32_t *ranks);      /* ncclCommCount of a communicator made here */
/* A second communicator with stream-ordered forms, between processes that can map each other's device memory (same GPU, or
 * GPUs of one node with peer access): every rank pulls its blocks out of the peers' send buffers (hipIpcMemHandle), ordering is
 * done by the GPU on flags in the POSIX shared-memory segment `shm_name` ("/name"; rank 0 creates it, all ranks must pass the
 * same fresh name), no host thread waits for GPU work.  This is what the tests use to run the exchange pipeline of
 * lig_shard_prove with real peers on a one-GPU box (W processes on the device); world <= 16. */
int  lig_ipc_comm_create(lig_ctx *ctx, const char *shm_name, uint32_t rank, uint32_t world, lig_comm *out);
void lig_ipc_comm_destroy(lig_comm *comm);                /* collective: returns when every rank has left (or after 15 s) */
/* host only: the block-cyclic deal of a job's committed rows (masks excluded) for packing size l: *rounds exchange rounds,
 * world * rounds + 1 chunk boundaries (chunk g = rows [b[g], b[g+1]) belongs to rank g mod world).  LIG_E_NOMEM: cap too small. */
int  lig_shard_plan(const lig_synth_job *job, uint32_t l, uint32_t world, uint64_t *rounds, uint64_t *boundaries, size_t cap);
int  lig_shard_prepare(lig_ctx *ctx, const lig_synth_job *job, uint32_t rank, uint32_t world, const lig_comm *comm, lig_shard **out);
int  lig_shard_prove(lig_shard *shard, const uint8_t **proof, size_t *proof_len, lig_proof_info *info);
void lig_shard_destroy(lig_shard *shard);

/* ==== one trace sharded over the GPUs, rows SUPPLIED BY THE CALLER (configs[4]: a real constraint generator on N GPUs): what
 * lig_rows_* is to lig_synth_*.  Every rank passes the kinds of ALL committed rows -- the deal (lig_shard_rows_plan: global
 * chunk g belongs to rank g mod world) and the encoding-stream positions are global -- and the message rows of ITS OWN chunks
 * only, in commit order (job->rows = all rows, job->msgs = the local rows; dense_rands_per_row, if given, covers all rows).
 * lig_shard_rows_commit = stage 1 on all ranks (same root and seed everywhere); each rank's constraint generator then derives
 * the randomness rows of its own rows; lig_shard_rows_prove takes those (local rows x k, zero rows for batch kinds) and the
 * public linear constant (NULL: minus the sum of all inner products, as lig_rows_prove).  Every rank obtains the envelope of
 * lig_rows_prove on the whole trace.  Replaces the per-row callbacks of include/zkp/nonbatch_context.hpp:445-471, :654-780,
 * :924-970 when the rows of one trace live on several GPUs.
 * The narrow row format (job->elem_bytes, one byte per row of the WHOLE trace) is accepted: job->msgs then holds this rank's rows only,
 * packed back to back in commit order; they are uploaded to a staging buffer and expanded on the device before stage 1.
 * LIFETIME: the local rows passed to lig_shard_rows_begin / lig_shard_rows_restart (host or device memory) are copied before the call
 * returns; randomness rows passed to lig_shard_rows_prove are consumed before it returns.  (Only with LIG_SHARD_UPLOADER=1 -- the round-4
 * path through the library's uploader thread, off by default: profiles/r05_rows_entry_hang.md -- full-width host rows are read until
 * lig_shard_rows_commit has returned; narrow rows always take the synchronous copy.)
 * FAILURE: a peer that dies, leaves or stops responding makes these calls return LIG_E_STATE (lig_comm.failed / .abort), they do not hang:
 * every wait on the error paths and in lig_shard_destroy is a bounded poll.  If kernels queued behind the failed collective still have
 * not drained 20 s after the communicator was aborted, the error text says "poisoned": the shard refuses further calls, lig_shard_destroy
 * returns at once and keeps the device buffers (the queued kernels may still touch them), the rows / randomness rows handed to the failed
 * call must stay alive, and the context must not be reused -- tear the process down. ==== */
int lig_shard_rows_plan(const uint8_t *kinds, size_t n_rows, uint32_t world, uint64_t *rounds, uint64_t *boundaries, size_t cap);
int lig_shard_rows_begin(lig_ctx *ctx, const lig_rows_job *job, uint32_t rank, uint32_t world, const lig_comm *comm, lig_shard **out);
int lig_shard_rows_restart(lig_shard *shard, const void *local_msgs, int msgs_on_device);   /* next trace, same shape; after lig_shard_rows_prove of the previous one (LIG_E_STATE otherwise) */
int lig_shard_rows_commit(lig_shard *shard, uint8_t root[32], uint8_t stage1_seed[32]);
int lig_shard_rows_prove(lig_shard *shard, const void *local_rands, int rands_on_device, const uint8_t *const_sum,
                         const uint8_t **proof, size_t *proof_len, lig_proof_info *info);
/* Sparse linear constraints on a rows shard: what lig_rows_set_linear is on one GPU.  `sys` describes the WHOLE trace (slot = global row *
 * l + column, exactly what lig_rows_set_linear takes) and is copied before the call returns.  COLLECTIVE CONTRACT: every rank passes
 * the same system, as every rank passes the kinds of all rows; ranks that set different systems are not detected (they produce an
 * envelope that fails its own linear check, or differing envelopes).  A rank keeps only the terms whose row it was dealt, samples only the
 * stream elements those terms and its slice [rank n_rhs / world, (rank + 1) n_rhs / world) of the right-hand sides need, and forms
 * its local rows x k matrix on the device.  Any time after lig_shard_rows_begin and before lig_shard_rows_prove (before or after the
 * commit); survives lig_shard_rows_restart; a second call replaces it; sys == NULL removes it; freed by lig_shard_destroy.
 * With a system set, lig_shard_rows_prove(local_rands = NULL) uses the formed matrix; const_sum == NULL then means the system's
 * constant -sum_c b_c r_c: the ranks' shares travel as one more element of the all-gather of partial accumulators (5k + 1 elements
 * instead of 5k; a shard without a system sends what it always sent), are added in rank order and negated on every rank; it is
 * returned in info->const_sum, identical on every rank, and info->valid_linear is a real check.  A non-NULL const_sum is used as given.
 * LIG_E_ARG: a system lig_linear_check rejects (nothing is launched), a job with dense_rands_per_row, local_rands != NULL in
 * lig_shard_rows_prove while a system is set.  LIG_E_STATE: a shard not made by lig_shard_rows_begin, a poisoned shard. */
int lig_shard_rows_set_linear(lig_shard *shard, const lig_linear_system *sys);
/* Per-proof VALUES of the coefficient table of the system set with lig_shard_rows_set_linear: what lig_rows_set_linear_values is on one
 * GPU.  coefs[] with the system's n_coefs, canonical -- the public right-hand sides b_c of a new statement are the entries named by
 * rhs_coef.  The values belong to the rank's attachment and stay in force over lig_shard_rows_restart until set again (a second
 * lig_shard_rows_set_linear drops them with the structure); coefs == NULL: back to the system's own table.  Copied before the call
 * returns; converted on the device, on the stream the rank's form runs on.  Nothing is re-checked, re-uploaded or regrouped: the call
 * costs one pass over n_coefs entries on the host and one small kernel, whatever the size of the system.
 * COLLECTIVE CONTRACT as lig_shard_rows_set_linear: every rank passes the same table; ranks that differ are not detected (they produce
 * an envelope that fails its own linear check, or differing envelopes).  No collective is involved: the call never waits for a peer.
 * With values set, lig_shard_rows_prove(local_rands = NULL, const_sum = NULL) proves that statement: info->const_sum and the envelope are
 * those of a shard whose system was set with these values as sys->coefs.
 * Any time after lig_shard_rows_set_linear and before lig_shard_rows_prove.  ERRORS, decided on the host before anything is launched:
 * LIG_E_ARG: a NULL shard, another n_coefs, an entry >= p; LIG_E_STATE: no system set, a shard not made by lig_shard_rows_begin, a
 * poisoned shard.  A refused call leaves the values in force as they were.  Device memory: n_coefs x 32 on top of the attachment. */
int lig_shard_rows_set_linear_values(lig_shard *shard, const uint8_t *coefs, uint64_t n_coefs);
/* of the system set last: the terms this rank kept and the distinct stream elements it samples per proof (LIG_E_STATE: no system set) */
int lig_shard_rows_linear_stats(const lig_shard *shard, uint64_t *local_terms, uint64_t *sampled_constraints);
/* host only, no context: the same two numbers for `rank` of `world` from the deal of lig_shard_rows_plan -- to size a node before a
 * GPU is touched.  LIG_E_ARG: world == 0, rank >= world, a system lig_linear_check rejects. */
int lig_linear_shard_count(const lig_linear_system *sys, const uint8_t *kinds, uint64_t rows, uint32_t l, uint32_t rank, uint32_t world,
                           uint64_t *local_terms, uint64_t *needed_constraints);
/* Derived slots on a rows shard: what lig_rows_set_derived is on one GPU (csrc/derive.hip, csrc/derive_plan.hpp).  `sys` and `d` describe
 * the WHOLE trace with global slots, exactly what lig_rows_set_derived takes.  COLLECTIVE CONTRACT as lig_shard_rows_set_linear: every
 * rank passes the same system and the same list -- the exchange schedule is computed from them on every rank; ranks that differ are not
 * detected (their all-gathers disagree in size, or they commit different rows).  The call itself issues NO collective and never waits
 * for a peer.  Accepted and refused lists are those of lig_derived_check against the kinds and widths of all rows of the job (LIG_E_ARG:
 * nothing launched, no collective, the previous list stays in force); LIG_E_STATE: a shard not made by lig_shard_rows_begin, a poisoned
 * shard; LIG_E_ARG: info->struct_bytes too small.  Copies what it needs before it returns; survives lig_shard_rows_restart; a second call
 * replaces the list; d == NULL or n == 0 removes it; lig_shard_rows_set_linear_values does not reach it; freed by lig_shard_destroy.
 *   A target is formed by the rank that was dealt its row, wave by wave (the waves of lig_derived_check, numbered over the whole list).
 *   Its other terms are LOCAL (on a row of the same rank) or IMPORTED (on a row of another rank, possibly derived there in an earlier
 *   wave).  Per wave w every rank q sends E_q(w) = the distinct slots it holds that a wave-w target of ANOTHER rank reads and that no
 *   earlier wave has sent, ascending: one all-gather of B(w) = max_q |E_q(w)| elements per rank, into an import buffer that is
 *   addressed absolutely over the commit.  A wave with B(w) = 0 issues no collective, on every rank alike: a list whose constraints are
 *   row-local (a machine word recomposed from bits of its own row) exchanges nothing.  Field addition is exact: the regrouped sum gives
 *   the bytes of lig_rows_set_derived.
 *   A product entry (LIG_DERIVED_PRODUCT) is formed by the rank that holds its row: the deal never splits a triple, so both operands are
 *   local and it never imports.  A re-formed slot that a target of another rank reads is sent in the first wave that reads it across
 *   ranks, a later wave than its own.  local_targets counts it, local_terms counts it as 2.
 *   WHERE  in lig_shard_rows_commit, on the main stream, before the first round's encode: per wave the export kernel and the all-gather
 *          (both only when B(w) > 0), then the wave kernel, which stores into the rank's local rows; the pads are not touched.  A failed
 *          collective takes the path of every other collective of the commit (LIG_E_STATE, possibly a poisoned shard).  Host rows that
 *          arrive round by round (LIG_SHARD_UPLOADER=1): every round's arrival is waited for first -- such a trace gives up the upload /
 *          encode overlap.  Without a list the commit queues exactly what it queued before.
 *   READERS see the derived values: lig_shard_rows_read_slots, lig_shard_rows_diagnose*, lig_shard_rows_explain*,
 *          lig_shard_rows_explain_slots*, lig_shard_rows_untouched_slots*, stage 2.
 * *info (or NULL; struct_bytes set by the caller): n_slots, n_terms, n_waves of the whole list; n_exchanges = waves with an all-gather;
 * of THIS rank: local_targets, local_terms + imported_terms (the other terms of its targets), imports = distinct foreign slots its
 * targets read, exports = slots it sends, exchange_bytes = 32 * world * sum_w B(w), the bytes it receives per commit.
 * lig_derived_shard_count: host only, no context, no shard: the same numbers for `rank` of `world` from the deal of lig_shard_rows_plan
 * (LIG_E_ARG also for world == 0, rank >= world, a NULL info).
 * Not done: sharing one plan between the ranks of a process; detecting ranks that pass different lists. */
typedef struct { uint32_t struct_bytes, reserved;
                 uint64_t n_slots, n_terms; uint32_t n_waves, n_exchanges;   /* whole list; waves that need an all-gather */
                 uint64_t local_targets, local_terms, imported_terms,        /* this rank */
                          imports, exports, exchange_bytes;                  /* distinct foreign slots read / own slots sent; bytes this rank receives per commit */
               } lig_derived_shard_info;                                                                            /* 80 bytes */
int lig_derived_shard_count(const lig_linear_system *sys, const uint8_t *kinds, uint64_t rows, uint32_t l, const uint8_t *elem_bytes /* NULL ok */,
                            const lig_derived_slot *d, uint64_t n, uint32_t rank, uint32_t world, lig_derived_shard_info *info);
int lig_shard_rows_set_derived(lig_shard *shard, const lig_linear_system *sys, const lig_derived_slot *d, uint64_t n, lig_derived_shard_info *info /* NULL ok */);

/* lig_rows_diagnose on a rows shard (csrc/diagnose.hip, csrc/shard.hip).  COLLECTIVE: every rank calls it with the same `sys` -- the system
 * of the WHOLE trace, global slots, as lig_shard_rows_set_linear takes it -- and the same caps.  EVERY RANK RETURNS THE SAME BYTES, and
 * they are exactly what lig_rows_diagnose returns for the whole trace on one GPU: lig_diag_linear records in ascending constraint number,
 * lig_diag_quad records in ascending (term in commit order, column) with GLOBAL row numbers, counts that cover all violations, a cap of
 * 0 for counts only.  sys == NULL: the quadratic part only.  sys->coefs is used as passed; the system set with
 * lig_shard_rows_set_linear is neither read nor written.
 * HOW: linear constraints go in slices of LIG_DIAG_SLICE constraints (default 2^22).  Per slice every rank sums a * w over the terms
 * whose row it holds (a rank without rows: zeros), ONE all-to-all sends the partials of sub-block h of the slice to rank h, which adds
 * the W partials, subtracts b_c and keeps its first lin_cap violations; counts and records are all-gathered in blocks of a fixed size and
 * merged on the host of every rank.  A quadratic term never spans ranks (the deal does not split a triple or a pair): each rank
 * evaluates its own, keeps its first quad_cap violations with the terms' global ordinals, and the blocks are all-gathered and merged by
 * (ordinal, column).  Arithmetic is exact and no atomic decides an order or a count: the same bytes on every run.  Whether a collective
 * is issued, how many and of which size depends on the sizes in sys, the caps, world and the slice size alone -- never on what a rank
 * holds.  world == 1: no collective at all (unless LIG_SHARD_FORCE_EXCHANGE is set), the call is lig_rows_diagnose.
 * WHEN: from the return of lig_shard_rows_commit until the next lig_shard_rows_restart, before or after lig_shard_rows_prove; the
 * envelope of a diagnosed shard is byte-identical to that of one that was not.
 * ERRORS, all decided on the host, identically on every rank, before any launch and any collective: LIG_E_ARG for a system
 * lig_linear_check rejects, a NULL array with a cap > 0, a short info->struct_bytes; LIG_E_STATE before the commit, for a shard not made
 * by lig_shard_rows_begin, for a poisoned shard.  FAILURE of a peer or of the communicator: as every lig_shard_* call (bounded polls,
 * lig_comm.failed after the streams have drained, lig_comm.abort after LIG_COMM_TIMEOUT_S, poisoning).
 * SCRATCH is allocated inside the call and freed before it returns (lig_comm.forget runs first; every send buffer is an allocation of
 * its own); the work runs on the context's main stream.  With S = min(LIG_DIAG_SLICE, n_constraints) rounded to a multiple of W, B = S / W
 * and T = the quadratic terms of the whole trace, a rank allocates at most
 *     64 S + 40 B + 8 (B + 1)  +  (W + 1) (16 + 40 min(lin_cap, n_constraints))  +  (W + 1) (16 + 52 min(quad_cap, T l))  bytes
 * plus what lig_rows_diagnose allocates whatever the witness: the uploaded system (8 n_terms + 8 n_constraints + 8 n_rhs + 32 n_coefs),
 * 4 bytes per row of the trace, 40 bytes per item of a quadratic slice (2^20 items) and the scan's temporary storage.
 * Not done: skipping the exchange for constraints whose terms all lie on one rank (it would make the schedule depend on the data). */
int lig_shard_rows_diagnose(lig_shard *shard, const lig_linear_system *sys, lig_diag_linear *lin_out, uint64_t lin_cap,
                            lig_diag_quad *quad_out, uint64_t quad_cap, lig_diag_info *info);
/* lig_shard_rows_diagnose against the system ATTACHED to the shard (lig_shard_rows_set_linear), with the values of
 * lig_shard_rows_set_linear_values in force: the statement lig_shard_rows_prove(local_rands = NULL, const_sum = NULL) would prove.  What
 * lig_rows_diagnose_attached is on one GPU: for the caller who has released the term list, and the only call that needs no hand-passed
 * "table of THIS statement".  COLLECTIVE: every rank calls it with the same caps.  EVERY RANK RETURNS THE SAME BYTES, and they are what
 * lig_shard_rows_diagnose -- and hence lig_rows_diagnose on the whole trace -- returns for the same statement.  Window, caps, *info, the
 * quadratic part, failure and poisoning rules are exactly those of lig_shard_rows_diagnose; whether a collective is issued, how many and
 * of which size depends on the system's sizes, the caps, world and the slice size alone.
 * HOW: a rank holds the slot-major index of its own rows with constraints numbered compactly through its need list, its slice of the
 * right-hand sides and the table in force -- all on its device.  The call regroups the index by compact constraint there (count, scan,
 * scatter, as lig_rows_diagnose_attached; the atomics only place a term inside its segment, the sums are exact).  The need list is
 * ascending, so a slice of LIG_DIAG_SLICE constraints of the whole trace is a contiguous compact range: the send buffer is zeroed, one lane
 * per compact constraint of the range (one workgroup and the fixed tree for one with more than 2048 local terms) sums a * w over its
 * local terms and -- a right-hand side has exactly one holder -- subtracts b_c when this rank holds it.  The owner of a sub-block then
 * only adds the W partials: the sum is the residual, exact and independent of rank order.  A constraint with a right-hand side and no
 * term anywhere comes out as -b_c, as on one GPU.  Everything behind the reduce is lig_shard_rows_diagnose.  No host pass over the terms,
 * no upload of the system; the table in force is read in place, behind an event when its conversion is still running on the side stream.
 * world == 1 without LIG_SHARD_FORCE_EXCHANGE: no collective, the call is lig_rows_diagnose_attached on the rank's matrix.
 * ERRORS, all decided on the host, identically on every rank, before any launch and any collective: LIG_E_ARG for a NULL shard, a NULL
 * array with a cap > 0, a NULL or short *info; LIG_E_STATE when no system is set, before the commit, for a shard not made by
 * lig_shard_rows_begin, for a poisoned shard.
 * SCRATCH lives for the call only, on the context's main stream (lig_comm.forget runs before any send buffer is freed); nothing the
 * attachment owns is written, and the envelope of a shard diagnosed this way is byte-identical to that of one that was not.  In the
 * formula of lig_shard_rows_diagnose the uploaded system is replaced by 8 bytes per local term, 12 per needed constraint and 4 per slice.
 * The terms, coefficients and witness values of the constraints it names: lig_shard_rows_explain_attached below.
 * Not done: sharing a prepared program between ranks, caching the regrouped list between calls. */
int lig_shard_rows_diagnose_attached(lig_shard *shard, lig_diag_linear *lin_out, uint64_t lin_cap, lig_diag_quad *quad_out,
                                     uint64_t quad_cap, lig_diag_info *info);

/* lig_rows_explain / lig_rows_read_slots on a rows shard (csrc/diagnose.hip, csrc/shard.hip).  lig_shard_rows_diagnose hands every rank
 * a constraint number and 32 residual bytes; a constraint may span ranks and no process holds the witness: the value of a term on a
 * derived QZ row or on a record slot of a mixed row exists only on the device of the rank that was dealt that row.
 * COLLECTIVE: every rank passes the same `sys` (the term list of the WHOLE trace with global slots, exactly what
 * lig_shard_rows_diagnose takes), the same asked list, the same term_cap, the same `slots`.  Slots are global: row * l + column over
 * the committed rows of the whole trace, of any kind.  EVERY RANK RECEIVES THE SAME BYTES, and they are the bytes of
 * lig_rows_explain(trace, sys, ...) / lig_rows_read_slots(trace, ...) on a one-GPU trace of the same rows: order, first_term, n_terms,
 * rhs, residual, coefficient values, value, reserved fields zero, info->n_terms_total and n_terms_reported.  info->ms_total is the
 * rank's own.
 * WHEN: the window of lig_shard_rows_diagnose -- from the return of lig_shard_rows_commit until the next lig_shard_rows_restart, before
 * or after lig_shard_rows_prove; LIG_E_STATE outside it, for a shard not made by lig_shard_rows_begin, for a poisoned shard.  Nothing a
 * proof depends on is written: the envelope of a shard that was explained or read is byte-identical to that of one that was not.
 * REFUSALS happen on the host, before any launch and any collective, and are decided identically on every rank, so a refused call
 * leaves the shard usable and no peer waiting.  LIG_E_ARG: sys == NULL or a sys lig_linear_check rejects; an asked list that is not
 * strictly ascending or names a constraint >= n_constraints; a slot >= rows * l of the whole trace; a NULL array with a non-zero
 * count (constraints, con_out with n_asked > 0; terms_out with term_cap > 0; slots, values with n_slots > 0); a NULL or short *info.
 * n_asked == 0 or n_slots == 0: LIG_OK, no launch, no collective.
 * world == 1 without LIG_SHARD_FORCE_EXCHANGE: no collective, the call is lig_rows_explain / lig_rows_read_slots on the rank's matrix;
 * with the knob set the exchange path runs with one rank.
 * HOW: the asked segments are on the host of every rank already: the m = sum of n_terms items are formed and put into the output order
 * there (no gather kernel, no copy back, and the system is NOT uploaded: only the m ordered terms, first_term[], the asked list, one
 * right-hand-side coefficient index per asked constraint and the coefficient table).  The values cross the ranks in pieces of
 * P = min(m, LIG_DIAG_SLICE) terms (the last piece ragged): a rank writes the canonical w of the terms whose row it holds and zero for
 * the others (a rank without rows: zeros), ONE all-gather of 32 P bytes per rank and piece (the tail of the last piece zeroed: the size is
 * fixed), and every rank adds the W received values -- a row has one owner, so exactly one summand is non-zero and the sum is exact and
 * independent of rank order.  The records are then filled and the residuals summed by the kernels of lig_rows_explain over the value
 * list (fixed tree, one workgroup per asked constraint, whatever its length).  con_out is complete whatever term_cap is, so all m values
 * are exchanged.  lig_shard_rows_read_slots runs the same exchange over the slot list in pieces of min(n_slots, LIG_DIAG_SLICE).
 * Whether a collective is issued, how many and of which size depends on m (or n_slots), world and the piece size alone -- never on
 * which rows a rank holds.  FAILURE of a peer or of the communicator: as lig_shard_rows_diagnose.
 * SCRATCH is allocated inside the call and freed before it returns (lig_comm.forget runs first; every send buffer is an allocation of
 * its own); the work runs on the context's main stream.  explain: 32 P (send) + 32 W P (receive) + 32 m (values) + 8 m (ordered
 * terms) + 32 n_coefs + 16 n_asked + 4 bytes per row of the trace, and the records, 88 n_asked + 84 min(m, term_cap); read_slots:
 * 68 P + 32 W P + 4 bytes per row of the trace.
 * The caller who has released the term list: lig_shard_rows_explain_attached below.  Not done: an all-to-all, reduce and all-gather
 * instead of the all-gather, which would halve the bytes (the calls are for short lists). */
int lig_shard_rows_explain(lig_shard *shard, const lig_linear_system *sys, const uint32_t *constraints, uint64_t n_asked,
                           lig_explain_constraint *con_out, lig_explain_term *terms_out, uint64_t term_cap, lig_explain_info *info);
int lig_shard_rows_read_slots(lig_shard *shard, const uint32_t *slots, uint64_t n_slots, uint8_t *values /* n_slots x 32 */);
/* lig_shard_rows_explain against the system ATTACHED to the shard (lig_shard_rows_set_linear), with the values of
 * lig_shard_rows_set_linear_values in force if any: the statement lig_shard_rows_prove(local_rands = NULL, const_sum = NULL) would
 * prove.  What lig_rows_explain_attached is on one GPU: no term list on any rank, no hand-passed "table of THIS statement"; a table still
 * converting on the side stream is waited for with its event, not with a device-wide synchronise.
 * COLLECTIVE: every rank passes the same asked list and the same term_cap.  EVERY RANK RECEIVES THE SAME BYTES, and they are exactly what
 * lig_shard_rows_explain returns for the term list of that system under the table in force -- and hence what lig_rows_explain_attached
 * returns on a one-GPU trace of the same rows: order (ascending asked constraint, slot, coef_index as an unsigned number), first_term,
 * n_terms, rhs, residual, coefficient values, witness values, reserved fields zero, n_terms_total, n_terms_reported.  A term the system
 * holds twice appears twice; a constraint with a right-hand side and no term anywhere has n_terms = 0 and residual -b_c; con_out is
 * complete whatever term_cap is.  info->ms_total is the rank's own.
 * WINDOW, FAILURE, POISONING as lig_shard_rows_explain: from the return of lig_shard_rows_commit until the next lig_shard_rows_restart,
 * before or after the proof; nothing a proof, the attachment or the table depends on is written (the envelope of an explained shard is
 * byte-identical to that of one that was not).
 * REFUSALS are decided on the host, identically on every rank, before any launch and any collective.  LIG_E_ARG: a NULL shard; a NULL or
 * short *info; constraints or con_out NULL with n_asked > 0; terms_out NULL with term_cap > 0; an asked list that is not strictly
 * ascending or names a constraint >= the system's n_constraints.  LIG_E_STATE: no system set, before the commit, a shard not made by
 * lig_shard_rows_begin, a poisoned shard.  n_asked == 0: LIG_OK, no launch, no collective.
 * HOW: a rank keeps exactly the terms whose row it was dealt, so the value of every term it holds is in its own local matrix and no value
 * is requested from a peer.
 *   1. select, on every rank's device: one lane per entry of the rank's slot-major index marks the entries whose constraint is asked (the
 *      compact number through the need list, then a binary search over the ascending asked list), a scan of the marks, and a collect
 *      without atomics into 48-byte records {position in the asked list, slot of the WHOLE trace, coef_index, valid = 1, the canonical
 *      committed w}: the local slot goes through the rank's local-row -> global-row table, the value comes from the local matrix.  The
 *      rank's count m_r comes back with the scan.
 *   2. ONE header all-gather whose size n_asked alone fixes (16 + 8 n_asked bytes per rank, n_asked rounded up to even): m_r, and per
 *      asked constraint whether this rank's slice of the right-hand sides holds its b_c and under which coefficient index -- two fields,
 *      LIG_COEF_ONE being 0xFFFFFFFF; a right-hand side has exactly one holder.  Afterwards every rank knows every m_r.
 *   3. with M = max m_r and P = min(M, LIG_DIAG_SLICE): ceil(M / P) all-gathers of 48 P bytes per rank; a rank's block beyond its own m_r
 *      is zeroed (valid = 0).  M = 0: none.
 *   4. every rank holds all sum m_r records: the 12-byte heads are put into the output order on the host (a total order: the result
 *      depends neither on rank order nor on the order inside a block), a kernel permutes the values, which never left the device, into
 *      that order, and the fill and finish kernels of lig_shard_rows_explain write the records, b_c from the header, the table in force
 *      read in place.
 * A collective's schedule never depends on a rank's OWN share.  Step 3 is the one place where the NUMBER of collectives depends on what the
 * ranks hold -- but only through the m_r every rank received in step 2, so every rank issues the same schedule.  A malformed block (a
 * record that names no asked constraint, counts that do not add up, two holders of one b_c, sum m_r >= 2^32) is LIG_E_STATE, never an
 * index.
 * world == 1 without LIG_SHARD_FORCE_EXCHANGE: no collective -- the same passes over the rank's share, which is compactly numbered
 * through its need list all the same, with a device copy in place of every all-gather; with the knob set the exchange path runs with one
 * rank.
 * SCRATCH lives for the call only, on the context's main stream (every send buffer is an allocation of its own, lig_comm.forget runs
 * before any of them is freed, and the scratch is abandoned when the shard is poisoned).  With T = the rank's local terms, S = sum m_r,
 * J = ceil(M / P):  8 (T + 1) marks and positions and the scan's temporary storage, 48 m_r collected records, (W + 1) header blocks,
 * 48 P (send) + 48 W P (receive), 16 J W P heads for the host's walk, 36 S unordered values and permutation, 44 S ordered terms, asked
 * positions and values, 4 bytes per local row, 8 W + 16 n_asked, and the records, 88 n_asked + 84 min(S, term_cap). */
int lig_shard_rows_explain_attached(lig_shard *shard, const uint32_t *constraints, uint64_t n_asked,
                                    lig_explain_constraint *con_out, lig_explain_term *terms_out, uint64_t term_cap, lig_explain_info *info);
/* lig_rows_explain_slots* / lig_rows_untouched_slots* on a rows shard: from a suspect SLOT to the other constraints through it, and the
 * witness slots no term touches.  No host can answer either: the terms of a slot lie in the share of the one rank that was dealt its row,
 * numbered compactly through that rank's need list, and the residuals of those constraints span ranks.
 * SLOTS ARE GLOBAL: row * l + column over the committed rows of the WHOLE trace; the asked list is strictly ascending.
 * COLLECTIVE: every rank passes the same arguments.  EVERY RANK RECEIVES THE SAME BYTES, and they are what
 * lig_rows_explain_slots_attached / lig_rows_untouched_slots_attached return on a one-GPU trace of the same rows under the same system
 * and the table in force: order and first_term, n_terms, constraint_terms, constraint numbers of the whole trace, coefficient values,
 * residuals, value and row_kind, every count in *info.  info->ms_total is the rank's own.
 * The _attached forms use the share lig_shard_rows_set_linear attached, with the values of lig_shard_rows_set_linear_values in force (a
 * conversion still running on the side stream is waited for with its event).  The forms with `sys` (the term list of the WHOLE trace, the
 * same on every rank) run lig_linear_check, make a temporary share of it on every rank (what lig_shard_rows_set_linear makes: 8 bytes per
 * kept term + 4 per local slot and needed constraint, and as much again in scratch), run the attached path on it -- one code path -- and
 * destroy it before they return; what is attached to the shard is then neither read nor modified.  For the same statement both forms
 * return the same bytes.
 * WINDOW, FAILURE, POISONING exactly as lig_shard_rows_explain_attached: from the return of lig_shard_rows_commit until the next
 * lig_shard_rows_restart, before or after the proof; the envelope of a shard that was asked is byte-identical to that of one that was not;
 * nothing the attachment owns is written.
 * REFUSALS are decided on the host, identically on every rank, before any launch and any collective.  LIG_E_ARG: a NULL shard; a NULL or
 * short *info; slots or slot_out NULL with n_asked > 0, terms_out NULL with term_cap > 0, out NULL with cap > 0; slots not strictly
 * ascending; a slot >= rows * l of the whole trace; on the forms with `sys`, a NULL sys or one lig_linear_check rejects.  LIG_E_STATE: no
 * system set (the _attached forms), before the commit or after the restart, a shard not made by lig_shard_rows_begin, a poisoned shard.
 * n_asked == 0: LIG_OK, no launch, no collective.
 * HOW, lig_shard_rows_explain_slots*:
 *   1. host: every asked slot's row goes through the rank's global -> local row table; the rank keeps the asked indices whose row it was
 *      dealt, with their LOCAL slot numbers (ascending: local rows are in commit order).
 *   2. device, over that sub-list: the segment lengths of the rank's own slot-major index, an exclusive scan, and a collect into 16-byte
 *      items {index in the asked list, constraint OF THE WHOLE TRACE (through the need list), coef_index, valid = 1}, one 16-byte store
 *      each -- one lane per item, a whole workgroup for a slot with more than 2048 terms (every term through a slot lies on its owner);
 *      the values with the gather of lig_rows_read_slots on the local matrix.  No atomic.
 *   3. ONE header all-gather whose size n_asked alone fixes (16 + 48 n_asked bytes per rank): m_r, and per asked slot {held, n_terms,
 *      value}.  A slot has exactly one holder; presence is a field of its own, never inferred from a zero value.
 *   4. with M = max m_r and P = min(M, LIG_DIAG_SLICE): ceil(M / P) all-gathers of 16 P bytes per rank; a rank's block beyond its own m_r
 *      is zeroed (valid = 0).  As in lig_shard_rows_explain_attached the NUMBER of collectives depends on what the ranks hold only through
 *      the m_r every rank has received.
 *   5. the host of every rank walks the items (a valid item past m_r, an index >= n_asked, an item for a slot another rank holds, a slot
 *      with two holders or none, counts that do not add up: LIG_E_STATE, never an index), puts them into the output order and takes the
 *      distinct constraints in ascending order.
 *   6. their sizes and residuals come from lig_shard_rows_explain_attached ITSELF, asked for the constraint records alone (term_cap = 0)
 *      after every collective of steps 3 and 4 is complete: one evaluator, as on one GPU.  The list is the same on every rank, so its
 *      collective schedule is too; with no term on any asked slot there is no such call on any rank.
 *   7. the fill kernel of lig_rows_explain_slots writes the records with the table in force, read in place behind its event.
 * HOW, lig_shard_rows_untouched_slots*: every rank runs the flag / scan / compact passes of the one-GPU call over its LOCAL LINEAR .. QZ
 * rows against its local index in slices of 2^22 slots, writes the slot numbers of the WHOLE trace and keeps its first
 * min(cap, selected) records on the device.  ONE header all-gather of 32 bytes {n_untouched, n_untouched_nonzero, kept, 0}, then, with
 * M = max kept and P = min(M, LIG_DIAG_SLICE), ceil(M / P) all-gathers of 40 P bytes per rank.  The host merges the W ascending lists by
 * slot and cuts at cap: the first cap of all are among each rank's first cap, so the cut is exact.  The counts are sums over ranks and
 * complete whatever cap is.
 * world == 1 without LIG_SHARD_FORCE_EXCHANGE: the same passes with a device copy in place of every all-gather, no collective (the
 * one-GPU call cannot serve: the share is compactly numbered); with the knob set the exchange path runs with one rank.
 * SCRATCH lives for the call only, on the context's main stream (every send buffer is an allocation of its own, lig_comm.forget runs
 * before any of them is freed, and the scratch is abandoned when the shard is poisoned).  Explain, with H = the asked slots the rank
 * holds, S = sum m_r, J = ceil(M / P), D = the distinct constraints: 56 H + 4 n_asked, (W + 1) (16 + 48 n_asked) for the headers, 16 m_r
 * collected items, 16 P (send) + 16 W P (receive) + 16 J W P for the host's walk, 88 D + 96 min(S, term_cap) for the records, and -- while
 * it runs -- the scratch of lig_shard_rows_explain_attached for D asked constraints.  Untouched: 16 bytes per local LINEAR .. QZ row, 16
 * per slot of a slice, 40 kept, 32 (W + 1), 40 P (send) + 40 W P (receive) + 40 J W P. */
int lig_shard_rows_explain_slots_attached(lig_shard *shard, const uint32_t *slots, uint64_t n_asked,
                                          lig_slot_record *slot_out, lig_slot_term *terms_out, uint64_t term_cap, lig_slot_info *info);
int lig_shard_rows_explain_slots(lig_shard *shard, const lig_linear_system *sys, const uint32_t *slots, uint64_t n_asked,
                                 lig_slot_record *slot_out, lig_slot_term *terms_out, uint64_t term_cap, lig_slot_info *info);
int lig_shard_rows_untouched_slots_attached(lig_shard *shard, int nonzero_only, lig_slot_value *out, uint64_t cap, lig_untouched_info *info);
int lig_shard_rows_untouched_slots(lig_shard *shard, const lig_linear_system *sys, int nonzero_only, lig_slot_value *out, uint64_t cap,
                                   lig_untouched_info *info);

/* sizeof of the public structs as this build of the library sees them, in the order {lig_batch_op, lig_synth_job, lig_proof_info,
 * lig_verify_info, lig_rows_job, lig_comm}: a binding in another language (ctypes, cgo, JNI) checks its own layouts against these at
 * load time -- members are appended to these structs over time and a short struct on the caller's side is read past its end. */
enum { LIG_ABI_STRUCTS = 6 };
void lig_abi_sizes(uint32_t out[LIG_ABI_STRUCTS]);

/* Measurement hook (no reference counterpart): while enabled, every lig_encode_rows launch group records HIP
 * events on the context stream immediately around the dominant kernel (k_encode_tiles).  lig_profile_read syncs
 * and returns the number of bracketed launches, the rows they covered and the summed kernel time. */
int lig_profile_enable(lig_ctx *ctx, int on);
int lig_profile_read(lig_ctx *ctx, uint64_t *launches, uint64_t *rows, double *total_ms);
/* the same restricted to the bracketed launches of exactly rows_in_launch rows (512 = the full chunks: what a rocprofv3 kernel table
 * lists per launch size).  rows_in_launch = 0: the derive waves of lig_rows_commit on a trace with a list of derived slots
 * (lig_rows_set_derived), one bracket per commit around all its waves -- with such a list set, lig_profile_read's sum includes them. */
int lig_profile_read_launches(lig_ctx *ctx, uint32_t rows_in_launch, uint64_t *launches, double *total_ms);

#ifdef __cplusplus
}
#endif
#endif /* LIG_HIP_H */
