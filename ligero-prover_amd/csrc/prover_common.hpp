// prover_common.hpp -- host-side helpers shared by the prover, the sharded prover and the verifier: transcript hashing
// and samplers (OpenSSL), the instance hash, the stage-1 seed, the coefficient draws and the self-check of stage 2, column
// sampling, Merkle decommitment, the protobuf envelope writer and the row plan of a synthetic job.  The rules of a ROWS job (kinds,
// narrow format) are in rows_plan.hpp, those of bringing caller rows from host memory (upload jobs, flag words) in upload_plan.hpp, both
// host only; the uploader thread is behind upload.hpp.  Everything here is internal to liblig_hip.so.
#pragma once
#include <openssl/evp.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "ctx_internal.hpp"
#include "fr29.hpp"
#include "host_field.hpp"
#include "rows_plan.hpp"
#include "upload_plan.hpp"

namespace H = lig::host;

namespace lig {
void launch_rng_fill_rows(hipStream_t s, const uint32_t* rk60_dev, uint64_t first, fr* out, size_t rows, uint32_t per_row,
                          size_t row_stride, uint32_t col_off, uint32_t elem_stride, uint64_t stream_stride);
void launch_rlc_rows29(hipStream_t s, const fr* U, size_t urs, uint32_t ues, const fr* Rn, size_t rrs, size_t rows, uint32_t count,
                       const f29s* rc_dev, fr* code, fr* lin, fr* part_code, fr* part_lin, uint32_t group_rows);
void launch_quad_rows29(hipStream_t s, const fr* U, size_t urs, uint32_t ues, uint32_t count, const uint32_t* triples_dev,
                        const f29s* rq2, const f29s* rq1, size_t n_triples, fr* quad, fr* part = nullptr, size_t part_elems = 0);
void launch_quad_rows29_view(hipStream_t s, CwView cw, uint32_t count, const uint32_t* triples_dev, const f29s* rq2, const f29s* rq1,
                             size_t n_triples, fr* quad, fr* part = nullptr, size_t part_elems = 0);
void launch_sum_elems(hipStream_t s, const fr* in, uint32_t count, uint32_t stride, fr* out, fr* neg_out);
void launch_rlc_accumulate29(hipStream_t s, const fr* U, size_t urs, uint32_t ues, const fr* Rn, size_t rrs, size_t rows, uint32_t count,
                             const f29s* rc_dev, fr* part_code, fr* part_lin, uint32_t group_rows);
void launch_rng_fill_rows_dense(hipStream_t s, const uint32_t* rk60_dev, uint64_t first, fr* out, size_t rows, uint32_t per_row, uint32_t k);
void launch_rand_rlc(hipStream_t s, const uint32_t* rk60_dev, uint64_t first, fr* out, const fr* msgs, size_t rows, uint32_t per_row, uint32_t k,
                     const f29s* rc_dev, uint32_t group_rows, fr* code_part, fr* lin_part);
void launch_lin_interleave(hipStream_t s, fr* out, const fr* accH, const fr* accC, uint32_t k);
void launch_rlc_combine(hipStream_t s, fr* acc, const fr* part, uint32_t groups, uint32_t count);
void launch_copy_from_host(hipStream_t s, uint8_t* dst_dev, const uint8_t* src_mapped, size_t bytes);
// narrow caller rows (lig_rows_job.elem_bytes, expand.hip): rows [first_row, first_row + rows) of the packed matrix -- row r at
// packed + off_dev[r], width widths_dev[r] -- into out + r * k, full width; slots l..k-1 of a narrow row are zeroed.
// prod_rows_dev[0 .. n_prod): the derived rows (LIG_ELEM_PRODUCT) among them, ascending row indices -- formed from the packed
// sources of the two rows in front of each (which may lie before first_row: they only have to be in `packed`)
// wd: the mixed rows (lig_rows_job.wide_per_row) among them -- mixed_rows_dev[0 .. n_mixed) ascending row indices, wide_dev[r] = the
// records of row r (every row of the matrix; NULL: the matrix has no mixed row), max_records = the largest count, flag_dev = one
// word that a record with a column >= l raises.  n_mixed == 0: nothing more is launched than without the member.
struct WideArgs { const uint32_t* mixed_rows_dev = nullptr; size_t n_mixed = 0; const uint32_t* wide_dev = nullptr; uint32_t max_records = 0; uint32_t* flag_dev = nullptr; };
void launch_expand_rows(hipStream_t s, const uint8_t* packed, const uint64_t* off_dev, const uint8_t* widths_dev, size_t first_row,
                        size_t rows, uint32_t l, uint32_t k, fr* out, const uint32_t* prod_rows_dev = nullptr, size_t n_prod = 0,
                        const WideArgs& wd = WideArgs());
}  // namespace lig

// (outside the anonymous namespace: these types appear in functions shared between translation units)
// the derived rows of a packed matrix, ascending, and their copy on the device: what launch_expand_rows takes for rows [b, e)
struct ProductRows {
    std::vector<uint32_t> rows;
    uint32_t* dev = nullptr;
    const uint32_t* first(size_t b) const { return dev + (std::lower_bound(rows.begin(), rows.end(), (uint32_t)b) - rows.begin()); }
    size_t count(size_t b, size_t e) const { return std::lower_bound(rows.begin(), rows.end(), (uint32_t)e) - std::lower_bound(rows.begin(), rows.end(), (uint32_t)b); }
};
// the mixed rows of a packed matrix (lig_rows_job.wide_per_row), ascending, with the records of every row (`wide`: empty when no row
// is mixed), their copies on the device and the flag word of k_expand_wide: what launch_expand_rows takes for rows [b, e)
struct WideRows {
    ProductRows mixed;
    std::vector<uint32_t> wide;
    uint32_t* wide_dev = nullptr; uint32_t* flag_dev = nullptr;
    uint32_t max_records = 0;
    bool any() const { return !mixed.rows.empty(); }
    lig::WideArgs args(size_t b, size_t e) const {
        lig::WideArgs a;
        if (!any()) return a;
        a.mixed_rows_dev = mixed.first(b); a.n_mixed = mixed.count(b, e); a.wide_dev = wide_dev; a.max_records = max_records; a.flag_dev = flag_dev;
        return a;
    }
    void release() { (void)hipFree(mixed.dev); (void)hipFree(wide_dev); (void)hipFree(flag_dev); mixed.dev = wide_dev = flag_dev = nullptr; }
};
// a packed plan (rows_plan.hpp) -> what launch_expand_rows reads on the device (expand.hip; synchronous copies, the caller frees)
int lig_internal_upload_narrow_plan(lig_ctx* c, const lig::NarrowPlan& plan, uint64_t** src_off_dev, uint8_t** widths_dev, ProductRows* prod, WideRows* wide);
// what a trace or a shard keeps of its job's header; ih = instance_hash of the public arguments
struct JobHeader {
    uint8_t encoding_seed[32] = {0}, program_hash[32] = {0}, ih[32] = {0};
    int64_t generated_at = 0;
    char version[17] = {0};
};

namespace {

using clk = std::chrono::steady_clock;
double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

// ---------------------------------------------------------------- host crypto (OpenSSL, as the reference: hash.hpp:153-214, csprng.hpp)
struct Sha256 {
    EVP_MD_CTX* c;
    Sha256() : c(EVP_MD_CTX_new()) { EVP_DigestInit_ex(c, EVP_sha256(), nullptr); }
    ~Sha256() { EVP_MD_CTX_free(c); }
    Sha256& add(const void* p, size_t n) { EVP_DigestUpdate(c, p, n); return *this; }
    void finish(uint8_t out[32]) { unsigned int l = 32; EVP_DigestFinal_ex(c, out, &l); }
};
// keystream element e of the AES-256-CTR stream (IV = 0): blocks 2e, 2e+1  -> field element (finite_field_gmp.hpp:66-78)
struct FieldStream {
    EVP_CIPHER_CTX* c;
    explicit FieldStream(const uint8_t key[32]) : c(EVP_CIPHER_CTX_new()) {
        const uint8_t iv[16] = {0};
        EVP_EncryptInit_ex(c, EVP_aes_256_ctr(), nullptr, key, iv);
    }
    ~FieldStream() { EVP_CIPHER_CTX_free(c); }
    // sequential draws (the engine is only ever read front to back on the host)
    void next(size_t count, std::vector<H::Fr>& out) {
        std::vector<uint8_t> zero(32 * count, 0), ks(32 * count);
        int len = 0;
        EVP_EncryptUpdate(c, ks.data(), &len, zero.data(), (int)zero.size());
        out.resize(count);
        for (size_t i = 0; i < count; i++) {
            H::Fr v;
            std::memcpy(v.v, ks.data() + 32 * i, 32);
            for (int w = 0; w < 4; w++) v.v[w] = (v.v[w] >> 2) | (w < 3 ? (v.v[w + 1] << 62) : 0);
            if (H::geq(v, H::P)) v = H::sub_nored(v, H::P);
            out[i] = v;
        }
    }
};

// instance_hash over arg0 = "Ligero\0" and the public arguments (src/webgpu_prover.cpp:110-168; src/webgpu_verifier.cpp mirrors it)
bool instance_hash(const uint8_t* args, const uint64_t* lens, uint64_t n_args, uint8_t out[32]) {
    if (n_args && (!args || !lens)) return false;
    std::memset(out, 0, 32);
    Sha256().add(out, 32).add("Ligero", 7).finish(out);
    for (uint64_t i = 0; i < n_args; i++) {
        uint8_t prev[32];
        std::memcpy(prev, out, 32);
        Sha256().add(prev, 32).add(args, lens[i]).finish(out);
        args += lens[i];
    }
    return true;
}
// lig_synth_job or lig_rows_job -> header; false: public arguments announced but not given
template <class Job> bool fill_job_header(const Job& job, JobHeader& h) {
    std::memcpy(h.encoding_seed, job.encoding_seed, 32);
    std::memcpy(h.program_hash, job.program_hash, 32);
    std::memcpy(h.version, job.version, 16);
    h.generated_at = job.generated_at;
    return instance_hash(job.public_args, job.public_arg_lens, job.n_public_args, h.ih);
}
void stage1_seed(const uint8_t root[32], const uint8_t ih[32], uint8_t out[32]) {
    Sha256().add("LigetronStage1", 15).add(root, 32).add(ih, 32).finish(out);
}

// hash_random_engine<sha256> (include/zkp/random.hpp:87-146)
struct HashRandomEngine {
    uint8_t seed[32], buf[32];
    uint64_t state = 0;
    int off = -1;
    explicit HashRandomEngine(const uint8_t s[32]) { std::memcpy(seed, s, 32); }
    uint8_t operator()() {
        if (off < 0) {
            Sha256 h;
            if (state) h.add(seed, 32);             // the seed is absorbed only after the first flush
            uint8_t le[8];
            for (int i = 0; i < 8; i++) le[i] = (uint8_t)(state >> (8 * i));
            h.add(le, 8).finish(buf);
            state++;
            off = 31;
        }
        return buf[off--];
    }
};
// boost::random::detail::generate_uniform_int(Engine&, T min, T max, boost::true_type) of
// boost/random/uniform_int_distribution.hpp (the integer-engine overload; unchanged since the header appeared in Boost 1.47,
// read from memory against 1.74 / 1.83 -- Boost is neither vendored upstream, CMakeLists.txt:67-69, nor in this image, so the
// sample indices stay "parity unpinned") for the 8-bit engine above (brange = 255, bmin = 0) and range_type = uint64_t
// (Distance = ptrdiff_t, include/util/portable_sample.hpp:26).  Tags B1..B4 name the statements of the Boost function in
// order; oracle/hash.c (boost_uniform) quotes them one by one.  Returns a value in [0, range].
uint64_t uniform_u64(HashRandomEngine& e, uint64_t range) {
    if (range == 0) return 0;                         // B1  if(range == 0) return min_value;
    if (range == 255) return e();                     // B2  else if(brange == range) return eng() - bmin + min_value;
    if (range < 255) {                                // B4  else (brange > range):
        const uint64_t bucket = 256 / (range + 1);    // B4a bucket_size: base_unsigned = uint8_t, brange == max -> 255/(range+1), +1 if 255%(range+1) == range: the same number
        for (;;) { const uint64_t r = e() / bucket; if (r <= range) return r; }      // B4b
    }
    for (;;) {                                        // B3  else if(brange < range) for(;;)
        const uint64_t limit = (range + 1) / 256;     // B3a (range < 2^64 - 1 always here: the max(range_type) special case cannot occur)
        uint64_t result = 0, mult = 1;                // B3b
        bool exact = false;
        while (mult <= limit) {                       // B3c
            result += (uint64_t)e() * mult;
            if (mult * 255 == range - mult + 1) { exact = true; break; }     // B3d: range+1 is a power of 256 -> return result
            mult *= 256;                              // B3e
        }
        if (exact) return result;
        uint64_t inc = uniform_u64(e, range / mult);  // B3f  generate_uniform_int(eng, 0, range/mult, true_type())
        if (UINT64_MAX / mult < inc) continue;        // B3g
        inc *= mult;                                  // B3h
        result += inc;
        if (result < inc || result > range) continue; // B3i, B3j
        return result;                                // B3k
    }
}
// portable_sample + sort (include/util/portable_sample.hpp:15-33, src/webgpu_prover.cpp:343-351)
std::vector<uint32_t> sample_columns(const uint8_t seed[32], uint32_t n, uint32_t t) {
    HashRandomEngine e(seed);
    std::vector<uint32_t> a(n), out;
    for (uint32_t i = 0; i < n; i++) a[i] = i;
    if (t > n) t = n;
    for (uint32_t i = 0; i < t; i++) {
        const uint64_t j = i + uniform_u64(e, (uint64_t)(n - 1) - i);
        std::swap(a[i], a[j]);
        out.push_back(a[i]);
    }
    std::sort(out.begin(), out.end());
    return out;
}
// merkle_tree::decommit + canonical sibling order (merkle_tree.hpp:155-215, proof_serializer.hpp:82-117)
std::vector<uint8_t> decommit(const uint8_t* nodes, size_t P, const std::vector<uint32_t>& idx) {
    std::vector<uint8_t> sib;
    std::vector<uint8_t> known(P, 0), upper(P, 0);
    for (uint32_t i : idx) known[i] = 1;
    size_t start = P - 1, end = 2 * P - 1;
    while (start > 0) {
        std::fill(upper.begin(), upper.end(), 0);
        for (size_t i = start; i < end; i += 2) {
            const size_t ll = i - start;
            const bool kl = known[ll], kr = known[ll + 1];
            if (kl && kr) upper[ll / 2] = 1;
            else if (kr) { sib.insert(sib.end(), nodes + 32 * i, nodes + 32 * i + 32); upper[ll / 2] = 1; }
            else if (kl) { sib.insert(sib.end(), nodes + 32 * (i + 1), nodes + 32 * (i + 1) + 32); upper[ll / 2] = 1; }
        }
        known.swap(upper);
        start = (start - 1) / 2; end = (end - 1) / 2;
    }
    return sib;
}

// ---------------------------------------------------------------- protobuf wire writer (proto/ligero_proof.proto, proto/common.proto)
struct Pb {
    std::vector<uint8_t> b;
    void var(uint64_t v) { do { uint8_t c = v & 0x7f; v >>= 7; if (v) c |= 0x80; b.push_back(c); } while (v); }
    void tag(uint32_t f, uint32_t wt) { var(((uint64_t)f << 3) | wt); }
    void u(uint32_t f, uint64_t v) { if (v) { tag(f, 0); var(v); } }
    void bytes(uint32_t f, const void* p, size_t n) { tag(f, 2); var(n); const uint8_t* q = (const uint8_t*)p; b.insert(b.end(), q, q + n); }
    void msg(uint32_t f, const Pb& m) { bytes(f, m.b.data(), m.b.size()); }
};
size_t varlen(uint64_t v) { size_t n = 1; while (v > 0x7f) { v >>= 7; n++; } return n; }

// serialize_proof (include/zkp/proof_serializer.hpp:166-191) + metadata (src/webgpu_prover.cpp:410-427), written
// straight into a caller-provided (pinned) buffer.  The four FixedU32Vector payloads are raw little-endian limb
// bytes: the three accumulators are copied in, the position of the sample payload is returned so that the
// device->host copy of the opened columns lands directly inside the envelope.
// (enc3 == nullptr: the framing is written, the three accumulators are NOT copied -- vec_off says where they belong, so that
// the caller can start the download of the opened columns first and copy them while it runs)
struct EnvelopeLayout { size_t total = 0, samples_off = 0, vec_off[3] = {0, 0, 0}; };
EnvelopeLayout write_envelope(uint8_t* dst, size_t cap, const char* version, const uint8_t program_hash[32], int64_t generated_at,
                              uint32_t k, uint32_t n, uint32_t t, const uint8_t root[32], const std::vector<uint8_t>& siblings,
                              const std::vector<uint32_t>& idx, const uint8_t* enc3, size_t sample_bytes) {
    auto digest = [](const uint8_t d[32]) { Pb m; m.bytes(1, d, 32); return m; };
    Pb meta;
    if (version[0]) meta.bytes(1, version, std::strlen(version));
    meta.u(2, 1); meta.u(3, 1);
    meta.msg(4, digest(program_hash));
    { Pb ts; ts.u(1, (uint64_t)generated_at); meta.msg(5, ts); }
    meta.u(6, k); meta.u(7, n); meta.u(8, t); meta.u(9, 128);
    Pb md;
    md.u(1, 1);
    md.msg(2, digest(root));
    for (size_t i = 0; i < siblings.size() / 32; i++) md.msg(3, digest(siblings.data() + 32 * i));
    if (!idx.empty()) { Pb pk; for (uint32_t v : idx) pk.var(v); md.bytes(4, pk.b.data(), pk.b.size()); }
    const size_t vec = (size_t)n * 32;
    auto fixed_len = [](size_t nb) { return nb ? 1 + varlen(nb) + nb : 0; };
    const size_t body_len = 1 + varlen(md.b.size()) + md.b.size() + 3 * (1 + varlen(fixed_len(vec)) + fixed_len(vec)) + 1 +
                            varlen(fixed_len(sample_bytes)) + fixed_len(sample_bytes);
    Pb head;
    head.msg(1, meta);
    head.tag(2, 2); head.var(body_len);
    head.msg(1, md);
    EnvelopeLayout L;
    size_t pos = 0;
    auto put = [&](const void* p, size_t nb) { if (pos + nb <= cap) std::memcpy(dst + pos, p, nb); pos += nb; };
    put(head.b.data(), head.b.size());
    for (uint32_t f = 2; f <= 5; f++) {
        const size_t nb = f < 5 ? vec : sample_bytes;
        Pb h;
        h.tag(f, 2); h.var(fixed_len(nb));
        if (nb) { h.tag(1, 2); h.var(nb); }
        put(h.b.data(), h.b.size());
        if (f < 5) { L.vec_off[f - 2] = pos; if (enc3) put(enc3 + (size_t)(f - 2) * vec, nb); else pos += nb; }
        else { L.samples_off = pos; pos += nb; }
    }
    L.total = pos;
    return L;
}

// Commit order: rows of the batch program in program order, then witness_manager's order for the synthetic stream
// (witness_manager.hpp:497-503): full linear rows, full quadratic triples, partial linear row, partial quadratic triple.
// Returns false for a malformed batch program.  n_init = rows that draw padding from the encoding stream at init time.
bool plan_rows(const lig_synth_job& job, uint32_t l, std::vector<RowDesc>& rows, size_t& n_init) {
    rows.clear();
    n_init = 0;
    if (job.n_batch_ops && !job.batch_ops) return false;
    for (uint64_t i = 0; i < job.n_batch_ops; i++) {
        const lig_batch_op& o = job.batch_ops[i];
        if (o.op >= LIG_BOP_COUNT || o.out >= 512 || o.x >= 512 || o.y >= 512) return false;
        const uint64_t need = o.op == LIG_BOP_SET ? 32ull * o.len : o.op == LIG_BOP_BIT_DECOMPOSE ? 4ull * o.len :
                              (o.op == LIG_BOP_SET_SCALAR || (o.op >= LIG_BOP_ADD_CONST && o.op <= LIG_BOP_MONTMUL_CONST)) ? 32 : 0;
        if (need && (!job.batch_data || o.data_off > job.batch_data_bytes || need > job.batch_data_bytes - o.data_off)) return false;
        if (o.op == LIG_BOP_SET && o.len > l) return false;
        if (o.op == LIG_BOP_BIT_DECOMPOSE) {
            if (o.len > 256) return false;
            for (uint32_t b = 0; b < o.len; b++) {           // every output slot inside the slab and different from the source
                uint32_t slot;
                std::memcpy(&slot, job.batch_data + o.data_off + 4ull * b, 4);
                if (slot >= 512 || slot == o.x) return false;
            }
        }
        switch (o.op) {
            case LIG_BOP_SET: case LIG_BOP_SET_SCALAR: rows.push_back({RK_INIT, 0}); n_init++; break;
            case LIG_BOP_COPY: case LIG_BOP_ASSERT_EQUAL: rows.push_back({RK_EQX, 0}); rows.push_back({RK_EQY, 0}); break;
            case LIG_BOP_MUL: case LIG_BOP_DIV: rows.push_back({RK_BQX, 0}); rows.push_back({RK_BQY, 0}); rows.push_back({RK_BQZ, 0}); break;
            case LIG_BOP_BIT_DECOMPOSE: for (uint32_t b = 0; b < o.len; b++) rows.push_back({RK_BIT, 0}); break;
            default: break;
        }
    }
    const size_t lf = job.n_linear / l, lp = job.n_linear % l, qf = job.n_quad / l, qp = job.n_quad % l;
    for (size_t i = 0; i < lf; i++) rows.push_back({0, l});
    for (size_t i = 0; i < qf; i++) for (uint8_t q = 1; q <= 3; q++) rows.push_back({q, l});
    if (lp) rows.push_back({0, (uint32_t)lp});
    if (qp) for (uint8_t q = 1; q <= 3; q++) rows.push_back({q, (uint32_t)qp});
    return true;
}
// Row-chunk schedule [begin, end) pairs.  Chunks are `big` rows except that the exposed end of a two-stream pipeline
// is kept short: `head` rows first (stage 2: the encode stream waits for the first randomness rows) and/or a short
// last chunk of `tail` rows (stage 1: the column hash of the last chunk runs after the last encode).
std::vector<std::pair<size_t, size_t>> chunk_schedule(size_t R, size_t big, size_t head, size_t tail) {
    std::vector<std::pair<size_t, size_t>> out;
    size_t b = 0;
    if (head && R > head + tail) { out.push_back({0, head}); b = head; }
    const size_t stop = (tail && R > b + tail) ? R - tail : R;
    while (b < stop) { const size_t e = std::min(stop, b + big); out.push_back({b, e}); b = e; }
    if (b < R) out.push_back({b, R});
    return out;
}

lig::f29s to_f29s_host(const H::Fr& plain, const H::Fr& scale) {
    const H::Fr m = H::mul(plain, scale);
    lig::f29s o;
    std::memset(&o, 0, sizeof o);
    for (int i = 0; i < 9; i++) {
        const int bit = 29 * i, w = bit >> 6, sh = bit & 63;
        uint64_t v = m.v[w] >> sh;
        if (sh > 35 && w < 3) v |= m.v[w + 1] << (64 - sh);
        o.v[i] = (uint32_t)(i < 8 ? (v & 0x1FFFFFFFull) : v);
    }
    return o;
}
const H::Fr R261 = {{0x2fd4e1568fffff57ull, 0x75bba827a494b01aull, 0x5301fa84819caa80ull, 0x0dc83629563d4475ull}};   // 2^261 mod p

// Stage-2 coefficients, both streams keyed by the stage-1 seed: one code-stream draw per row that has a code check, in commit order
// (code[r]; zero for a row without one), one quadratic-stream draw per term of quad_terms (quad[i])
struct Coefficients { std::vector<H::Fr> code, quad; };
Coefficients draw_coefficients(const uint8_t seed1[32], const std::vector<RowDesc>& rows) {
    Coefficients cf;
    std::vector<H::Fr> rc;
    FieldStream code_s(seed1), quad_s(seed1);
    size_t n_code = 0;
    for (const RowDesc& d : rows) n_code += has_code_check(d.kind);
    code_s.next(n_code, rc);
    quad_s.next(quad_terms(rows).size() / 3, cf.quad);
    cf.code.assign(rows.size(), H::from_u64(0));
    for (size_t r = 0, ci = 0; r < rows.size(); r++) if (has_code_check(rows[r].kind)) cf.code[r] = rc[ci++];
    return cf;
}
// the table the stage-2 kernels read, for the rows and terms a device holds (global indices; nullptr: all of them, in order):
// [rc of every row | rq * 2^522 of every term | rq * 2^261 of every term | one spare], 29-bit limbs
std::vector<lig::f29s> coef_table(const Coefficients& cf, const std::vector<size_t>* rows, const std::vector<size_t>* terms) {
    const size_t nr = rows ? rows->size() : cf.code.size(), nt = terms ? terms->size() : cf.quad.size();
    const H::Fr R261sq = H::mul(R261, R261);
    std::vector<lig::f29s> coef(nr + 2 * nt + 1);
    std::memset(coef.data(), 0, coef.size() * sizeof(lig::f29s));
    for (size_t r = 0; r < nr; r++) coef[r] = to_f29s_host(cf.code[rows ? (*rows)[r] : r], R261);
    for (size_t i = 0; i < nt; i++) {
        const H::Fr& rq = cf.quad[terms ? (*terms)[i] : i];
        coef[nr + i] = to_f29s_host(rq, R261sq);
        coef[nr + nt + i] = to_f29s_host(rq, R261);
    }
    return coef;
}

// The self-check on the three decoded accumulators (dec: 3 x n; src/webgpu_prover.cpp:355-386,465-469, webgpu_verifier.cpp:412-442):
// the code polynomial has degree < k, the linear polynomial sums to minus the constant over the l data slots, the quadratic one
// vanishes on them
struct SelfCheck { int valid_code, valid_linear, valid_quad; };
SelfCheck self_check(const H::Fr* dec, const uint8_t const_sum[32], uint32_t l, uint32_t k, uint32_t n) {
    auto is_zero = [](const H::Fr& v) { return !(v.v[0] | v.v[1] | v.v[2] | v.v[3]); };
    SelfCheck ok;
    ok.valid_code = 1;
    for (uint32_t i = k; i < n; i++) if (!is_zero(dec[i])) ok.valid_code = 0;
    H::Fr a;
    std::memcpy(a.v, const_sum, 32);
    for (uint32_t i = 0; i < l; i++) a = H::add(a, dec[(size_t)n + i]);
    ok.valid_linear = is_zero(a);
    ok.valid_quad = 1;
    for (uint32_t i = 0; i < l; i++) if (!is_zero(dec[2 * (size_t)n + i])) ok.valid_quad = 0;
    return ok;
}

}  // namespace

#define TRY(x) do { int rc__ = (x); if (rc__ != LIG_OK) return rc__; } while (0)


// launch granularity shared by the prover, the sharded prover and the verifier
struct lig_tune {
#ifndef LIG_CHUNK
#define LIG_CHUNK 512
#endif
    static constexpr size_t CHUNK = LIG_CHUNK;       // rows per encode / hash / accumulate launch group
    static constexpr uint32_t GROUP = 64;      // rows per lazily accumulated group (n-column passes; k-column passes use GROUP / 4)
#ifndef LIG_DOT_GROUP
#define LIG_DOT_GROUP 8
#endif
    static constexpr uint32_t DOT_GROUP = LIG_DOT_GROUP;   // rows per group of the fused coset-2 encode + dot (lig_internal_encode_dot): 64 groups x 1024 threads per chunk
};

// a sparse linear system on the device (linear.hip; lig_hip.h: lig_linear_system): create = lig_linear_check + upload + regroup by
// slot, synchronous on the context stream; form = enqueue on `st` the rows x k randomness matrix for the stream whose round keys are
// in rk60_dev -- the constant (32 bytes, pinned host memory) is valid once the work queued on `st` has been waited for
// Two objects (linear.hip): lig_linear_program = the regrouped structure, immutable after the prepare, reference counted, shared;
// lig_linear = one user's ATTACHMENT to a program: a reference plus everything a form writes (r, partial sums, the pinned constant,
// an overriding coefficient table).  create = prepare + attach + release: a program nobody else holds.
struct lig_linear;
int lig_internal_linear_prepare(lig_ctx* c, const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, lig_linear_program** out);
int lig_internal_linear_attach(lig_ctx* c, const lig_linear_program* P, lig_linear** out);
bool lig_internal_linear_fits(const lig_ctx* c, const lig_linear_program* P, const uint8_t* kinds, uint64_t rows);      // device, l, k, rows, kinds (host only)
// canonical table -> the attachment's own Montgomery copy, enqueued on `st` (the stream its forms run on); NULL: the program's table
int lig_internal_linear_set_values(lig_ctx* c, lig_linear* L, const uint8_t* coefs, uint64_t n_coefs, hipStream_t st);
int lig_internal_linear_create(lig_ctx* c, const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, lig_linear** out);
void lig_internal_linear_destroy(lig_linear* L);
int lig_internal_linear_form(lig_ctx* c, lig_linear* L, const uint32_t* rk60_dev, fr* rands_dev, hipStream_t st);
const uint8_t* lig_internal_linear_const(const lig_linear* L);
// one rank of a sharded trace (lig_shard_rows_set_linear): the system describes the whole trace, `grow` = the global row of every local row.
// The rank keeps the terms of its rows, samples the constraints it needs (stats), forms its local rows x k matrix and its un-negated
// share of sum_c b_c r_c (partial_dev, one device element); const_buf = 32 pinned bytes the shard downloads the summed shares into.
int lig_internal_linear_create_shard(lig_ctx* c, const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, const std::vector<size_t>& grow, uint32_t rank,
                                     uint32_t world, lig_linear** out);
void lig_internal_linear_shard_count(const lig_linear_system* sys, uint32_t l, const std::vector<size_t>& grow, uint64_t rows, uint32_t rank, uint32_t world,
                                     uint64_t* local_terms, uint64_t* needed);
void lig_internal_linear_stats(const lig_linear* L, uint64_t* local_terms, uint64_t* sampled);
const fr* lig_internal_linear_partial_dev(const lig_linear* L);
uint8_t* lig_internal_linear_const_buf(lig_linear* L);
// a read-only view of an attachment (lig_rows_diagnose_attached): the slot-major index of its program -- the segment of slot s is
// ent[begin[s] .. begin[s + 1]), ent = (constraint, coefficient index) --, the right-hand sides, and the Montgomery table IN FORCE for
// this attachment (the program's, or the values of lig_rows_set_linear_values).  coef_ready: NULL, or the event recorded behind the
// conversion of those values on the stream they were set on -- a reader on another stream waits for it first.
struct lig_linear_view {
    bool sharded = false;                              // one rank's local, compactly numbered structure: not a system of the whole trace
    uint64_t n_constraints = 0, n_terms = 0, n_rhs = 0;
    uint32_t n_slots = 0;
    // sharded: begin[] covers the LOCAL slots of rows_local rows, n_terms = the terms kept, n_rhs = the rank's slice of the right-hand sides;
    // ent[].x and rhs_c[] are COMPACT numbers i < n_need, need[i] = the constraint of the whole trace (ascending); n_constraints stays global
    const uint32_t* need = nullptr;
    uint64_t n_need = 0, rows_local = 0;
    const uint32_t* begin = nullptr;
    const uint2* ent = nullptr;
    const uint32_t *rhs_c = nullptr, *rhs_coef = nullptr;
    const fr* coef = nullptr;
    hipEvent_t coef_ready = nullptr;
};
lig_linear_view lig_internal_linear_view(const lig_linear* L);

// derived slots (derive.hip; lig_hip.h: lig_rows_set_derived): create = lig_linear_check + plan_derived (derive_plan.hpp) against the kinds and
// widths given (elem_bytes: one per row, or NULL) + the program copied to the device, its table converted on the context stream; synchronous.
// run = one launch per wave on `st` over the expanded rows x k matrix `msgs` (stage 1, in front of the first encode).
struct lig_derive;
int lig_internal_derive_create(lig_ctx* c, const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, const uint8_t* elem_bytes, const lig_derived_slot* d,
                               uint64_t n, lig_derive** out, lig_derived_info* info);
void lig_internal_derive_destroy(lig_derive* D);
int lig_internal_derive_run(lig_ctx* c, const lig_derive* D, fr* msgs, hipStream_t st);
// the same on a rows shard (lig_shard_rows_set_derived): owner = the rank of every row of the whole trace (the deal); create = the check above +
// plan_derived_shard for `rank`, the rank's program on the device, and what the shard has to provide: a send block of send_elems and an
// import buffer of import_elems elements.  run = per wave export kernel + all_gather (only for a wave in which something crosses ranks) +
// wave kernel on `st`.  count = the numbers alone, host only.
struct lig_derive_shard;
int lig_internal_derive_shard_count(const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, uint32_t l, const uint8_t* elem_bytes, const lig_derived_slot* d,
                                    uint64_t n, const std::vector<uint32_t>& owner, uint32_t rank, uint32_t world, lig_derived_shard_info* info);
int lig_internal_derive_shard_create(lig_ctx* c, const lig_linear_system* sys, const uint8_t* kinds, uint64_t rows, const uint8_t* elem_bytes, const lig_derived_slot* d,
                                     uint64_t n, const std::vector<uint32_t>& owner, uint32_t rank, uint32_t world, lig_derive_shard** out, uint64_t* send_elems,
                                     uint64_t* import_elems, lig_derived_shard_info* info);
void lig_internal_derive_shard_destroy(lig_derive_shard* D);
int lig_internal_derive_shard_run(lig_ctx* c, const lig_derive_shard* D, fr* msgs, fr* send, fr* imported, hipStream_t st,
                                  const std::function<int(const void*, void*, size_t, const char*)>& all_gather);
// lig_rows_diagnose (diagnose.hip): the residual of every linear constraint of `sys` (NULL: none; it has passed lig_linear_check) and of every
// (quadratic term, column < l) over the committed rows x k matrix `msgs`; tri_dev = the trace's quadratic terms, 3 row indices each.
// Blocking, on the context's main stream; waits the way a proof does (lig_internal_wait_stream, prover.hip).
int lig_internal_rows_diagnose(lig_ctx* c, const fr* msgs, uint64_t rows, const uint32_t* tri_dev, uint64_t n_quad_terms, const lig_linear_system* sys,
                               lig_diag_linear* lin_out, uint64_t lin_cap, lig_diag_quad* quad_out, uint64_t quad_cap, lig_diag_info* info);
// lig_rows_diagnose_attached: the same passes over the statement ATTACHED to the trace (`att`: not sharded), regrouped by constraint on the device
int lig_internal_rows_diagnose_attached(lig_ctx* c, const fr* msgs, uint64_t rows, const uint32_t* tri_dev, uint64_t n_quad_terms, const lig_linear* att,
                                        lig_diag_linear* lin_out, uint64_t lin_cap, lig_diag_quad* quad_out, uint64_t quad_cap, lig_diag_info* info);
// lig_rows_explain / lig_rows_explain_attached / lig_rows_read_slots (diagnose.hip): the asked constraints of `sys` (it has passed
// lig_linear_check) or of the statement attached (`att`: not sharded) as records over the committed matrix; the asked list and the slots are
// checked here, on the host, before anything is launched (LIG_E_ARG).  Blocking, main stream only, scratch per call.
int lig_internal_rows_explain(lig_ctx* c, const fr* msgs, const lig_linear_system* sys, const uint32_t* asked, uint64_t n_asked, lig_explain_constraint* con_out,
                              lig_explain_term* terms_out, uint64_t term_cap, lig_explain_info* info);
int lig_internal_rows_explain_attached(lig_ctx* c, const fr* msgs, const lig_linear* att, const uint32_t* asked, uint64_t n_asked, lig_explain_constraint* con_out,
                                       lig_explain_term* terms_out, uint64_t term_cap, lig_explain_info* info);
int lig_internal_rows_read_slots(lig_ctx* c, const fr* msgs, uint64_t rows, const uint32_t* slots, uint64_t n_slots, uint8_t* values);
// lig_rows_explain_slots* / lig_rows_untouched_slots* (diagnose.hip): the constraints through the asked slots, and the LINEAR .. QZ slots no term
// touches, straight from the slot-major index of `v` -- the view of the trace's attachment, or lig_internal_linear_program_view of a program
// prepared from the caller's term list (its own table in force).  kinds: one per committed row.  The asked slots are checked here, on the
// host, before anything is launched (LIG_E_ARG); a sharded view is LIG_E_STATE.  Blocking, main stream only, scratch per call.
lig_linear_view lig_internal_linear_program_view(const lig_linear_program* P);
int lig_internal_rows_explain_slots(lig_ctx* c, const fr* msgs, const uint8_t* kinds, uint64_t rows, const lig_linear_view& v, const uint32_t* slots, uint64_t n_asked,
                                    lig_slot_record* slot_out, lig_slot_term* terms_out, uint64_t term_cap, lig_slot_info* info);
int lig_internal_rows_untouched_slots(lig_ctx* c, const fr* msgs, const uint8_t* kinds, uint64_t rows, const lig_linear_view& v, int nonzero_only, lig_slot_value* out,
                                      uint64_t cap, lig_untouched_info* info);
hipError_t lig_internal_wait_stream(hipStream_t st);
// lig_shard_rows_diagnose (diagnose.hip): what one rank of a sharded rows job holds, and the shard's collectives and waits (shard.hip).
// all_to_all / all_gather run on the context's main stream (stream-ordered forms) or after it has drained (host-synchronous callbacks);
// drain = the bounded wait of every lig_shard_* call; settle_failed = after a failure: drain within bounds, true when the shard is
// poisoned (the scratch of the call then outlives it); forget = lig_comm.forget.
struct lig_diag_shard {
    const fr* msgs = nullptr;                          // the committed LOCAL rows x k
    const std::vector<size_t>* grow = nullptr;         // global row of every local row
    uint64_t rows_global = 0;
    const uint32_t* tri_dev = nullptr;                 // local quadratic terms, local row indices
    const std::vector<size_t>* triple_ord = nullptr;   // their global ordinals
    uint64_t n_terms_global = 0;
    uint32_t rank = 0, world = 1;
    uint64_t slice = 0;                                // LIG_DIAG_SLICE
    std::function<int(const void*, void*, size_t, const char*)> all_to_all, all_gather;
    std::function<int(const char*)> drain;
    std::function<bool()> settle_failed;
    std::function<void()> forget;
};
int lig_internal_shard_diagnose(lig_ctx* c, const lig_diag_shard& v, const lig_linear_system* sys, lig_diag_linear* lin_out, uint64_t lin_cap, lig_diag_quad* quad_out,
                                uint64_t quad_cap, lig_diag_info* info);
// lig_shard_rows_diagnose_attached: the same collective schedule over the rank's share ATTACHED to the shard (`att`: sharded), regrouped by
// compact constraint on the device; the holder of a right-hand side subtracts it in its partial
int lig_internal_shard_diagnose_attached(lig_ctx* c, const lig_diag_shard& v, const lig_linear* att, lig_diag_linear* lin_out, uint64_t lin_cap,
                                         lig_diag_quad* quad_out, uint64_t quad_cap, lig_diag_info* info);
// lig_shard_rows_explain / lig_shard_rows_read_slots (diagnose.hip) on the same view (all_to_all is not used): sys has passed
// lig_linear_check, asked explain_asked_ok, the slots explain_slots_ok against the rows of the whole trace; n_asked > 0, n_slots > 0.
int lig_internal_shard_explain(lig_ctx* c, const lig_diag_shard& v, const lig_linear_system* sys, const uint32_t* asked, uint64_t n_asked,
                               lig_explain_constraint* con_out, lig_explain_term* terms_out, uint64_t term_cap, lig_explain_info* info);
int lig_internal_shard_read_slots(lig_ctx* c, const lig_diag_shard& v, const uint32_t* slots, uint64_t n_slots, uint8_t* values);
// lig_shard_rows_explain_attached: the asked constraints from the rank's share ATTACHED to the shard (`att`: sharded) -- selected on the
// device, the records gathered whole; asked has passed explain_asked_ok against the global constraint count, n_asked > 0.  alone: one rank
// without the forced exchange -- the same passes without a collective.
int lig_internal_shard_explain_attached(lig_ctx* c, const lig_diag_shard& v, const lig_linear* att, bool alone, const uint32_t* asked, uint64_t n_asked,
                                        lig_explain_constraint* con_out, lig_explain_term* terms_out, uint64_t term_cap, lig_explain_info* info);
// lig_shard_rows_explain_slots* / lig_shard_rows_untouched_slots*: the constraints through the asked slots (of the WHOLE trace, checked and
// strictly ascending, n_asked > 0) and the untouched LINEAR .. QZ slots from the rank's share `att` (sharded: the one attached to the shard,
// or a temporary one made from the caller's term list); kinds: one per committed row of the whole trace; alone as above.
int lig_internal_shard_explain_slots(lig_ctx* c, const lig_diag_shard& v, const lig_linear* att, bool alone, const uint8_t* kinds, const uint32_t* slots, uint64_t n_asked,
                                     lig_slot_record* slot_out, lig_slot_term* terms_out, uint64_t term_cap, lig_slot_info* info);
int lig_internal_shard_untouched_slots(lig_ctx* c, const lig_diag_shard& v, const lig_linear* att, bool alone, const uint8_t* kinds, int nonzero_only, lig_slot_value* out,
                                       uint64_t cap, lig_untouched_info* info);

// the batch program of a job on the device: committed rows are written to rows_out in program order (prover.hip)
int lig_run_batch_program(lig_ctx* c, const lig_synth_job& job, fr* rows_out);
// witness values of the synthetic stream rows [first, rows.size()) (one draw of the witness_key stream per data slot of every
// linear / x / y row in commit order, z = x*y); row r is written to msgs + r*k.  Enqueued on the context stream.
int lig_internal_synth_witness(lig_ctx* c, const uint8_t witness_key[32], const std::vector<RowDesc>& rows, size_t first, fr* msgs);
// the three mask rows of stage 1 in place (maskcw: 3 x n, reference layout) from element epos of the encoding stream, whose round keys
// are in c->rk_dev: a memset and six launches on `stream`; dots = one device element of scratch (prover.hip)
int lig_internal_form_mask_rows(lig_ctx* c, hipStream_t stream, uint64_t epos, fr* maskcw, fr* dots);
