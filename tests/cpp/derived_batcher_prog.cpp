// derived_batcher_prog.cpp -- hip_proof_meta::derive_products: the z row of every triple the guest records is NOT shipped
// (LIG_ELEM_PRODUCT); the library forms x * y mod p on the device.  The oracle plays guest + witness_manager (lo_form_rows: rows
// with their pads); the triples cycle through bit operands, 8-byte operands and the oracle's own full field elements.  What the
// guest hands over as z is garbage throughout: the expected bytes come from the oracle's prover over the TRUE rows.
//   part A  two passes, dense randomness rows: envelope == lo_prove_rows, shipped_bytes() == the figure computed here
//   part B  set_linear_system with the true statement (one constraint w[s] = b_s per data slot): valid, envelope == lo_prove_rows
//   part C  the same with a guest whose statement about one z slot is false: valid_linear == 0
//   usage: derived_batcher_prog                       one GPU
//          derived_batcher_prog rank world /shm_name   one trace sharded over `world` processes (comm_ipc)
// Prints one JSON line.
// TEST CODE: links oracle/liblig_oracle.so as the checker.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/lig_hip_row_batcher.hpp"
#include "../../oracle/lig_oracle.h"

int main(int argc, char** argv) {
    const bool sharded = argc >= 4;
    const uint32_t rank = sharded ? std::atoi(argv[1]) : 0, world = sharded ? std::atoi(argv[2]) : 1;
    const uint32_t l = 320, k = 512, n = 2048;
    lo_job j;
    std::memset(&j, 0, sizeof j);
    j.l = l; j.k = k; j.n = n; j.t = 192;
    j.n_linear = 320 * 90;                            // full rows only (every row carries l constraints); two stage-1 chunks and more
    j.n_quad = 320 * 100;                             // linear rows come first: 300 triple rows, so that each of two ranks holds triples
    for (int i = 0; i < 32; i++) j.encoding_seed[i] = (uint8_t)(5 * i + 3);
    lo_synth_key(13, j.witness_key);
    j.generated_at = 4343;
    j.threads = 4;
    const size_t R = lo_job_rows(&j) - 3;
    std::vector<lo_fr> rows(R * (size_t)k), mc(k), ml(2 * (size_t)k), mq(2 * (size_t)k);
    std::vector<uint8_t> kinds(R);
    lo_form_rows(&j, rows.data(), mc.data(), ml.data(), mq.data());
    lo_row_kinds(&j, kinds.data());
    // the guest's witness: triple t has bit operands (t % 3 == 0), 8-byte operands (1), or the oracle's field elements with the
    // oracle's own z = x * y mod p (2); pads (slots l..k-1) stay as formed.  cls[r]: the width row r is shipped in without derivation
    uint64_t st = 0x9E3779B97F4A7C15ull;
    auto next = [&] { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    std::vector<uint8_t> cls(R, 32);
    size_t t = 0, first_z = 0;
    for (size_t r = 0; r < R; r++) {
        if (kinds[r] != 1) continue;
        lo_fr* x = rows.data() + r * (size_t)k;
        lo_fr* y = x + k;
        lo_fr* z = y + k;
        if (!first_z) first_z = r + 2;
        const int c = (int)(t++ % 3);
        if (c == 2) continue;
        for (uint32_t i = 0; i < l; i++) {
            std::memset(&x[i], 0, sizeof(lo_fr)); std::memset(&y[i], 0, sizeof(lo_fr)); std::memset(&z[i], 0, sizeof(lo_fr));
            x[i].v[0] = c == 0 ? (i == 0 ? 1 : next() & 1) : (i == 0 ? ~0ull : next());
            y[i].v[0] = c == 0 ? (i == 0 ? 1 : next() & 1) : (i == 0 ? ~0ull : next());
            const unsigned __int128 p = (unsigned __int128)x[i].v[0] * y[i].v[0];
            z[i].v[0] = (uint64_t)p; z[i].v[1] = (uint64_t)(p >> 64);
        }
        cls[r] = cls[r + 1] = c == 0 ? (uint8_t)LIG_ELEM_BIT : 8;
        cls[r + 2] = c == 0 ? (uint8_t)LIG_ELEM_BIT : 32;              // a product of two 8-byte words fits no narrow width
    }
    // what the guest hands over as z: garbage in the data slots (the true pads: they are the encoding stream either way)
    std::vector<lo_fr> junk(k);
    auto width_bytes = [&](uint8_t w) -> size_t { return w == 32 ? (size_t)k * 32 : w == LIG_ELEM_BIT ? ((size_t)l + 31) / 32 * 4 : (size_t)l * w; };

    // the statement: constraint s = data slot s (row-major), +1 * w = b_s
    const size_t S = R * (size_t)l;
    std::vector<uint32_t> term_begin(S + 1), rhs_c(S), rhs_b(S);
    std::vector<lig_lin_term> terms(S);
    std::vector<uint8_t> coefs(S * 32);
    for (size_t s = 0; s < S; s++) {
        term_begin[s] = (uint32_t)s;
        terms[s] = lig_lin_term{(uint32_t)s, LIG_COEF_ONE};
        rhs_c[s] = (uint32_t)s; rhs_b[s] = (uint32_t)s;
        std::memcpy(&coefs[32 * s], &rows[(s / l) * (size_t)k + s % l], 32);
    }
    term_begin[S] = (uint32_t)S;
    lig_linear_system sys;
    std::memset(&sys, 0, sizeof sys);
    sys.struct_bytes = sizeof sys;
    sys.n_constraints = S; sys.n_terms = S; sys.n_rhs = S; sys.n_coefs = S;
    sys.term_begin = term_begin.data(); sys.terms = terms.data(); sys.rhs_constraint = rhs_c.data(); sys.rhs_coef = rhs_b.data();
    sys.coefs = coefs.data();
    sys.first_random = 0;

    // this rank's rows (all of them on one GPU) and the bytes they take on the link, with and without the z rows
    std::vector<uint8_t> mine(R, world == 1);
    if (sharded) {
        uint64_t rounds = 0;
        std::vector<uint64_t> b((size_t)world * ((R + 511) / 512 + 2) + 2);
        if (lig_shard_rows_plan(kinds.data(), R, world, &rounds, b.data(), b.size()) != LIG_OK) { std::fprintf(stderr, "lig_shard_rows_plan failed\n"); return 1; }
        for (uint64_t g = rank; g < rounds * world; g += world) for (uint64_t r = b[g]; r < b[g + 1]; r++) mine[r] = 1;
    }
    size_t computed = 0, underived = 0, local_rows = 0, derived_rows = 0;
    for (size_t r = 0; r < R; r++) {
        if (!mine[r]) continue;
        local_rows++;
        underived += width_bytes(cls[r]);
        if (kinds[r] != 3) computed += width_bytes(cls[r]);
        else derived_rows++;
    }

    lig_ctx* ctx = nullptr;
    if (lig_ctx_create(&ctx, 0, l, k, n) != LIG_OK) { std::fprintf(stderr, "ctx: %s\n", ctx ? lig_last_error(ctx) : "?"); return 1; }
    lig_comm comm;
    if (sharded && lig_ipc_comm_create(ctx, argv[3], rank, world, &comm) != LIG_OK) { std::fprintf(stderr, "comm: %s\n", lig_last_error(ctx)); return 1; }
    int ok = 0;
    try {
        ligero::hip_proof_meta meta;
        std::memcpy(meta.encoding_seed, j.encoding_seed, 32);
        meta.generated_at = j.generated_at;
        meta.narrow_rows = true;
        meta.narrowest = true;
        meta.derive_products = true;
        auto at = [&](const std::vector<lo_fr>& v, size_t r) { return reinterpret_cast<const uint64_t*>(v.data() + r * (size_t)k); };
        auto replay = [&](ligero::hip_row_batcher& b, const std::vector<lo_fr>* rands) {
            for (size_t r = 0; r < R;) {
                if (kinds[r] == 0) { b.linear_callback(at(rows, r), rands ? at(*rands, r) : nullptr); r += 1; }
                else {
                    std::memcpy(junk.data(), rows.data() + (r + 2) * (size_t)k, (size_t)k * 32);
                    for (uint32_t i = 0; i < l; i++) junk[i].v[0] ^= 0x5555 + i, junk[i].v[2] = i;
                    b.quadratic_callback(at(rows, r), at(rows, r + 1), reinterpret_cast<const uint64_t*>(junk.data()), rands ? at(*rands, r) : nullptr,
                                         rands ? at(*rands, r + 1) : nullptr, rands ? at(*rands, r + 2) : nullptr);
                    r += 3;
                }
            }
            b.mask_callback(k, 2 * (size_t)k, 2 * (size_t)k);
        };
        int equals_oracle = 0, honest_valid = 0, linear_equals = 0, false_valid_linear = -1;
        size_t shipped = 0;
        std::vector<lo_fr> rands(R * (size_t)k);
        {   // part A
            ligero::hip_row_batcher b(ctx, meta);
            if (sharded) b.shard_over(rank, world, &comm);
            replay(b, nullptr);
            uint8_t root[32], seed1[32];
            b.commit(root, seed1);
            shipped = b.shipped_bytes();
            lo_fr cs;
            lo_rand_rows(&j, seed1, rands.data(), &cs);
            replay(b, &rands);
            size_t len = 0;
            lig_proof_info info;
            const uint8_t* proof = b.prove(nullptr, &len, &info);
            lo_proof P;
            if (lo_prove_rows(&j, kinds.data(), R, rows.data(), mc.data(), ml.data(), mq.data(), rands.data(), nullptr, &P) != 0)
                throw std::runtime_error("oracle prover failed");
            equals_oracle = len == P.proof_len && !std::memcmp(proof, P.proof, len) && !std::memcmp(root, P.root, 32) && P.valid_quad == 1 &&
                            local_rows == b.local_rows();
            lo_proof_free(&P);
        }
        {   // part B: the true statement as a term list, no second run of the guest
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_system(sys);
            if (sharded) b.shard_over(rank, world, &comm);
            replay(b, nullptr);
            uint8_t root[32], seed1[32];
            b.commit(root, seed1);
            size_t len = 0;
            lig_proof_info info;
            const uint8_t* proof = b.prove(nullptr, &len, &info);
            honest_valid = info.valid_code && info.valid_linear && info.valid_quad && b.shipped_bytes() == shipped;
            lo_fr cs;
            lo_rand_rows(&j, seed1, rands.data(), &cs);
            lo_proof P;
            if (lo_prove_rows(&j, kinds.data(), R, rows.data(), mc.data(), ml.data(), mq.data(), rands.data(), nullptr, &P) != 0)
                throw std::runtime_error("oracle prover failed");
            linear_equals = len == P.proof_len && !std::memcmp(proof, P.proof, len);
            lo_proof_free(&P);
        }
        {   // part C: the guest states z[5] + 1 for one slot of its first triple: the derived row holds the product, the constraint fails
            std::vector<uint8_t> lie = coefs;
            lie[32 * (first_z * (size_t)l + 5)] ^= 1;
            lig_linear_system bad = sys;
            bad.coefs = lie.data();
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_system(bad);
            if (sharded) b.shard_over(rank, world, &comm);
            replay(b, nullptr);
            uint8_t root[32], seed1[32];
            b.commit(root, seed1);
            size_t len = 0;
            lig_proof_info info;
            (void)b.prove(nullptr, &len, &info);
            false_valid_linear = info.valid_linear;
        }
        ok = equals_oracle && honest_valid && linear_equals && false_valid_linear == 0 && shipped == computed;
        std::printf("{\"rank\": %u, \"equals_oracle\": %s, \"local_rows\": %zu, \"derived_rows\": %zu, \"shipped_bytes\": %zu, \"computed_bytes\": %zu, \"underived_bytes\": %zu, "
                    "\"linear_honest_valid\": %s, \"linear_equals_oracle\": %s, \"linear_false_valid_linear\": %d}\n", rank, equals_oracle ? "true" : "false",
                    local_rows, derived_rows, shipped, computed, underived, honest_valid ? "true" : "false", linear_equals ? "true" : "false", false_valid_linear);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rank %u error: %s\n", rank, e.what());
    }
    if (sharded) lig_ipc_comm_destroy(&comm);
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
