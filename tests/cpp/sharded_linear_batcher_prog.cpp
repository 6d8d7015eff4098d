// sharded_linear_batcher_prog.cpp -- hip_row_batcher::shard_over together with set_linear_system: ONE guest trace proved by `world`
// processes (here all on GPU 0, communicator of csrc/comm_ipc.hip), every rank hands the batcher the term list of the WHOLE trace, runs
// the guest ONCE (no pass-2 callbacks) and calls prove(nullptr).  Every rank must end with the envelope of the unsharded batcher with the
// same system, which is the oracle's envelope: the system is the statement of the oracle's synthetic stream (one constraint w[s] = b_s
// per witness slot, as in linear_batcher_prog.cpp).   usage: sharded_linear_batcher_prog rank world /shm_name
// Prints one JSON line: {"rank", "equal_unsharded", "equal_oracle", "const_equal", "valid", "second_proof_equal", "local_rows"}.
// TEST CODE: links oracle/liblig_oracle.so as the guest and the checker.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/lig_hip_row_batcher.hpp"
#include "../../oracle/lig_oracle.h"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const uint32_t rank = std::atoi(argv[1]), world = std::atoi(argv[2]);
    const uint32_t l = 320, k = 512, n = 2048;
    lo_job j;
    std::memset(&j, 0, sizeof j);
    j.l = l; j.k = k; j.n = n; j.t = 192;
    j.n_linear = 320 * 5;                             // full rows only: every row carries l constraints
    j.n_quad = 320 * 2;
    for (int i = 0; i < 32; i++) j.encoding_seed[i] = (uint8_t)(7 * i + 1);
    lo_synth_key(11, j.witness_key);
    j.generated_at = 777;
    j.threads = 4;
    const size_t R = lo_job_rows(&j) - 3;
    std::vector<lo_fr> rows(R * (size_t)k), mc(k), ml(2 * (size_t)k), mq(2 * (size_t)k);
    std::vector<uint8_t> kinds(R);
    lo_form_rows(&j, rows.data(), mc.data(), ml.data(), mq.data());
    lo_row_kinds(&j, kinds.data());
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
    if (lig_linear_check(&sys, kinds.data(), R, l) != LIG_OK) { std::fprintf(stderr, "lig_linear_check rejects the system\n"); return 1; }

    lig_ctx* ctx = nullptr;
    if (lig_ctx_create(&ctx, 0, l, k, n) != LIG_OK) { std::fprintf(stderr, "ctx: %s\n", ctx ? lig_last_error(ctx) : "?"); return 1; }
    lig_comm comm;
    if (lig_ipc_comm_create(ctx, argv[3], rank, world, &comm) != LIG_OK) { std::fprintf(stderr, "comm: %s\n", lig_last_error(ctx)); return 1; }
    int ok = 0;
    try {
        ligero::hip_proof_meta meta;
        std::memcpy(meta.encoding_seed, j.encoding_seed, 32);
        meta.generated_at = j.generated_at;
        auto at = [&](size_t r) { return reinterpret_cast<const uint64_t*>(rows.data() + r * (size_t)k); };
        auto pass1 = [&](ligero::hip_row_batcher& b) {      // the guest's only run: no randomness rows anywhere
            for (size_t r = 0; r < R;) {
                if (kinds[r] == 0) { b.linear_callback(at(r)); r += 1; }
                else { b.quadratic_callback(at(r), at(r + 1), at(r + 2)); r += 3; }
            }
            b.mask_callback(k, 2 * (size_t)k, 2 * (size_t)k);
        };
        std::vector<uint8_t> unsharded;
        uint8_t root_u[32], seed_u[32];
        {
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_system(sys);
            pass1(b);
            b.commit(root_u, seed_u);
            size_t len = 0;
            const uint8_t* proof = b.prove(nullptr, &len);
            unsharded.assign(proof, proof + len);
        }
        lo_proof P;
        if (lo_prove(&j, &P) != 0) throw std::runtime_error("oracle prover failed");
        std::vector<lo_fr> dense(R * (size_t)k);
        lo_fr cs;
        lo_rand_rows(&j, P.stage1_seed, dense.data(), &cs);     // (only its constant is used)
        int equal_u = 0, equal_o = 0, const_equal = 0, valid = 0, again = 0;
        size_t local = 0;
        {
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_system(sys);                   // before shard_over: both orders are allowed
            b.shard_over(rank, world, &comm);
            pass1(b);
            uint8_t root[32], seed1[32];
            b.commit(root, seed1);
            size_t len = 0;
            lig_proof_info info;
            const uint8_t* proof = b.prove(nullptr, &len, &info);
            equal_u = len == unsharded.size() && !std::memcmp(proof, unsharded.data(), len) && !std::memcmp(root, root_u, 32) && !std::memcmp(seed1, seed_u, 32);
            equal_o = len == P.proof_len && !std::memcmp(proof, P.proof, len) && !std::memcmp(root, P.root, 32);
            const_equal = !std::memcmp(info.const_sum, &cs, 32);
            valid = info.valid_code && info.valid_linear && info.valid_quad;
            local = b.local_rows();
            // the next proof of the same program, the system given after shard_over this time
            b.reset();
            b.set_linear_system(sys);
            pass1(b);
            b.commit(root, seed1);
            proof = b.prove(nullptr, &len, &info);
            again = len == unsharded.size() && !std::memcmp(proof, unsharded.data(), len) && info.valid_linear;
        }       // the batcher (and its shard) goes before the communicator
        lo_proof_free(&P);
        ok = equal_u && equal_o && const_equal && valid && again;
        auto tf = [](int v) { return v ? "true" : "false"; };
        std::printf("{\"rank\": %u, \"equal_unsharded\": %s, \"equal_oracle\": %s, \"const_equal\": %s, \"valid\": %s, \"second_proof_equal\": %s, \"local_rows\": %zu}\n",
                    rank, tf(equal_u), tf(equal_o), tf(const_equal), tf(valid), tf(again), local);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rank %u error: %s\n", rank, e.what());
    }
    lig_ipc_comm_destroy(&comm);
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
