// linear_batcher_prog.cpp -- hip_row_batcher::set_linear_system / hip_row_verifier::set_linear_system: the row-batching shim with the
// program's linear constraints as a sparse term list and NO pass-2 callbacks produces the envelope the two-pass shim produces from
// the dense randomness rows of the same system, and the verifier shim accepts it without a run of the guest.
// The system is the statement of the oracle's synthetic stream: one constraint w[s] = b_s per witness slot in commit order
// (a single +1 term; b_s, the witness value, in the table), so its randomness rows are the stream's dense rows (lo_rand_rows).
// Prints one JSON line: {"equal_envelopes", "valid_linear", "const_equal", "verifier_accepts", "rows"}.
// TEST CODE: links oracle/liblig_oracle.so as the guest (rows with their pads) and for the dense rows of the two-pass run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/lig_hip_row_batcher.hpp"
#include "../../oracle/lig_oracle.h"

int main() {
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
    // the term list: constraint c = slot c (row-major over the data slots), +1 * w = b with b in the table
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
    if (lig_linear_check(&sys, kinds.data(), R, l) != LIG_OK) { std::fprintf(stderr, "lig_linear_check rejects the system\n"); return 1; }

    lig_ctx* ctx = nullptr;
    if (lig_ctx_create(&ctx, 0, l, k, n) != LIG_OK) { std::fprintf(stderr, "ctx: %s\n", ctx ? lig_last_error(ctx) : "?"); return 1; }
    int ok = 0;
    try {
        ligero::hip_proof_meta meta;
        std::memcpy(meta.encoding_seed, j.encoding_seed, 32);
        meta.generated_at = j.generated_at;
        auto at = [&](const std::vector<lo_fr>& v, size_t r) { return reinterpret_cast<const uint64_t*>(v.data() + r * (size_t)k); };
        auto replay = [&](ligero::hip_row_batcher& b, const std::vector<lo_fr>* rands) {
            for (size_t r = 0; r < R;) {
                if (kinds[r] == 0) { b.linear_callback(at(rows, r), rands ? at(*rands, r) : nullptr); r += 1; }
                else {
                    b.quadratic_callback(at(rows, r), at(rows, r + 1), at(rows, r + 2), rands ? at(*rands, r) : nullptr,
                                         rands ? at(*rands, r + 1) : nullptr, rands ? at(*rands, r + 2) : nullptr);
                    r += 3;
                }
            }
            b.mask_callback(k, 2 * (size_t)k, 2 * (size_t)k);
        };
        // the two-pass shim: dense randomness rows and the constant from the guest's second run
        std::vector<uint8_t> two_pass;
        uint8_t seed_a[32], root_a[32];
        lo_fr cs;
        {
            ligero::hip_row_batcher b(ctx, meta);
            replay(b, nullptr);
            b.commit(root_a, seed_a);
            std::vector<lo_fr> rands(R * (size_t)k);
            lo_rand_rows(&j, seed_a, rands.data(), &cs);
            replay(b, &rands);
            size_t len = 0;
            const uint8_t* proof = b.prove(reinterpret_cast<const uint8_t*>(&cs), &len);
            two_pass.assign(proof, proof + len);
        }
        // the one-pass shim: the term list, no second run, no constant
        int equal = 0, const_equal = 0, valid_linear = 0, again = 0;
        {
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_system(sys);
            replay(b, nullptr);
            uint8_t root[32], seed1[32];
            b.commit(root, seed1);
            size_t len = 0;
            lig_proof_info info;
            const uint8_t* proof = b.prove(nullptr, &len, &info);
            equal = len == two_pass.size() && !std::memcmp(proof, two_pass.data(), len) && !std::memcmp(root, root_a, 32) && !std::memcmp(seed1, seed_a, 32);
            const_equal = !std::memcmp(info.const_sum, &cs, 32);
            valid_linear = info.valid_code && info.valid_linear && info.valid_quad;
            // the next proof of the same program: the structure stays resident on the trace
            b.reset();
            replay(b, nullptr);
            b.commit(root, seed1);
            proof = b.prove(nullptr, &len, &info);
            again = len == two_pass.size() && !std::memcmp(proof, two_pass.data(), len) && info.valid_linear;
        }
        // the verifier shim: the envelope and the public structure, nothing else
        ligero::hip_row_verifier v(ctx, meta);
        v.expect_rows(kinds);
        v.set_linear_system(sys);
        uint8_t vseed[32];
        lig_verify_info vi;
        const bool accepts = v.begin(two_pass.data(), two_pass.size(), vseed) && v.finish(nullptr, &vi) && vi.valid_linear && vi.linear_equal;
        ok = equal && const_equal && valid_linear && again && accepts;
        std::printf("{\"equal_envelopes\": %s, \"const_equal\": %s, \"valid_linear\": %s, \"second_proof_equal\": %s, \"verifier_accepts\": %s, \"rows\": %zu}\n",
                    equal ? "true" : "false", const_equal ? "true" : "false", valid_linear ? "true" : "false", again ? "true" : "false",
                    accepts ? "true" : "false", R);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
    }
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
