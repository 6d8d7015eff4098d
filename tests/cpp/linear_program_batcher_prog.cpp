// linear_program_batcher_prog.cpp -- hip_row_batcher::set_linear_program / set_linear_values and the same on hip_row_verifier: ONE
// lig_linear_program (lig_linear_prepare) feeds a batcher through two proofs around a reset() -- the second a new statement of the
// same program, its right-hand sides given as values of the coefficient table -- and a verifier through both envelopes.  The
// envelopes must be those of the set_linear_system path (one batcher per statement, each with a system of its own).
// The system is the statement of the oracle's synthetic stream: one constraint w[s] = b_s per witness slot in commit order
// (a single +1 term; b_s, the witness value, in the table).  The second statement changes witnesses of the first row, hence b_s.
// Prints one JSON line: {"first_equal", "second_equal", "valid", "verifier_accepts", "wrong_values_rejected", "rows"}.
// TEST CODE: links oracle/liblig_oracle.so as the guest (rows with their pads).
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
    std::vector<uint8_t> coefs(S * 32), coefs2;
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

    // the second statement: other witnesses in 40 slots of row 0 (a LINEAR row), the table follows
    std::vector<lo_fr> rows2 = rows;
    if (kinds[0] != 0) { std::fprintf(stderr, "row 0 is not a linear row\n"); return 1; }
    for (size_t s = 0; s < 40; s++) {
        const uint64_t v[4] = {0x1234567ull * (s + 1), s, 0, 0};
        std::memcpy(&rows2[s * 3], v, 32);
    }
    coefs2 = coefs;
    for (size_t s = 0; s < l; s++) std::memcpy(&coefs2[32 * s], &rows2[s], 32);
    lig_linear_system sys2 = sys;
    sys2.coefs = coefs2.data();

    lig_ctx* ctx = nullptr;
    if (lig_ctx_create(&ctx, 0, l, k, n) != LIG_OK) { std::fprintf(stderr, "ctx: %s\n", ctx ? lig_last_error(ctx) : "?"); return 1; }
    int ok = 0;
    lig_linear_program* prog = nullptr;
    try {
        ligero::hip_proof_meta meta;
        std::memcpy(meta.encoding_seed, j.encoding_seed, 32);
        meta.generated_at = j.generated_at;
        auto at = [&](const std::vector<lo_fr>& v, size_t r) { return reinterpret_cast<const uint64_t*>(v.data() + r * (size_t)k); };
        auto replay = [&](ligero::hip_row_batcher& b, const std::vector<lo_fr>& w) {
            for (size_t r = 0; r < R;) {
                if (kinds[r] == 0) { b.linear_callback(at(w, r)); r += 1; }
                else { b.quadratic_callback(at(w, r), at(w, r + 1), at(w, r + 2)); r += 3; }
            }
            b.mask_callback(k, 2 * (size_t)k, 2 * (size_t)k);
        };
        uint8_t root[32], seed1[32];
        // the yardstick: one batcher and one system per statement
        std::vector<uint8_t> want[2];
        for (int i = 0; i < 2; i++) {
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_system(i ? sys2 : sys);
            replay(b, i ? rows2 : rows);
            b.commit(root, seed1);
            size_t len = 0;
            lig_proof_info info;
            const uint8_t* proof = b.prove(nullptr, &len, &info);
            if (!info.valid_linear) throw std::runtime_error("the set_linear_system path fails its own linear check");
            want[i].assign(proof, proof + len);
        }
        if (want[0] == want[1]) throw std::runtime_error("the two statements give the same envelope");
        if (lig_linear_prepare(ctx, &sys, kinds.data(), R, &prog) != LIG_OK) throw std::runtime_error(std::string("lig_linear_prepare: ") + lig_last_error(ctx));
        int first = 0, second = 0, valid = 0;
        {
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_program(prog);
            replay(b, rows);
            b.commit(root, seed1);
            size_t len = 0;
            lig_proof_info info;
            const uint8_t* proof = b.prove(nullptr, &len, &info);
            first = len == want[0].size() && !std::memcmp(proof, want[0].data(), len);
            valid = info.valid_code && info.valid_linear && info.valid_quad;
            // the next statement of the same program: same shape, the attachment stays, only the values change
            b.reset();
            b.set_linear_values(coefs2.data(), S);
            replay(b, rows2);
            b.commit(root, seed1);
            proof = b.prove(nullptr, &len, &info);
            second = len == want[1].size() && !std::memcmp(proof, want[1].data(), len);
            valid = valid && info.valid_code && info.valid_linear && info.valid_quad;
        }
        // the verifier shim: one program, both envelopes, the values of the second statement on the second
        ligero::hip_row_verifier v(ctx, meta);
        v.expect_rows(kinds);
        v.set_linear_program(prog);
        uint8_t vseed[32];
        lig_verify_info vi;
        bool accepts = v.begin(want[0].data(), want[0].size(), vseed) && v.finish(nullptr, &vi) && vi.valid_linear && vi.linear_equal;
        // the second envelope against the program's own table: another statement
        const bool wrong = v.begin(want[1].data(), want[1].size(), vseed) && !v.finish(nullptr, &vi) && !vi.valid_linear && vi.valid_merkle;
        v.set_linear_values(coefs2.data(), S);
        accepts = accepts && v.begin(want[1].data(), want[1].size(), vseed) && v.finish(nullptr, &vi) && vi.valid_linear && vi.linear_equal;
        ok = first && second && valid && accepts && wrong;
        std::printf("{\"first_equal\": %s, \"second_equal\": %s, \"valid\": %s, \"verifier_accepts\": %s, \"wrong_values_rejected\": %s, \"rows\": %zu}\n",
                    first ? "true" : "false", second ? "true" : "false", valid ? "true" : "false", accepts ? "true" : "false", wrong ? "true" : "false", R);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
    }
    lig_linear_program_release(prog);
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
