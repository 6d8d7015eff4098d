// derived_slots_batcher_prog.cpp -- hip_row_batcher::set_derived_slots: the outputs of the guest's eval() calls are NOT computed by the
// driver; the library forms them from their defining constraints in commit() (lig_rows_set_derived).  The oracle plays guest +
// witness_manager (lo_form_rows: rows with their pads).  The shape is i32_add's: LINEAR row 0 is a bit row that carries 40 machine words,
// word c = sum_j 2^j * bit (row 1, column c + j), j < 33 -- the eval of a recomposition.  What the guest hands over at those 40 slots is 0,
// so row 0 ships as a pure bit row of ceil(l / 8) bytes; the expected bytes come from the oracle's prover over the TRUE rows.
//   part A  two passes, dense randomness rows: envelope == lo_prove_rows, shipped_bytes() == the figure computed here
//   part B  set_linear_system with the true statement (one constraint w[s] = b_s per data slot): valid, envelope == lo_prove_rows; then
//           reset() and the next proof of the same shape WITHOUT a second set_derived_slots: the list is kept, the same envelope
//   part C  a guest one of whose bits differs from the statement: the derived word moves with it and valid_linear == 0
//   part D  a batcher with shard_over() refuses the call, and shard_over() refuses a batcher that has a list
// Prints one JSON line.
// TEST CODE: links oracle/liblig_oracle.so as the checker.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../../include/lig_hip_row_batcher.hpp"
#include "../../oracle/lig_oracle.h"

int main() {
    const uint32_t l = 320, k = 512, n = 2048, WORDS = 40, BITS = 33;
    lo_job j;
    std::memset(&j, 0, sizeof j);
    j.l = l; j.k = k; j.n = n; j.t = 192;
    j.n_linear = 320 * 6;                             // full rows only (every row carries l constraints); linear rows come first
    j.n_quad = 320 * 2;
    for (int i = 0; i < 32; i++) j.encoding_seed[i] = (uint8_t)(3 * i + 7);
    lo_synth_key(17, j.witness_key);
    j.generated_at = 2222;
    j.threads = 4;
    const size_t R = lo_job_rows(&j) - 3;
    std::vector<lo_fr> rows(R * (size_t)k), mc(k), ml(2 * (size_t)k), mq(2 * (size_t)k);
    std::vector<uint8_t> kinds(R);
    lo_form_rows(&j, rows.data(), mc.data(), ml.data(), mq.data());
    lo_row_kinds(&j, kinds.data());
    if (R < 3 || kinds[0] != 0 || kinds[1] != 0) { std::fprintf(stderr, "unexpected row order\n"); return 1; }
    // the guest's witness: rows 0 and 1 are bits (pads stay as formed); then the 40 words of row 0 in integers
    uint64_t st = 0x9E3779B97F4A7C15ull;
    auto next = [&] { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    for (size_t r = 0; r < 2; r++)
        for (uint32_t i = 0; i < l; i++) { std::memset(&rows[r * k + i], 0, sizeof(lo_fr)); rows[r * k + i].v[0] = next() & 1; }
    for (uint32_t i = 0; i < BITS; i++) rows[k + i].v[0] = 1;                    // word 0 = 2^33 - 1
    auto word = [&](const std::vector<lo_fr>& m, uint32_t c) { uint64_t v = 0; for (uint32_t b = 0; b < BITS; b++) v |= (m[k + c + b].v[0] & 1) << b; return v; };
    for (uint32_t c = 0; c < WORDS; c++) rows[c].v[0] = word(rows, c);
    // the defining constraints: sum_j 2^j * w[row 1, c + j] - w[row 0, c] = 0
    std::vector<uint32_t> d_begin(WORDS + 1);
    std::vector<lig_lin_term> d_terms;
    std::vector<uint8_t> d_coefs(BITS * 32, 0);
    std::vector<lig_derived_slot> list(WORDS);
    for (uint32_t b = 0; b < BITS; b++) d_coefs[32 * b + b / 8] = (uint8_t)(1u << (b % 8));
    for (uint32_t c = 0; c < WORDS; c++) {
        d_begin[c] = (uint32_t)d_terms.size();
        for (uint32_t b = 0; b < BITS; b++) d_terms.push_back(lig_lin_term{l + c + b, b});
        d_terms.push_back(lig_lin_term{c, LIG_COEF_NEG_ONE});
        list[WORDS - 1 - c] = lig_derived_slot{c, c};                            // any order
    }
    d_begin[WORDS] = (uint32_t)d_terms.size();
    lig_linear_system dsys;
    std::memset(&dsys, 0, sizeof dsys);
    dsys.struct_bytes = sizeof dsys;
    dsys.n_constraints = WORDS; dsys.n_terms = d_terms.size(); dsys.n_coefs = BITS;
    dsys.term_begin = d_begin.data(); dsys.terms = d_terms.data(); dsys.coefs = d_coefs.data();

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

    // what the guest hands over: the true rows with 0 at the 40 derived slots
    std::vector<lo_fr> guest = rows;
    for (uint32_t c = 0; c < WORDS; c++) std::memset(&guest[c], 0, sizeof(lo_fr));
    const size_t bit_row = ((size_t)l + 31) / 32 * 4;
    const size_t computed = 2 * bit_row + (R - 2) * (size_t)k * 32, underived = (size_t)l * 8 + bit_row + (R - 2) * (size_t)k * 32;

    lig_ctx* ctx = nullptr;
    if (lig_ctx_create(&ctx, 0, l, k, n) != LIG_OK) { std::fprintf(stderr, "ctx: %s\n", ctx ? lig_last_error(ctx) : "?"); return 1; }
    int ok = 0;
    try {
        ligero::hip_proof_meta meta;
        std::memcpy(meta.encoding_seed, j.encoding_seed, 32);
        meta.generated_at = j.generated_at;
        meta.narrow_rows = true;
        meta.narrowest = true;
        auto at = [&](const std::vector<lo_fr>& v, size_t r) { return reinterpret_cast<const uint64_t*>(v.data() + r * (size_t)k); };
        auto replay = [&](ligero::hip_row_batcher& b, const std::vector<lo_fr>& from, const std::vector<lo_fr>* rands) {
            for (size_t r = 0; r < R;) {
                if (kinds[r] == 0) { b.linear_callback(at(from, r), rands ? at(*rands, r) : nullptr); r += 1; }
                else {
                    b.quadratic_callback(at(from, r), at(from, r + 1), at(from, r + 2), rands ? at(*rands, r) : nullptr,
                                         rands ? at(*rands, r + 1) : nullptr, rands ? at(*rands, r + 2) : nullptr);
                    r += 3;
                }
            }
            b.mask_callback(k, 2 * (size_t)k, 2 * (size_t)k);
        };
        auto oracle_equal = [&](const uint8_t seed1[32], const uint8_t* proof, size_t len, const uint8_t* root) {
            std::vector<lo_fr> rands(R * (size_t)k);
            lo_fr cs;
            lo_rand_rows(&j, seed1, rands.data(), &cs);
            lo_proof P;
            if (lo_prove_rows(&j, kinds.data(), R, rows.data(), mc.data(), ml.data(), mq.data(), rands.data(), nullptr, &P) != 0)
                throw std::runtime_error("oracle prover failed");
            const int eq = len == P.proof_len && !std::memcmp(proof, P.proof, len) && (!root || !std::memcmp(root, P.root, 32));
            lo_proof_free(&P);
            return eq;
        };
        int equals_oracle = 0, honest_valid = 0, linear_equals = 0, kept_over_reset = 0, false_valid_linear = -1, refused = 0;
        size_t shipped = 0;
        {   // part A
            ligero::hip_row_batcher b(ctx, meta);
            b.set_derived_slots(dsys, list.data(), list.size());
            replay(b, guest, nullptr);
            uint8_t root[32], seed1[32];
            b.commit(root, seed1);
            shipped = b.shipped_bytes();
            std::vector<lo_fr> rands(R * (size_t)k);
            lo_fr cs;
            lo_rand_rows(&j, seed1, rands.data(), &cs);
            replay(b, guest, &rands);
            size_t len = 0;
            lig_proof_info info;
            const uint8_t* proof = b.prove(nullptr, &len, &info);
            equals_oracle = oracle_equal(seed1, proof, len, root);
        }
        {   // part B
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_system(sys);
            b.set_derived_slots(dsys, list.data(), list.size());
            for (int rep = 0; rep < 2; rep++) {
                if (rep) b.reset();
                replay(b, guest, nullptr);
                uint8_t root[32], seed1[32];
                b.commit(root, seed1);
                size_t len = 0;
                lig_proof_info info;
                const uint8_t* proof = b.prove(nullptr, &len, &info);
                const int valid = info.valid_code && info.valid_linear && info.valid_quad && b.shipped_bytes() == shipped;
                const int eq = oracle_equal(seed1, proof, len, root);
                if (!rep) { honest_valid = valid; linear_equals = eq; } else kept_over_reset = valid && eq;
            }
        }
        {   // part C: bit 3 of word 5 flipped in what the guest hands over; the statement still names the old word
            std::vector<lo_fr> moved = guest;
            moved[k + 5 + 3].v[0] ^= 1;
            std::vector<uint8_t> stated = coefs;                                  // ... and the bit as handed over, so that only the WORDS disagree
            stated[32 * ((size_t)l + 5 + 3)] ^= 1;
            lig_linear_system claim = sys;
            claim.coefs = stated.data();
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_system(claim);
            b.set_derived_slots(dsys, list.data(), list.size());
            replay(b, moved, nullptr);
            uint8_t root[32], seed1[32];
            b.commit(root, seed1);
            size_t len = 0;
            lig_proof_info info;
            (void)b.prove(nullptr, &len, &info);
            false_valid_linear = info.valid_linear;
        }
        {   // part D
            lig_comm comm;
            std::memset(&comm, 0, sizeof comm);
            ligero::hip_row_batcher b(ctx, meta);
            b.shard_over(0, 1, &comm);
            try { b.set_derived_slots(dsys, list.data(), list.size()); } catch (const std::logic_error&) { refused++; }
            ligero::hip_row_batcher b2(ctx, meta);
            b2.set_derived_slots(dsys, list.data(), list.size());
            try { b2.shard_over(0, 1, &comm); } catch (const std::logic_error&) { refused++; }
        }
        ok = equals_oracle && honest_valid && linear_equals && kept_over_reset && false_valid_linear == 0 && refused == 2 && shipped == computed && shipped < underived;
        std::printf("{\"equals_oracle\": %s, \"derived_slots\": %u, \"shipped_bytes\": %zu, \"computed_bytes\": %zu, \"underived_bytes\": %zu, "
                    "\"linear_honest_valid\": %s, \"linear_equals_oracle\": %s, \"kept_over_reset\": %s, \"linear_false_valid_linear\": %d, \"sharded_refusals\": %d}\n",
                    equals_oracle ? "true" : "false", WORDS, shipped, computed, underived, honest_valid ? "true" : "false", linear_equals ? "true" : "false",
                    kept_over_reset ? "true" : "false", false_valid_linear, refused);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
    }
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
