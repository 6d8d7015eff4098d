// shard_derived_slots_batcher_prog.cpp -- hip_row_batcher::shard_set_derived_slots on a batcher with shard_over(): ONE guest trace proved by
// `world` = 2 processes (both on GPU 0, communicator of csrc/comm_ipc.hip); the outputs of the guest's eval() calls are NOT computed by the
// driver, every rank forms the ones on its own rows in commit() (lig_shard_rows_set_derived).  The oracle plays guest + witness_manager
// (lo_form_rows).  20 rows, dealt 0..9 | 10..19.  LINEAR row 0 (rank 0) is a bit row that carries 40 machine words: word c = sum_j 2^j * bit
// (row 1, column c + j) for c < 20 -- bits of rank 0's own rows -- and of (row 10, column c + j) for c >= 20 -- bits rank 1 holds, which
// travel in the one all-gather of the list's only wave.  What the guest hands over at the 40 slots is 0; the expected bytes come from the
// oracle's prover over the TRUE rows.     usage: shard_derived_slots_batcher_prog rank world /shm_name
//   part A  set_linear_system with the true statement (one constraint w[s] = b_s per data slot) + shard_set_derived_slots: valid, envelope
//           == lo_prove_rows; then reset() and the next proof WITHOUT a second shard_set_derived_slots: the list is kept, the same envelope
//   part B  a guest one of whose bits ON THE OTHER RANK differs from the statement: the derived word moves with it and valid_linear == 0
//   part C  an unsharded batcher refuses the call
// Prints one JSON line.
// TEST CODE: links oracle/liblig_oracle.so as the checker.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../../include/lig_hip_row_batcher.hpp"
#include "../../oracle/lig_oracle.h"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const uint32_t rank = std::atoi(argv[1]), world = std::atoi(argv[2]);
    const uint32_t l = 320, k = 512, n = 2048, WORDS = 40, BITS = 33, FAR = 10;
    lo_job j;
    std::memset(&j, 0, sizeof j);
    j.l = l; j.k = k; j.n = n; j.t = 192;
    j.n_linear = 320 * 14;                            // full rows only (every row carries l constraints); linear rows come first
    j.n_quad = 320 * 2;
    for (int i = 0; i < 32; i++) j.encoding_seed[i] = (uint8_t)(5 * i + 3);
    lo_synth_key(19, j.witness_key);
    j.generated_at = 2323;
    j.threads = 4;
    const size_t R = lo_job_rows(&j) - 3;
    std::vector<lo_fr> rows(R * (size_t)k), mc(k), ml(2 * (size_t)k), mq(2 * (size_t)k);
    std::vector<uint8_t> kinds(R);
    lo_form_rows(&j, rows.data(), mc.data(), ml.data(), mq.data());
    lo_row_kinds(&j, kinds.data());
    uint64_t rounds = 0, bnd[8];
    if (R != 20 || kinds[0] != 0 || kinds[1] != 0 || kinds[FAR] != 0) { std::fprintf(stderr, "unexpected row order\n"); return 1; }
    if (world != 2 || lig_shard_rows_plan(kinds.data(), R, world, &rounds, bnd, 8) != LIG_OK || rounds != 1 || bnd[1] != FAR) { std::fprintf(stderr, "unexpected deal\n"); return 1; }
    // the guest's witness: rows 0, 1 and 10 are bits (pads stay as formed); then the 40 words of row 0 in integers
    uint64_t st = 0x9E3779B97F4A7C15ull;
    auto next = [&] { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    for (size_t r : {(size_t)0, (size_t)1, (size_t)FAR})
        for (uint32_t i = 0; i < l; i++) { std::memset(&rows[r * k + i], 0, sizeof(lo_fr)); rows[r * k + i].v[0] = next() & 1; }
    auto bits_row = [&](uint32_t c) { return c < WORDS / 2 ? (size_t)1 : (size_t)FAR; };
    auto word = [&](const std::vector<lo_fr>& m, uint32_t c) { uint64_t v = 0; for (uint32_t b = 0; b < BITS; b++) v |= (m[bits_row(c) * k + c + b].v[0] & 1) << b; return v; };
    for (uint32_t c = 0; c < WORDS; c++) rows[c].v[0] = word(rows, c);
    // the defining constraints: sum_j 2^j * w[bits row, c + j] - w[row 0, c] = 0
    std::vector<uint32_t> d_begin(WORDS + 1);
    std::vector<lig_lin_term> d_terms;
    std::vector<uint8_t> d_coefs(BITS * 32, 0);
    std::vector<lig_derived_slot> list(WORDS);
    for (uint32_t b = 0; b < BITS; b++) d_coefs[32 * b + b / 8] = (uint8_t)(1u << (b % 8));
    for (uint32_t c = 0; c < WORDS; c++) {
        d_begin[c] = (uint32_t)d_terms.size();
        for (uint32_t b = 0; b < BITS; b++) d_terms.push_back(lig_lin_term{(uint32_t)bits_row(c) * l + c + b, b});
        d_terms.push_back(lig_lin_term{c, LIG_COEF_NEG_ONE});
        list[WORDS - 1 - c] = lig_derived_slot{c, c};                            // any order
    }
    d_begin[WORDS] = (uint32_t)d_terms.size();
    lig_linear_system dsys;
    std::memset(&dsys, 0, sizeof dsys);
    dsys.struct_bytes = sizeof dsys;
    dsys.n_constraints = WORDS; dsys.n_terms = d_terms.size(); dsys.n_coefs = BITS;
    dsys.term_begin = d_begin.data(); dsys.terms = d_terms.data(); dsys.coefs = d_coefs.data();
    // what the ranks are about to exchange, from the host-only count: one wave, one all-gather of the 52 distinct bits of row 10
    lig_derived_shard_info cnt[2];
    for (uint32_t q = 0; q < 2; q++) {
        std::memset(&cnt[q], 0, sizeof cnt[q]);
        cnt[q].struct_bytes = sizeof cnt[q];
        if (lig_derived_shard_count(&dsys, kinds.data(), R, l, nullptr, list.data(), list.size(), q, world, &cnt[q]) != LIG_OK) { std::fprintf(stderr, "count refused\n"); return 1; }
    }
    const uint64_t far_bits = WORDS / 2 + BITS - 1;                               // columns 20 .. 71 of row 10
    const int counted = cnt[0].n_waves == 1 && cnt[0].n_exchanges == 1 && cnt[0].local_targets == WORDS && cnt[1].local_targets == 0 &&
                        cnt[0].imported_terms == (uint64_t)(WORDS / 2) * BITS && cnt[0].imports == far_bits && cnt[1].exports == far_bits &&
                        cnt[0].exchange_bytes == 32 * 2 * far_bits && cnt[1].exchange_bytes == cnt[0].exchange_bytes;

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

    lig_ctx* ctx = nullptr;
    if (lig_ctx_create(&ctx, 0, l, k, n) != LIG_OK) { std::fprintf(stderr, "ctx: %s\n", ctx ? lig_last_error(ctx) : "?"); return 1; }
    lig_comm comm;
    if (lig_ipc_comm_create(ctx, argv[3], rank, world, &comm) != LIG_OK) { std::fprintf(stderr, "comm: %s\n", lig_last_error(ctx)); return 1; }
    int ok = 0;
    try {
        ligero::hip_proof_meta meta;
        std::memcpy(meta.encoding_seed, j.encoding_seed, 32);
        meta.generated_at = j.generated_at;
        meta.narrow_rows = true;
        meta.narrowest = true;
        auto at = [&](const std::vector<lo_fr>& v, size_t r) { return reinterpret_cast<const uint64_t*>(v.data() + r * (size_t)k); };
        auto replay = [&](ligero::hip_row_batcher& b, const std::vector<lo_fr>& from) {      // the guest's only run: no randomness rows anywhere
            for (size_t r = 0; r < R;) {
                if (kinds[r] == 0) { b.linear_callback(at(from, r)); r += 1; }
                else { b.quadratic_callback(at(from, r), at(from, r + 1), at(from, r + 2)); r += 3; }
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
            const int eq = len == P.proof_len && !std::memcmp(proof, P.proof, len) && !std::memcmp(root, P.root, 32);
            lo_proof_free(&P);
            return eq;
        };
        int honest_valid = 0, equals_oracle = 0, kept_over_reset = 0, false_valid_linear = -1, refused = 0;
        size_t local = 0;
        {   // part A
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_system(sys);
            b.shard_over(rank, world, &comm);
            b.shard_set_derived_slots(dsys, list.data(), list.size());
            for (int rep = 0; rep < 2; rep++) {
                if (rep) b.reset();
                replay(b, guest);
                uint8_t root[32], seed1[32];
                b.commit(root, seed1);
                size_t len = 0;
                lig_proof_info info;
                const uint8_t* proof = b.prove(nullptr, &len, &info);
                const int valid = info.valid_code && info.valid_linear && info.valid_quad;
                const int eq = oracle_equal(seed1, proof, len, root);
                if (!rep) { honest_valid = valid; equals_oracle = eq; local = b.local_rows(); } else kept_over_reset = valid && eq;
            }
        }
        {   // part B: bit 3 of word 25 -- a bit of row 10, which rank 1 holds -- flipped in what the guest hands over; the statement still names the old word
            std::vector<lo_fr> moved = guest;
            moved[(size_t)FAR * k + 25 + 3].v[0] ^= 1;
            std::vector<uint8_t> stated = coefs;                                  // ... and the bit as handed over, so that only the WORDS disagree
            stated[32 * ((size_t)FAR * l + 25 + 3)] ^= 1;
            lig_linear_system claim = sys;
            claim.coefs = stated.data();
            ligero::hip_row_batcher b(ctx, meta);
            b.shard_over(rank, world, &comm);
            b.set_linear_system(claim);
            b.shard_set_derived_slots(dsys, list.data(), list.size());
            replay(b, moved);
            uint8_t root[32], seed1[32];
            b.commit(root, seed1);
            size_t len = 0;
            lig_proof_info info;
            (void)b.prove(nullptr, &len, &info);
            false_valid_linear = info.valid_linear;
        }
        {   // part C
            ligero::hip_row_batcher b(ctx, meta);
            try { b.shard_set_derived_slots(dsys, list.data(), list.size()); } catch (const std::logic_error&) { refused++; }
        }
        ok = counted && honest_valid && equals_oracle && kept_over_reset && false_valid_linear == 0 && refused == 1;
        auto tf = [](int v) { return v ? "true" : "false"; };
        std::printf("{\"rank\": %u, \"counted\": %s, \"honest_valid\": %s, \"equals_oracle\": %s, \"kept_over_reset\": %s, \"false_valid_linear\": %d, "
                    "\"unsharded_refusals\": %d, \"local_rows\": %zu, \"exchange_bytes\": %llu}\n",
                    rank, tf(counted), tf(honest_valid), tf(equals_oracle), tf(kept_over_reset), false_valid_linear, refused, local, (unsigned long long)cnt[0].exchange_bytes);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rank %u error: %s\n", rank, e.what());
    }
    lig_ipc_comm_destroy(&comm);
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
