// derived_products_batcher_prog.cpp -- hip_row_batcher::set_derived_slots with PRODUCT ENTRIES (hip_row_batcher::product_entry,
// LIG_DERIVED_PRODUCT): the guest  t = eval(a + b); u = t * c; v = eval(u + d)  in 40 columns.  The driver computes none of t, u, v: t is
// column i of the x row of the first triple, u of its z row (derive_products: not shipped), v of LINEAR row 3; a, b, d are columns of
// LINEAR rows 0, 1, 2 and c the y row.  The list: t with its constraint (wave 1), u as a product entry (wave 2), v with its constraint
// (wave 3).  The oracle plays guest + witness_manager (lo_form_rows: rows with their pads); the expected bytes come from the oracle's
// prover over the TRUE rows, the expected values of t, u, v from 64-bit integers here.  One pass with set_linear_system (the statement
// w[s] = b_s per data slot): valid, envelope == lo_prove_rows, read_slots == the integers.  Prints one JSON line.
// TEST CODE: links oracle/liblig_oracle.so as the checker.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../../include/lig_hip_row_batcher.hpp"
#include "../../oracle/lig_oracle.h"

int main() {
    const uint32_t l = 320, k = 512, n = 2048, COLS = 40;
    lo_job j;
    std::memset(&j, 0, sizeof j);
    j.l = l; j.k = k; j.n = n; j.t = 192;
    j.n_linear = 320 * 6;                             // full rows only; linear rows come first
    j.n_quad = 320 * 2;
    for (int i = 0; i < 32; i++) j.encoding_seed[i] = (uint8_t)(5 * i + 3);
    lo_synth_key(23, j.witness_key);
    j.generated_at = 3333;
    j.threads = 4;
    const size_t R = lo_job_rows(&j) - 3;
    std::vector<lo_fr> rows(R * (size_t)k), mc(k), ml(2 * (size_t)k), mq(2 * (size_t)k);
    std::vector<uint8_t> kinds(R);
    lo_form_rows(&j, rows.data(), mc.data(), ml.data(), mq.data());
    lo_row_kinds(&j, kinds.data());
    const size_t X = 6, Y = 7, Z = 8, V = 3;
    if (R < 12 || kinds[0] != 0 || kinds[5] != 0 || kinds[X] != 1 || kinds[Y] != 2 || kinds[Z] != 3) { std::fprintf(stderr, "unexpected row order\n"); return 1; }
    // the guest's witness in the 40 columns: a, b, c, d below 2^20, so t < 2^21, u < 2^41, v < 2^42
    uint64_t st = 0x9E3779B97F4A7C15ull;
    auto next = [&] { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    auto set = [&](size_t r, uint32_t c, uint64_t v) { std::memset(&rows[r * k + c], 0, sizeof(lo_fr)); std::memcpy(&rows[r * k + c], &v, 8); };
    std::vector<uint64_t> want;                       // t, u, v per column
    for (uint32_t c = 0; c < COLS; c++) {
        const uint64_t a = next() & 0xFFFFF, b = next() & 0xFFFFF, y = c == 7 ? 0 : next() & 0xFFFFF, d = next() & 0xFFFFF;
        set(0, c, a); set(1, c, b); set(Y, c, y); set(2, c, d);
        set(X, c, a + b); set(Z, c, (a + b) * y); set(V, c, (a + b) * y + d);
        want.push_back(a + b); want.push_back((a + b) * y); want.push_back((a + b) * y + d);
    }
    // the defining constraints: 2c: a + b - t = 0;  2c + 1: u + d - v = 0
    std::vector<uint32_t> d_begin;
    std::vector<lig_lin_term> d_terms;
    std::vector<lig_derived_slot> list;
    std::vector<uint32_t> slots;                      // t, u, v per column, as `want`
    for (uint32_t c = 0; c < COLS; c++) {
        const uint32_t t = (uint32_t)X * l + c, u = (uint32_t)Z * l + c, v = (uint32_t)V * l + c;
        d_begin.push_back((uint32_t)d_terms.size());
        d_terms.push_back(lig_lin_term{c, LIG_COEF_ONE}); d_terms.push_back(lig_lin_term{l + c, LIG_COEF_ONE}); d_terms.push_back(lig_lin_term{t, LIG_COEF_NEG_ONE});
        d_begin.push_back((uint32_t)d_terms.size());
        d_terms.push_back(lig_lin_term{v, LIG_COEF_NEG_ONE}); d_terms.push_back(lig_lin_term{u, LIG_COEF_ONE}); d_terms.push_back(lig_lin_term{2 * l + c, LIG_COEF_ONE});
        list.push_back(lig_derived_slot{v, 2 * c + 1});                            // any order: the last wave first
        list.push_back(ligero::hip_row_batcher::product_entry(u));
        list.push_back(lig_derived_slot{t, 2 * c});
        slots.push_back(t); slots.push_back(u); slots.push_back(v);
    }
    d_begin.push_back((uint32_t)d_terms.size());
    lig_linear_system dsys;
    std::memset(&dsys, 0, sizeof dsys);
    dsys.struct_bytes = sizeof dsys;
    dsys.n_constraints = 2 * COLS; dsys.n_terms = d_terms.size();
    dsys.term_begin = d_begin.data(); dsys.terms = d_terms.data();

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

    // what the guest hands over: the true rows with 0 at t and v and GARBAGE at u (a derive_products z row is not shipped)
    std::vector<lo_fr> guest = rows;
    for (uint32_t c = 0; c < COLS; c++) {
        std::memset(&guest[X * k + c], 0, sizeof(lo_fr));
        std::memset(&guest[V * k + c], 0, sizeof(lo_fr));
        std::memset(&guest[Z * k + c], 0xAB, 8);
    }

    lig_ctx* ctx = nullptr;
    if (lig_ctx_create(&ctx, 0, l, k, n) != LIG_OK) { std::fprintf(stderr, "ctx: %s\n", ctx ? lig_last_error(ctx) : "?"); return 1; }
    int ok = 0;
    try {
        ligero::hip_proof_meta meta;
        std::memcpy(meta.encoding_seed, j.encoding_seed, 32);
        meta.generated_at = j.generated_at;
        meta.narrow_rows = true;
        meta.narrowest = true;
        meta.derive_products = true;
        auto at = [&](const std::vector<lo_fr>& v, size_t r) { return reinterpret_cast<const uint64_t*>(v.data() + r * (size_t)k); };
        ligero::hip_row_batcher b(ctx, meta);
        b.set_linear_system(sys);
        b.set_derived_slots(dsys, list.data(), list.size());
        for (size_t r = 0; r < R;) {
            if (kinds[r] == 0) { b.linear_callback(at(guest, r), nullptr); r += 1; }
            else { b.quadratic_callback(at(guest, r), at(guest, r + 1), at(guest, r + 2), nullptr, nullptr, nullptr); r += 3; }
        }
        b.mask_callback(k, 2 * (size_t)k, 2 * (size_t)k);
        uint8_t root[32], seed1[32];
        b.commit(root, seed1);
        std::vector<uint8_t> got(slots.size() * 32);
        b.read_slots(slots.data(), slots.size(), got.data());
        int values_equal = 1;
        for (size_t i = 0; i < slots.size(); i++) {
            uint8_t w[32] = {0};
            std::memcpy(w, &want[i], 8);
            if (std::memcmp(w, &got[32 * i], 32)) values_equal = 0;
        }
        size_t len = 0;
        lig_proof_info info;
        const uint8_t* proof = b.prove(nullptr, &len, &info);
        const int valid = info.valid_code && info.valid_linear && info.valid_quad;
        std::vector<lo_fr> rands(R * (size_t)k);
        lo_fr cs;
        lo_rand_rows(&j, seed1, rands.data(), &cs);
        lo_proof P;
        if (lo_prove_rows(&j, kinds.data(), R, rows.data(), mc.data(), ml.data(), mq.data(), rands.data(), nullptr, &P) != 0) throw std::runtime_error("oracle prover failed");
        const int equals_oracle = len == P.proof_len && !std::memcmp(proof, P.proof, len) && !std::memcmp(root, P.root, 32);
        lo_proof_free(&P);
        ok = values_equal && valid && equals_oracle;
        std::printf("{\"values_equal\": %s, \"valid\": %s, \"equals_oracle\": %s, \"entries\": %zu}\n", values_equal ? "true" : "false", valid ? "true" : "false",
                    equals_oracle ? "true" : "false", list.size());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
    }
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
