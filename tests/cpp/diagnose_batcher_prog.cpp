// diagnose_batcher_prog.cpp -- hip_row_batcher::diagnose: the row-batching shim names the violated constraints of a corrupted stream.
// The rows are the oracle's synthetic stream; the system is its statement, one constraint w[s] = b_s per witness slot in commit order
// (tests/cpp/linear_batcher_prog.cpp).  After the right-hand sides are fixed a few slots are changed (limb 0 ^ 1): a linear-row slot
// breaks one linear constraint, an x or z slot of a triple a linear constraint and a quadratic term.
// Prints one JSON line: the changed slots, what diagnose() reported after commit() and again after prove(), and valid_linear of the proof;
// tests/test_gpu_diagnose_batcher.py changes the same slots in its own copy of the rows and compares with tests/diagnose_ref.py.
// TEST CODE: links oracle/liblig_oracle.so as the guest (rows with their pads).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lig_hip_row_batcher.hpp"
#include "../../oracle/lig_oracle.h"

static std::string hex32(const uint8_t* b) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (int i = 0; i < 32; i++) { s += d[b[i] >> 4]; s += d[b[i] & 15]; }
    return s;
}

int main() {
    const uint32_t l = 320, k = 512, n = 2048;
    lo_job j;
    std::memset(&j, 0, sizeof j);
    j.l = l; j.k = k; j.n = n; j.t = 192;
    j.n_linear = 320 * 5;
    j.n_quad = 320 * 2;
    for (int i = 0; i < 32; i++) j.encoding_seed[i] = (uint8_t)i;
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
    // the corrupted stream: a slot of the first linear row, of the last one, the x and the z of the first triple, the z of the second
    size_t first_lin = R, last_lin = 0, first_x = R;
    for (size_t r = 0; r < R; r++) {
        if (kinds[r] == 0) { if (first_lin == R) first_lin = r; last_lin = r; }
        if (kinds[r] == 1 && first_x == R) first_x = r;
    }
    if (first_lin == R || first_x == R || first_x + 5 >= R) { std::fprintf(stderr, "unexpected row kinds\n"); return 1; }
    const std::vector<uint32_t> changed = {(uint32_t)(first_lin * l + 3), (uint32_t)(last_lin * l + l - 1), (uint32_t)(first_x * l + 200),
                                           (uint32_t)((first_x + 2) * l + 11), (uint32_t)((first_x + 5) * l + 257)};
    for (uint32_t s : changed) reinterpret_cast<uint32_t*>(&rows[(s / l) * (size_t)k + s % l])[0] ^= 1u;

    lig_ctx* ctx = nullptr;
    if (lig_ctx_create(&ctx, 0, l, k, n) != LIG_OK) { std::fprintf(stderr, "ctx: %s\n", ctx ? lig_last_error(ctx) : "?"); return 1; }
    int ok = 0;
    try {
        ligero::hip_proof_meta meta;
        std::memcpy(meta.encoding_seed, j.encoding_seed, 32);
        meta.generated_at = j.generated_at;
        auto at = [&](size_t r) { return reinterpret_cast<const uint64_t*>(rows.data() + r * (size_t)k); };
        ligero::hip_row_batcher b(ctx, meta);
        b.set_linear_system(sys);
        for (size_t r = 0; r < R;) {
            if (kinds[r] == 0) { b.linear_callback(at(r), nullptr); r += 1; }
            else { b.quadratic_callback(at(r), at(r + 1), at(r + 2), nullptr, nullptr, nullptr); r += 3; }
        }
        b.mask_callback(k, 2 * (size_t)k, 2 * (size_t)k);
        uint8_t root[32], seed1[32];
        b.commit(root, seed1);
        std::vector<lig_diag_linear> lin(16), lin2(16);
        std::vector<lig_diag_quad> quad(16), quad2(16);
        lig_diag_info di, di2;
        b.diagnose(lin.data(), lin.size(), quad.data(), quad.size(), &di);
        size_t len = 0;
        lig_proof_info info;
        b.prove(nullptr, &len, &info);
        b.diagnose(lin2.data(), lin2.size(), quad2.data(), quad2.size(), &di2);
        const bool same_after = di2.n_linear_bad == di.n_linear_bad && di2.n_quad_bad == di.n_quad_bad && di2.n_linear_reported == di.n_linear_reported &&
                                di2.n_quad_reported == di.n_quad_reported && !std::memcmp(lin.data(), lin2.data(), di.n_linear_reported * sizeof(lig_diag_linear)) &&
                                !std::memcmp(quad.data(), quad2.data(), di.n_quad_reported * sizeof(lig_diag_quad));
        std::printf("{\"rows\": %zu, \"changed\": [", R);
        for (size_t i = 0; i < changed.size(); i++) std::printf("%s%u", i ? ", " : "", changed[i]);
        std::printf("], \"n_linear_bad\": %llu, \"n_quad_bad\": %llu, \"linear\": [", (unsigned long long)di.n_linear_bad, (unsigned long long)di.n_quad_bad);
        for (uint64_t i = 0; i < di.n_linear_reported; i++) std::printf("%s[%u, \"%s\"]", i ? ", " : "", lin[i].constraint, hex32(lin[i].residual).c_str());
        std::printf("], \"quad\": [");
        for (uint64_t i = 0; i < di.n_quad_reported; i++)
            std::printf("%s[%u, %u, %u, %u, \"%s\"]", i ? ", " : "", quad[i].row_x, quad[i].row_y, quad[i].row_z, quad[i].column, hex32(quad[i].residual).c_str());
        std::printf("], \"same_after_prove\": %s, \"valid_linear\": %d, \"valid_quad\": %d}\n", same_after ? "true" : "false", info.valid_linear, info.valid_quad);
        ok = 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
    }
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
