// diagnose_attached_batcher_prog.cpp -- hip_row_batcher::diagnose_attached: a batcher that was given a PREPARED program (set_linear_program)
// and this statement's values (set_linear_values) has no term list, and still names the violated linear constraint.
// The rows are the oracle's synthetic stream; the statement is one constraint w[s] = b_s per witness slot in commit order
// (tests/cpp/diagnose_batcher_prog.cpp).  The program is prepared with a table that is wrong in a few entries; the values set on the batcher
// are the true ones, so an evaluation against the program's own table would name other constraints.  After the right-hand sides are fixed
// one slot of a linear row and one z slot of a triple are changed (limb 0 ^ 1).
// Prints one JSON line: the changed slots, what diagnose_attached() reported after commit() and again after prove(), what the present
// diagnose() reported on the same batcher (the quadratic part only), and which misuse raised std::logic_error;
// tests/test_gpu_diagnose_attached_batcher.py changes the same slots in its own copy of the rows and compares with tests/diagnose_ref.py.
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
    // the corrupted stream: a slot of the last linear row, the z of the first triple
    size_t first_lin = R, last_lin = 0, first_x = R;
    for (size_t r = 0; r < R; r++) {
        if (kinds[r] == 0) { if (first_lin == R) first_lin = r; last_lin = r; }
        if (kinds[r] == 1 && first_x == R) first_x = r;
    }
    if (first_lin == R || first_x == R || first_x + 5 >= R) { std::fprintf(stderr, "unexpected row kinds\n"); return 1; }
    const std::vector<uint32_t> changed = {(uint32_t)(last_lin * l + l - 1), (uint32_t)((first_x + 2) * l + 11)};
    for (uint32_t s : changed) reinterpret_cast<uint32_t*>(&rows[(s / l) * (size_t)k + s % l])[0] ^= 1u;

    // the table the program is prepared with: wrong in three entries the witness does NOT violate under the true values
    std::vector<uint8_t> stale = coefs;
    const std::vector<uint32_t> stale_at = {(uint32_t)(first_lin * l + 3), (uint32_t)(first_x * l + 200), (uint32_t)(S - 1)};
    for (uint32_t s : stale_at) stale[32 * (size_t)s] ^= 1u;
    lig_linear_system stale_sys = sys;
    stale_sys.coefs = stale.data();

    lig_ctx* ctx = nullptr;
    if (lig_ctx_create(&ctx, 0, l, k, n) != LIG_OK) { std::fprintf(stderr, "ctx: %s\n", ctx ? lig_last_error(ctx) : "?"); return 1; }
    lig_linear_program* prog = nullptr;
    int ok = 0;
    try {
        if (lig_linear_prepare(ctx, &stale_sys, kinds.data(), R, &prog) != LIG_OK) throw std::runtime_error(std::string("lig_linear_prepare: ") + lig_last_error(ctx));
        // every pointer of the system may be released now: the term list is gone before the batcher exists
        std::vector<lig_lin_term>().swap(terms);
        std::vector<uint32_t>().swap(term_begin);
        ligero::hip_proof_meta meta;
        std::memcpy(meta.encoding_seed, j.encoding_seed, 32);
        meta.generated_at = j.generated_at;
        auto at = [&](size_t r) { return reinterpret_cast<const uint64_t*>(rows.data() + r * (size_t)k); };
        auto feed = [&](ligero::hip_row_batcher& b) {
            for (size_t r = 0; r < R;) {
                if (kinds[r] == 0) { b.linear_callback(at(r), nullptr); r += 1; }
                else { b.quadratic_callback(at(r), at(r + 1), at(r + 2), nullptr, nullptr, nullptr); r += 3; }
            }
            b.mask_callback(k, 2 * (size_t)k, 2 * (size_t)k);
        };
        std::vector<lig_diag_linear> lin(16), lin2(16), lin3(16);
        std::vector<lig_diag_quad> quad(16), quad2(16), quad3(16);
        lig_diag_info di, di2, di3;
        auto raises = [&](ligero::hip_row_batcher& b) {
            try { b.diagnose_attached(lin3.data(), lin3.size(), quad3.data(), quad3.size(), &di3); } catch (const std::logic_error&) { return true; }
            return false;
        };
        uint8_t root[32], seed1[32];
        ligero::hip_row_batcher b(ctx, meta);
        b.set_linear_program(prog);
        b.set_linear_values(coefs.data(), S);
        feed(b);
        const bool raised_before_commit = raises(b);
        b.commit(root, seed1);
        b.diagnose_attached(lin.data(), lin.size(), quad.data(), quad.size(), &di);
        b.diagnose(lin3.data(), lin3.size(), quad3.data(), quad3.size(), &di3);      // no term list: the quadratic part only
        const bool plain_quad_only = di3.n_linear_bad == 0 && di3.n_linear_reported == 0 && di3.n_quad_bad == di.n_quad_bad && di3.n_quad_reported == di.n_quad_reported &&
                                     !std::memcmp(quad.data(), quad3.data(), di.n_quad_reported * sizeof(lig_diag_quad));
        size_t len = 0;
        lig_proof_info info;
        b.prove(nullptr, &len, &info);
        b.diagnose_attached(lin2.data(), lin2.size(), quad2.data(), quad2.size(), &di2);
        const bool same_after = di2.n_linear_bad == di.n_linear_bad && di2.n_quad_bad == di.n_quad_bad && di2.n_linear_reported == di.n_linear_reported &&
                                di2.n_quad_reported == di.n_quad_reported && !std::memcmp(lin.data(), lin2.data(), di.n_linear_reported * sizeof(lig_diag_linear)) &&
                                !std::memcmp(quad.data(), quad2.data(), di.n_quad_reported * sizeof(lig_diag_quad));
        // misuse: no linear structure at all (after its commit); a sharded batcher (never committed: its comm is not used)
        ligero::hip_row_batcher none(ctx, meta);
        feed(none);
        none.commit(root, seed1);
        const bool raised_without_linear = raises(none);
        lig_comm comm;
        std::memset(&comm, 0, sizeof comm);
        ligero::hip_row_batcher sharded(ctx, meta);
        sharded.shard_over(0, 1, &comm);
        const uint32_t tiny_begin[2] = {0, 1};
        const lig_lin_term tiny_term = {0, LIG_COEF_ONE};
        lig_linear_system tiny;
        std::memset(&tiny, 0, sizeof tiny);
        tiny.struct_bytes = sizeof tiny;
        tiny.n_constraints = 1; tiny.n_terms = 1;
        tiny.term_begin = tiny_begin; tiny.terms = &tiny_term;
        sharded.set_linear_system(tiny);
        const bool raised_sharded = raises(sharded);
        std::printf("{\"rows\": %zu, \"changed\": [", R);
        for (size_t i = 0; i < changed.size(); i++) std::printf("%s%u", i ? ", " : "", changed[i]);
        std::printf("], \"stale\": [");
        for (size_t i = 0; i < stale_at.size(); i++) std::printf("%s%u", i ? ", " : "", stale_at[i]);
        std::printf("], \"n_linear_bad\": %llu, \"n_quad_bad\": %llu, \"linear\": [", (unsigned long long)di.n_linear_bad, (unsigned long long)di.n_quad_bad);
        for (uint64_t i = 0; i < di.n_linear_reported; i++) std::printf("%s[%u, \"%s\"]", i ? ", " : "", lin[i].constraint, hex32(lin[i].residual).c_str());
        std::printf("], \"quad\": [");
        for (uint64_t i = 0; i < di.n_quad_reported; i++)
            std::printf("%s[%u, %u, %u, %u, \"%s\"]", i ? ", " : "", quad[i].row_x, quad[i].row_y, quad[i].row_z, quad[i].column, hex32(quad[i].residual).c_str());
        std::printf("], \"same_after_prove\": %s, \"plain_diagnose_quadratic_only\": %s, \"valid_linear\": %d, \"valid_quad\": %d, ", same_after ? "true" : "false",
                    plain_quad_only ? "true" : "false", info.valid_linear, info.valid_quad);
        std::printf("\"raised_before_commit\": %s, \"raised_without_linear\": %s, \"raised_sharded\": %s}\n", raised_before_commit ? "true" : "false",
                    raised_without_linear ? "true" : "false", raised_sharded ? "true" : "false");
        ok = 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
    }
    lig_linear_program_release(prog);
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
