// explain_batcher_prog.cpp -- hip_row_batcher::explain / explain_attached / read_slots: the constraints diagnose_attached() named, shown
// with their terms, coefficient values, committed witness values, right-hand sides and residuals.
// The rows are the oracle's synthetic stream; the statement is one constraint w[s] = b_s per witness slot in commit order
// (tests/cpp/diagnose_attached_batcher_prog.cpp).  The system is given with a table that is wrong in one entry; the values set on the
// batcher are the true ones.  After the right-hand sides are fixed one slot of a linear row and one z slot of a triple are changed
// (limb 0 ^ 1).  A first batcher holds the system (set_linear_system): explain() and explain_attached() must agree byte for byte, after
// commit() and again after prove().  A second batcher holds a prepared program only: explain() has no term list (std::logic_error),
// explain_attached() returns the bytes of the first.
// Prints one JSON line; tests/test_gpu_explain_batcher.py changes the same slots in its own copy of the rows and compares with
// tests/explain_ref.py.
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
    size_t last_lin = 0, first_x = R;
    for (size_t r = 0; r < R; r++) {
        if (kinds[r] == 0) last_lin = r;
        if (kinds[r] == 1 && first_x == R) first_x = r;
    }
    if (first_x == R || first_x + 5 >= R) { std::fprintf(stderr, "unexpected row kinds\n"); return 1; }
    const std::vector<uint32_t> changed = {(uint32_t)(last_lin * l + l - 1), (uint32_t)((first_x + 2) * l + 11)};
    for (uint32_t s : changed) reinterpret_cast<uint32_t*>(&rows[(s / l) * (size_t)k + s % l])[0] ^= 1u;
    // the table the system is given with: wrong in one entry, which the values set on the batcher put right
    std::vector<uint8_t> stale = coefs;
    const uint32_t stale_at = 3;
    stale[32 * (size_t)stale_at] ^= 1u;
    lig_linear_system stale_sys = sys;
    stale_sys.coefs = stale.data();

    lig_ctx* ctx = nullptr;
    if (lig_ctx_create(&ctx, 0, l, k, n) != LIG_OK) { std::fprintf(stderr, "ctx: %s\n", ctx ? lig_last_error(ctx) : "?"); return 1; }
    lig_linear_program* prog = nullptr;
    int ok = 0;
    try {
        if (lig_linear_prepare(ctx, &stale_sys, kinds.data(), R, &prog) != LIG_OK) throw std::runtime_error(std::string("lig_linear_prepare: ") + lig_last_error(ctx));
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
        struct Answer {
            std::vector<lig_explain_constraint> con;
            std::vector<lig_explain_term> terms;
            lig_explain_info info;
            bool same(const Answer& o) const {
                return info.n_terms_total == o.info.n_terms_total && info.n_terms_reported == o.info.n_terms_reported && con.size() == o.con.size() &&
                       !std::memcmp(con.data(), o.con.data(), con.size() * sizeof(lig_explain_constraint)) &&
                       !std::memcmp(terms.data(), o.terms.data(), info.n_terms_reported * sizeof(lig_explain_term));
            }
        };
        const uint64_t cap = 8;
        auto blank = [&](size_t n_asked) { Answer a; a.con.resize(n_asked); a.terms.resize(cap); std::memset(&a.info, 0, sizeof a.info); return a; };
        uint8_t root[32], seed1[32];
        ligero::hip_row_batcher b(ctx, meta);
        b.set_linear_system(stale_sys);
        b.set_linear_values(coefs.data(), S);
        feed(b);
        bool raised_before_commit = false;
        {
            Answer a = blank(1);
            const uint32_t one = 0;
            try { b.explain_attached(&one, 1, a.con.data(), a.terms.data(), cap, &a.info); } catch (const std::logic_error&) { raised_before_commit = true; }
            try { b.explain(&one, 1, a.con.data(), a.terms.data(), cap, &a.info); raised_before_commit = false; } catch (const std::logic_error&) {}
            uint8_t v[32];
            try { b.read_slots(&one, 1, v); raised_before_commit = false; } catch (const std::logic_error&) {}
        }
        b.commit(root, seed1);
        // which constraints: what diagnose_attached() names, and the (satisfied) constraint whose program entry is stale
        std::vector<lig_diag_linear> lin(16);
        std::vector<lig_diag_quad> quad(16);
        lig_diag_info di;
        b.diagnose_attached(lin.data(), lin.size(), quad.data(), quad.size(), &di);
        std::vector<uint32_t> asked = {stale_at};
        for (uint64_t i = 0; i < di.n_linear_reported; i++) asked.push_back(lin[i].constraint);
        Answer att = blank(asked.size()), lst = blank(asked.size()), att2 = blank(asked.size()), from_prog = blank(asked.size());
        b.explain_attached(asked.data(), asked.size(), att.con.data(), att.terms.data(), cap, &att.info);
        b.explain(asked.data(), asked.size(), lst.con.data(), lst.terms.data(), cap, &lst.info);
        // the committed elements: the two changed slots, one of them twice, and slot 0, in no order
        const std::vector<uint32_t> slots = {changed[1], 0u, changed[0], changed[1]};
        std::vector<uint8_t> values(slots.size() * 32);
        b.read_slots(slots.data(), slots.size(), values.data());
        size_t len = 0;
        lig_proof_info info;
        b.prove(nullptr, &len, &info);
        b.explain_attached(asked.data(), asked.size(), att2.con.data(), att2.terms.data(), cap, &att2.info);

        // a batcher with a prepared program: no term list
        ligero::hip_row_batcher pb(ctx, meta);
        pb.set_linear_program(prog);
        pb.set_linear_values(coefs.data(), S);
        feed(pb);
        pb.commit(root, seed1);
        bool raised_without_terms = false;
        try { pb.explain(asked.data(), asked.size(), from_prog.con.data(), from_prog.terms.data(), cap, &from_prog.info); } catch (const std::logic_error&) { raised_without_terms = true; }
        pb.explain_attached(asked.data(), asked.size(), from_prog.con.data(), from_prog.terms.data(), cap, &from_prog.info);
        // misuse: no linear structure at all (after its commit); a sharded batcher (never committed: its comm is not used)
        ligero::hip_row_batcher none(ctx, meta);
        feed(none);
        none.commit(root, seed1);
        bool raised_without_linear = false;
        {
            Answer a = blank(asked.size());
            try { none.explain_attached(asked.data(), asked.size(), a.con.data(), a.terms.data(), cap, &a.info); } catch (const std::logic_error&) { raised_without_linear = true; }
        }
        std::vector<uint8_t> none_values(slots.size() * 32);
        none.read_slots(slots.data(), slots.size(), none_values.data());      // reading needs no statement
        lig_comm comm;
        std::memset(&comm, 0, sizeof comm);
        ligero::hip_row_batcher sharded(ctx, meta);
        sharded.shard_over(0, 1, &comm);
        int raised_sharded = 0;
        {
            Answer a = blank(1);
            const uint32_t one = 0;
            uint8_t v[32];
            try { sharded.explain(&one, 1, a.con.data(), a.terms.data(), cap, &a.info); } catch (const std::logic_error&) { raised_sharded++; }
            try { sharded.explain_attached(&one, 1, a.con.data(), a.terms.data(), cap, &a.info); } catch (const std::logic_error&) { raised_sharded++; }
            try { sharded.read_slots(&one, 1, v); } catch (const std::logic_error&) { raised_sharded++; }
        }
        std::printf("{\"rows\": %zu, \"changed\": [%u, %u], \"stale\": %u, \"asked\": [", R, changed[0], changed[1], stale_at);
        for (size_t i = 0; i < asked.size(); i++) std::printf("%s%u", i ? ", " : "", asked[i]);
        std::printf("], \"n_terms_total\": %llu, \"n_terms_reported\": %llu, \"constraints\": [", (unsigned long long)att.info.n_terms_total,
                    (unsigned long long)att.info.n_terms_reported);
        for (size_t i = 0; i < att.con.size(); i++)
            std::printf("%s[%u, %llu, %llu, \"%s\", \"%s\"]", i ? ", " : "", att.con[i].constraint, (unsigned long long)att.con[i].n_terms,
                        (unsigned long long)att.con[i].first_term, hex32(att.con[i].rhs).c_str(), hex32(att.con[i].residual).c_str());
        std::printf("], \"terms\": [");
        for (uint64_t i = 0; i < att.info.n_terms_reported; i++)
            std::printf("%s[%u, %u, %u, \"%s\", \"%s\"]", i ? ", " : "", att.terms[i].constraint, att.terms[i].slot, att.terms[i].coef_index, hex32(att.terms[i].coef).c_str(),
                        hex32(att.terms[i].value).c_str());
        std::printf("], \"slots\": [");
        for (size_t i = 0; i < slots.size(); i++) std::printf("%s[%u, \"%s\"]", i ? ", " : "", slots[i], hex32(&values[32 * i]).c_str());
        std::printf("], \"list_equals_attached\": %s, \"same_after_prove\": %s, \"program_equals_system\": %s, \"read_without_statement\": %s, ",
                    lst.same(att) ? "true" : "false", att2.same(att) ? "true" : "false", from_prog.same(att) ? "true" : "false", none_values == values ? "true" : "false");
        std::printf("\"valid_linear\": %d, \"raised_before_commit\": %s, \"raised_without_terms\": %s, \"raised_without_linear\": %s, \"raised_sharded\": %d}\n",
                    info.valid_linear, raised_before_commit ? "true" : "false", raised_without_terms ? "true" : "false", raised_without_linear ? "true" : "false",
                    raised_sharded);
        ok = 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
    }
    lig_linear_program_release(prog);
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
