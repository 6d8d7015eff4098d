// explain_slots_batcher_prog.cpp -- hip_row_batcher::explain_slots / explain_slots_attached / untouched_slots / untouched_slots_attached: the
// constraints through asked slots with their sizes, coefficient values and residuals, and the witness slots no constraint touches.
// The rows are the oracle's synthetic stream.  The statement (no right-hand sides, so most constraints are violated and carry a residual):
//   constraint c < 3000:  w[37 c mod S] + T[c mod 3] * w[(101 c + 5) mod S]  (- w[123] when c is even)
// with the table T = (5, 7, 11).  The system is given with a table that is wrong in entry 0; the values set on the batcher are the true ones.
// A first batcher holds the system (set_linear_system): the term-list forms and the attached forms must agree byte for byte, after
// commit() and again after prove().  A second batcher holds a prepared program only: the term-list forms have no term list
// (std::logic_error), the attached forms return the bytes of the first.
// Prints one JSON line; tests/test_gpu_explain_slots_batcher.py asks the Python binding the same questions on the same trace.
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
    const uint32_t S = (uint32_t)(R * (size_t)l), NC = 3000, hot = 123;
    std::vector<uint32_t> term_begin(1, 0u);
    std::vector<lig_lin_term> terms;
    for (uint32_t c = 0; c < NC; c++) {
        terms.push_back(lig_lin_term{(uint32_t)((37ull * c) % S), LIG_COEF_ONE});
        terms.push_back(lig_lin_term{(uint32_t)((101ull * c + 5) % S), c % 3});
        if (c % 2 == 0) terms.push_back(lig_lin_term{hot, LIG_COEF_NEG_ONE});
        term_begin.push_back((uint32_t)terms.size());
    }
    std::vector<uint8_t> coefs(3 * 32, 0), stale;
    coefs[0] = 5; coefs[32] = 7; coefs[64] = 11;
    stale = coefs;
    stale[0] = 6;
    lig_linear_system sys;
    std::memset(&sys, 0, sizeof sys);
    sys.struct_bytes = sizeof sys;
    sys.n_constraints = NC; sys.n_terms = terms.size(); sys.n_coefs = 3;
    sys.term_begin = term_begin.data(); sys.terms = terms.data(); sys.coefs = stale.data();

    lig_ctx* ctx = nullptr;
    if (lig_ctx_create(&ctx, 0, l, k, n) != LIG_OK) { std::fprintf(stderr, "ctx: %s\n", ctx ? lig_last_error(ctx) : "?"); return 1; }
    lig_linear_program* prog = nullptr;
    int ok = 0;
    try {
        if (lig_linear_prepare(ctx, &sys, kinds.data(), R, &prog) != LIG_OK) throw std::runtime_error(std::string("lig_linear_prepare: ") + lig_last_error(ctx));
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
        const uint64_t cap = 48, ucap = 24;
        const std::vector<uint32_t> asked = {0u, 5u, 37u, hot, 3000u, S - 1};
        struct Answer {
            std::vector<lig_slot_record> rec;
            std::vector<lig_slot_term> terms;
            lig_slot_info info;
            std::vector<lig_slot_value> un;
            lig_untouched_info uinfo;
            bool same(const Answer& o) const {
                return info.n_terms_total == o.info.n_terms_total && info.n_terms_reported == o.info.n_terms_reported &&
                       info.n_constraints_distinct == o.info.n_constraints_distinct && uinfo.n_untouched == o.uinfo.n_untouched &&
                       uinfo.n_untouched_nonzero == o.uinfo.n_untouched_nonzero && uinfo.n_reported == o.uinfo.n_reported &&
                       !std::memcmp(rec.data(), o.rec.data(), rec.size() * sizeof(lig_slot_record)) &&
                       !std::memcmp(terms.data(), o.terms.data(), info.n_terms_reported * sizeof(lig_slot_term)) &&
                       !std::memcmp(un.data(), o.un.data(), uinfo.n_reported * sizeof(lig_slot_value));
            }
        };
        auto blank = [&]() {
            Answer a;
            a.rec.resize(asked.size()); a.terms.resize(cap); a.un.resize(ucap);
            std::memset(a.rec.data(), 0, a.rec.size() * sizeof(lig_slot_record));
            std::memset(&a.info, 0, sizeof a.info); std::memset(&a.uinfo, 0, sizeof a.uinfo);
            return a;
        };
        auto ask = [&](ligero::hip_row_batcher& b, bool attached) {
            Answer a = blank();
            if (attached) {
                b.explain_slots_attached(asked.data(), asked.size(), a.rec.data(), a.terms.data(), cap, &a.info);
                b.untouched_slots_attached(true, a.un.data(), ucap, &a.uinfo);
            } else {
                b.explain_slots(asked.data(), asked.size(), a.rec.data(), a.terms.data(), cap, &a.info);
                b.untouched_slots(true, a.un.data(), ucap, &a.uinfo);
            }
            return a;
        };
        auto raises = [&](ligero::hip_row_batcher& b, bool attached) {      // how many of the two forms throw std::logic_error
            int raised = 0;
            Answer a = blank();
            try {
                if (attached) b.explain_slots_attached(asked.data(), asked.size(), a.rec.data(), a.terms.data(), cap, &a.info);
                else b.explain_slots(asked.data(), asked.size(), a.rec.data(), a.terms.data(), cap, &a.info);
            } catch (const std::logic_error&) { raised++; }
            try {
                if (attached) b.untouched_slots_attached(false, a.un.data(), ucap, &a.uinfo);
                else b.untouched_slots(false, a.un.data(), ucap, &a.uinfo);
            } catch (const std::logic_error&) { raised++; }
            return raised;
        };
        uint8_t root[32], seed1[32];
        ligero::hip_row_batcher b(ctx, meta);
        b.set_linear_system(sys);
        b.set_linear_values(coefs.data(), 3);
        feed(b);
        const int raised_before_commit = raises(b, true) + raises(b, false);
        b.commit(root, seed1);
        const Answer att = ask(b, true), lst = ask(b, false);
        size_t len = 0;
        lig_proof_info info;
        b.prove(nullptr, &len, &info);
        const Answer att2 = ask(b, true);

        // a batcher with a prepared program: no term list
        ligero::hip_row_batcher pb(ctx, meta);
        pb.set_linear_program(prog);
        pb.set_linear_values(coefs.data(), 3);
        feed(pb);
        pb.commit(root, seed1);
        const int raised_without_terms = raises(pb, false);
        const Answer from_prog = ask(pb, true);
        // misuse: no linear structure at all (after its commit); a sharded batcher (never committed: its comm is not used)
        ligero::hip_row_batcher none(ctx, meta);
        feed(none);
        none.commit(root, seed1);
        const int raised_without_linear = raises(none, true) + raises(none, false);
        lig_comm comm;
        std::memset(&comm, 0, sizeof comm);
        ligero::hip_row_batcher sharded(ctx, meta);
        sharded.shard_over(0, 1, &comm);
        const int raised_sharded = raises(sharded, true) + raises(sharded, false);

        std::printf("{\"rows\": %zu, \"asked\": [", R);
        for (size_t i = 0; i < asked.size(); i++) std::printf("%s%u", i ? ", " : "", asked[i]);
        std::printf("], \"n_terms_total\": %llu, \"n_terms_reported\": %llu, \"n_constraints_distinct\": %llu, \"slots\": [", (unsigned long long)att.info.n_terms_total,
                    (unsigned long long)att.info.n_terms_reported, (unsigned long long)att.info.n_constraints_distinct);
        for (size_t i = 0; i < att.rec.size(); i++)
            std::printf("%s[%u, %u, %llu, %llu, \"%s\"]", i ? ", " : "", att.rec[i].slot, att.rec[i].row_kind, (unsigned long long)att.rec[i].n_terms,
                        (unsigned long long)att.rec[i].first_term, hex32(att.rec[i].value).c_str());
        std::printf("], \"terms\": [");
        for (uint64_t i = 0; i < att.info.n_terms_reported; i++)
            std::printf("%s[%u, %u, %u, %u, \"%s\", \"%s\"]", i ? ", " : "", att.terms[i].slot, att.terms[i].constraint, att.terms[i].coef_index, att.terms[i].constraint_terms,
                        hex32(att.terms[i].coef).c_str(), hex32(att.terms[i].residual).c_str());
        std::printf("], \"n_untouched\": %llu, \"n_untouched_nonzero\": %llu, \"n_reported\": %llu, \"untouched\": [", (unsigned long long)att.uinfo.n_untouched,
                    (unsigned long long)att.uinfo.n_untouched_nonzero, (unsigned long long)att.uinfo.n_reported);
        for (uint64_t i = 0; i < att.uinfo.n_reported; i++)
            std::printf("%s[%u, %u, \"%s\"]", i ? ", " : "", att.un[i].slot, att.un[i].row_kind, hex32(att.un[i].value).c_str());
        std::printf("], \"list_equals_attached\": %s, \"same_after_prove\": %s, \"program_equals_system\": %s, ", lst.same(att) ? "true" : "false",
                    att2.same(att) ? "true" : "false", from_prog.same(att) ? "true" : "false");
        std::printf("\"raised_before_commit\": %d, \"raised_without_terms\": %d, \"raised_without_linear\": %d, \"raised_sharded\": %d}\n", raised_before_commit,
                    raised_without_terms, raised_without_linear, raised_sharded);
        ok = 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
    }
    lig_linear_program_release(prog);
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
