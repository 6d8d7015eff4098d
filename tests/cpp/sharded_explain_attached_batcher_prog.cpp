// sharded_explain_attached_batcher_prog.cpp -- hip_row_batcher::shard_explain_attached on a sharded batcher (shard_over +
// set_linear_system -> lig_shard_rows_explain_attached): ONE guest trace with ONE wrong witness slot, held by `world` processes (here all
// on GPU 0, communicator of csrc/comm_ipc.hip).  Every rank sets the system of the WHOLE trace (one constraint w[s] = b_s per witness
// slot), commits, calls diagnose_attached(), then shard_explain_attached() of the constraints it reported together with two satisfied
// ones on rows of the first and of the last rank's share: a collective call over the ranks' shares whose records must be the bytes of
// explain() -- the term list -- on the same batcher, on every rank; with set_linear_values() the records follow the values; the same
// bytes come back after prove().  std::logic_error: before commit(), on an unsharded batcher, and from explain_attached() on the sharded
// one.   usage: sharded_explain_attached_batcher_prog rank world /shm_name
// Prints one JSON line with every record; tests/test_gpu_shard_explain_attached_batcher.py changes the same slot in its own copy of the
// rows and compares with tests/explain_ref.py.
// TEST CODE: links oracle/liblig_oracle.so as the guest.
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

struct Answer {
    std::vector<lig_explain_constraint> con;
    std::vector<lig_explain_term> terms;
    lig_explain_info info;
    bool same(const Answer& o) const {
        return info.n_terms_total == o.info.n_terms_total && info.n_terms_reported == o.info.n_terms_reported && con.size() == o.con.size() &&
               !std::memcmp(con.data(), o.con.data(), con.size() * sizeof(lig_explain_constraint)) &&
               !std::memcmp(terms.data(), o.terms.data(), info.n_terms_reported * sizeof(lig_explain_term));
    }
    void print(const char* name) const {
        std::printf("\"%s\": {\"n_terms_total\": %llu, \"n_terms_reported\": %llu, \"constraints\": [", name, (unsigned long long)info.n_terms_total,
                    (unsigned long long)info.n_terms_reported);
        for (size_t i = 0; i < con.size(); i++)
            std::printf("%s[%u, %llu, %llu, \"%s\", \"%s\"]", i ? ", " : "", con[i].constraint, (unsigned long long)con[i].n_terms, (unsigned long long)con[i].first_term,
                        hex32(con[i].rhs).c_str(), hex32(con[i].residual).c_str());
        std::printf("], \"terms\": [");
        for (uint64_t i = 0; i < info.n_terms_reported; i++)
            std::printf("%s[%u, %u, %u, \"%s\", \"%s\"]", i ? ", " : "", terms[i].constraint, terms[i].slot, terms[i].coef_index, hex32(terms[i].coef).c_str(),
                        hex32(terms[i].value).c_str());
        std::printf("]}");
    }
};

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
    // the statement: one constraint w[s] = b_s per witness slot, b_s taken from the honest witness
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
    // another statement of the same structure: the right-hand side of constraint 3 (a row of the first rank's share) changes
    std::vector<uint8_t> other = coefs;
    other[32 * 3] ^= 2;
    // ... and then one witness slot changes: column 7 of the last QX row of the trace (a row of the last rank's share)
    size_t bad_row = R;
    for (size_t r = 0; r < R; r++) if (kinds[r] == 1) bad_row = r;
    if (bad_row == R) { std::fprintf(stderr, "no QX row\n"); return 1; }
    const uint32_t bad_col = 7, bad_slot = (uint32_t)(bad_row * l + bad_col);
    reinterpret_cast<uint8_t*>(&rows[bad_row * (size_t)k + bad_col])[0] ^= 1;

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
        const uint64_t cap = 8;
        auto blank = [&](size_t n_asked) { Answer a; a.con.resize(n_asked); a.terms.resize(cap); std::memset(&a.info, 0, sizeof a.info); return a; };
        uint8_t root[32], seed1[32];
        bool raised_before_commit = false, raised_attached = false, raised_unsharded = false;
        bool same_as_explain = false, values_same_as_explain = false, same_after_values_removed = false, same_after_prove = false;
        size_t local = 0;
        std::vector<uint32_t> asked;
        Answer first, with_values;
        lig_diag_info di;
        {
            ligero::hip_row_batcher u(ctx, meta);         // never sharded: nothing is launched
            Answer a = blank(1);
            const uint32_t one = 0;
            try { u.shard_explain_attached(&one, 1, a.con.data(), a.terms.data(), cap, &a.info); } catch (const std::logic_error&) { raised_unsharded = true; }
        }
        {
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_system(sys);
            b.shard_over(rank, world, &comm);
            for (size_t r = 0; r < R;) {
                if (kinds[r] == 0) { b.linear_callback(at(r)); r += 1; }
                else { b.quadratic_callback(at(r), at(r + 1), at(r + 2)); r += 3; }
            }
            b.mask_callback(k, 2 * (size_t)k, 2 * (size_t)k);
            {
                Answer a = blank(1);
                const uint32_t one = 0;
                try { b.shard_explain_attached(&one, 1, a.con.data(), a.terms.data(), cap, &a.info); } catch (const std::logic_error&) { raised_before_commit = true; }
            }
            b.commit(root, seed1);
            std::vector<lig_diag_linear> lin(16);
            std::vector<lig_diag_quad> quad(16);
            b.diagnose_attached(lin.data(), lin.size(), quad.data(), quad.size(), &di);
            asked = {3u};                                  // a satisfied constraint on the first row ...
            for (uint64_t i = 0; i < di.n_linear_reported; i++) asked.push_back(lin[i].constraint);
            asked.push_back((uint32_t)(S - 1));            // ... and one on the last
            first = blank(asked.size()); with_values = blank(asked.size());
            Answer plain = blank(asked.size()), again = blank(asked.size());
            b.shard_explain_attached(asked.data(), asked.size(), first.con.data(), first.terms.data(), cap, &first.info);
            b.explain(asked.data(), asked.size(), plain.con.data(), plain.terms.data(), cap, &plain.info);
            same_as_explain = first.same(plain);
            try { b.explain_attached(asked.data(), asked.size(), again.con.data(), again.terms.data(), cap, &again.info); } catch (const std::logic_error&) { raised_attached = true; }
            b.set_linear_values(other.data(), S);
            b.shard_explain_attached(asked.data(), asked.size(), with_values.con.data(), with_values.terms.data(), cap, &with_values.info);
            b.explain(asked.data(), asked.size(), plain.con.data(), plain.terms.data(), cap, &plain.info);
            values_same_as_explain = with_values.same(plain) && !with_values.same(first);
            b.set_linear_values(nullptr, 0);
            b.shard_explain_attached(asked.data(), asked.size(), again.con.data(), again.terms.data(), cap, &again.info);
            same_after_values_removed = again.same(first);
            size_t len = 0;
            lig_proof_info info;
            (void)b.prove(nullptr, &len, &info);
            again = blank(asked.size());
            b.shard_explain_attached(asked.data(), asked.size(), again.con.data(), again.terms.data(), cap, &again.info);
            same_after_prove = len > 0 && !info.valid_linear && again.same(first);
            local = b.local_rows();
        }       // the batcher (and its shard) goes before the communicator
        std::printf("{\"rank\": %u, \"rows\": %zu, \"bad_slot\": %u, \"n_linear_bad\": %llu, \"asked\": [", rank, R, bad_slot, (unsigned long long)di.n_linear_bad);
        for (size_t i = 0; i < asked.size(); i++) std::printf("%s%u", i ? ", " : "", asked[i]);
        std::printf("], ");
        first.print("first");
        std::printf(", ");
        with_values.print("with_values");
        auto tf = [](bool v) { return v ? "true" : "false"; };
        std::printf(", \"raised_before_commit\": %s, \"raised_attached\": %s, \"raised_unsharded\": %s, \"same_as_explain\": %s, \"values_same_as_explain\": %s, "
                    "\"same_after_values_removed\": %s, \"same_after_prove\": %s, \"local_rows\": %zu}\n",
                    tf(raised_before_commit), tf(raised_attached), tf(raised_unsharded), tf(same_as_explain), tf(values_same_as_explain), tf(same_after_values_removed),
                    tf(same_after_prove), local);
        ok = 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rank %u error: %s\n", rank, e.what());
    }
    lig_ipc_comm_destroy(&comm);
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
