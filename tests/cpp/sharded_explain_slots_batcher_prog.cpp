// sharded_explain_slots_batcher_prog.cpp -- hip_row_batcher::shard_explain_slots* / shard_untouched_slots* on a sharded batcher (shard_over +
// set_linear_system -> lig_shard_rows_explain_slots*, lig_shard_rows_untouched_slots*): ONE guest trace with ONE wrong witness slot, held by
// `world` processes (here all on GPU 0, communicator of csrc/comm_ipc.hip).  Every rank sets the system of the WHOLE trace -- constraint s
// is w[s] = b_s, but for s % 64 == 7 it is w[s + 1] = b_s: slot s is touched by nothing, slot s + 1 by two constraints --, commits, and asks
// for slots on rows of the first and of the last rank's share, the wrong one among them: a collective call over the ranks' shares whose
// records must be the bytes of the term-list form on the same batcher, on every rank; with set_linear_values() the records follow the
// values; the same bytes come back after prove().  std::logic_error: before commit(), on an unsharded batcher, and from the unsharded
// members on the sharded one.   usage: sharded_explain_slots_batcher_prog rank world /shm_name
// Prints one JSON line with every record; tests/test_gpu_shard_explain_slots_batcher.py changes the same slot in its own copy of the rows
// and compares with tests/slots_ref.py.
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
    std::vector<lig_slot_record> rec;
    std::vector<lig_slot_term> terms;
    lig_slot_info info;
    bool same(const Answer& o) const {
        return info.n_terms_total == o.info.n_terms_total && info.n_terms_reported == o.info.n_terms_reported &&
               info.n_constraints_distinct == o.info.n_constraints_distinct && rec.size() == o.rec.size() &&
               !std::memcmp(rec.data(), o.rec.data(), rec.size() * sizeof(lig_slot_record)) &&
               !std::memcmp(terms.data(), o.terms.data(), info.n_terms_reported * sizeof(lig_slot_term));
    }
    void print(const char* name) const {
        std::printf("\"%s\": {\"counts\": [%llu, %llu, %llu], \"slots\": [", name, (unsigned long long)info.n_terms_total, (unsigned long long)info.n_terms_reported,
                    (unsigned long long)info.n_constraints_distinct);
        for (size_t i = 0; i < rec.size(); i++)
            std::printf("%s[%u, %u, %llu, %llu, \"%s\"]", i ? ", " : "", rec[i].slot, rec[i].row_kind, (unsigned long long)rec[i].n_terms, (unsigned long long)rec[i].first_term,
                        hex32(rec[i].value).c_str());
        std::printf("], \"terms\": [");
        for (uint64_t i = 0; i < info.n_terms_reported; i++)
            std::printf("%s[%u, %u, %u, %u, \"%s\", \"%s\"]", i ? ", " : "", terms[i].slot, terms[i].constraint, terms[i].coef_index, terms[i].constraint_terms,
                        hex32(terms[i].coef).c_str(), hex32(terms[i].residual).c_str());
        std::printf("]}");
    }
};
struct Untouched {
    std::vector<lig_slot_value> out;
    lig_untouched_info info;
    bool same(const Untouched& o) const {
        return info.n_untouched == o.info.n_untouched && info.n_untouched_nonzero == o.info.n_untouched_nonzero && info.n_reported == o.info.n_reported &&
               !std::memcmp(out.data(), o.out.data(), info.n_reported * sizeof(lig_slot_value));
    }
    void print(const char* name) const {
        std::printf("\"%s\": {\"counts\": [%llu, %llu, %llu], \"values\": [", name, (unsigned long long)info.n_untouched, (unsigned long long)info.n_untouched_nonzero,
                    (unsigned long long)info.n_reported);
        for (uint64_t i = 0; i < info.n_reported; i++) std::printf("%s[%u, %u, \"%s\"]", i ? ", " : "", out[i].slot, out[i].row_kind, hex32(out[i].value).c_str());
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
    j.n_linear = 320 * 5;                             // full rows only
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
    // the statement: constraint s is w[slot_of(s)] = b_s, b_s taken from the honest witness; slot_of(s) = s + 1 for s % 64 == 7, else s
    const size_t S = R * (size_t)l;
    auto slot_of = [](size_t s) { return s % 64 == 7 ? s + 1 : s; };
    std::vector<uint32_t> term_begin(S + 1), rhs_c(S), rhs_b(S);
    std::vector<lig_lin_term> terms(S);
    std::vector<uint8_t> coefs(S * 32);
    for (size_t s = 0; s < S; s++) {
        const size_t at = slot_of(s);
        term_begin[s] = (uint32_t)s;
        terms[s] = lig_lin_term{(uint32_t)at, LIG_COEF_ONE};
        rhs_c[s] = (uint32_t)s; rhs_b[s] = (uint32_t)s;
        std::memcpy(&coefs[32 * s], &rows[(at / l) * (size_t)k + at % l], 32);
    }
    term_begin[S] = (uint32_t)S;
    lig_linear_system sys;
    std::memset(&sys, 0, sizeof sys);
    sys.struct_bytes = sizeof sys;
    sys.n_constraints = S; sys.n_terms = S; sys.n_rhs = S; sys.n_coefs = S;
    sys.term_begin = term_begin.data(); sys.terms = terms.data(); sys.rhs_constraint = rhs_c.data(); sys.rhs_coef = rhs_b.data();
    sys.coefs = coefs.data();
    // another statement of the same structure: the right-hand side of constraint 8 (slot 8 of the first rank's share: two constraints) changes
    std::vector<uint8_t> other = coefs;
    other[32 * 8] ^= 2;
    // ... and then one witness slot changes: column 9 of the last QX row of the trace (a row of the last rank's share)
    size_t bad_row = R;
    for (size_t r = 0; r < R; r++) if (kinds[r] == 1) bad_row = r;
    if (bad_row == R) { std::fprintf(stderr, "no QX row\n"); return 1; }
    const uint32_t bad_col = 9, bad_slot = (uint32_t)(bad_row * l + bad_col);
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
        const uint64_t cap = 16, ucap = 6;
        auto blank = [&](size_t n_asked) { Answer a; a.rec.resize(n_asked); a.terms.resize(cap); std::memset(&a.info, 0, sizeof a.info); return a; };
        auto ublank = [&]() { Untouched u; u.out.resize(ucap); std::memset(&u.info, 0, sizeof u.info); return u; };
        uint8_t root[32], seed1[32];
        int raised_before_commit = 0, raised_unsharded_members = 0, raised_unsharded = 0;
        bool same_as_list = false, values_same_as_list = false, same_after_values_removed = false, same_after_prove = false, untouched_same_as_list = false;
        size_t local = 0;
        // slots 7 (no term), 8 (two constraints), 9 on the first row; the changed slot and its neighbour; the last slot of the trace
        const std::vector<uint32_t> asked = {7u, 8u, 9u, bad_slot, bad_slot + 1, (uint32_t)(S - 1)};
        Answer first, with_values;
        Untouched un, un_nonzero;
        auto four_raise = [&](ligero::hip_row_batcher& b, bool shard_members) {      // how many of the four members throw std::logic_error
            int raised = 0;
            Answer a = blank(1);
            Untouched u = ublank();
            const uint32_t one = 0;
            for (int which = 0; which < 4; which++) {
                try {
                    if (shard_members) {
                        if (which == 0) b.shard_explain_slots(&one, 1, a.rec.data(), a.terms.data(), cap, &a.info);
                        if (which == 1) b.shard_explain_slots_attached(&one, 1, a.rec.data(), a.terms.data(), cap, &a.info);
                        if (which == 2) b.shard_untouched_slots(false, u.out.data(), ucap, &u.info);
                        if (which == 3) b.shard_untouched_slots_attached(false, u.out.data(), ucap, &u.info);
                    } else {
                        if (which == 0) b.explain_slots(&one, 1, a.rec.data(), a.terms.data(), cap, &a.info);
                        if (which == 1) b.explain_slots_attached(&one, 1, a.rec.data(), a.terms.data(), cap, &a.info);
                        if (which == 2) b.untouched_slots(false, u.out.data(), ucap, &u.info);
                        if (which == 3) b.untouched_slots_attached(false, u.out.data(), ucap, &u.info);
                    }
                } catch (const std::logic_error&) { raised++; }
            }
            return raised;
        };
        {
            ligero::hip_row_batcher u(ctx, meta);         // never sharded: nothing is launched
            u.set_linear_system(sys);
            raised_unsharded = four_raise(u, true);
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
            raised_before_commit = four_raise(b, true);
            b.commit(root, seed1);
            raised_unsharded_members = four_raise(b, false);
            first = blank(asked.size()); with_values = blank(asked.size());
            Answer plain = blank(asked.size()), again = blank(asked.size());
            b.shard_explain_slots_attached(asked.data(), asked.size(), first.rec.data(), first.terms.data(), cap, &first.info);
            b.shard_explain_slots(asked.data(), asked.size(), plain.rec.data(), plain.terms.data(), cap, &plain.info);
            same_as_list = first.same(plain);
            un = ublank(); un_nonzero = ublank();
            Untouched uplain = ublank();
            b.shard_untouched_slots_attached(false, un.out.data(), ucap, &un.info);
            b.shard_untouched_slots(false, uplain.out.data(), ucap, &uplain.info);
            untouched_same_as_list = un.same(uplain);
            b.shard_untouched_slots_attached(true, un_nonzero.out.data(), 2, &un_nonzero.info);
            b.set_linear_values(other.data(), S);
            b.shard_explain_slots_attached(asked.data(), asked.size(), with_values.rec.data(), with_values.terms.data(), cap, &with_values.info);
            b.shard_explain_slots(asked.data(), asked.size(), plain.rec.data(), plain.terms.data(), cap, &plain.info);
            values_same_as_list = with_values.same(plain) && !with_values.same(first);
            b.set_linear_values(nullptr, 0);
            b.shard_explain_slots_attached(asked.data(), asked.size(), again.rec.data(), again.terms.data(), cap, &again.info);
            same_after_values_removed = again.same(first);
            size_t len = 0;
            lig_proof_info info;
            (void)b.prove(nullptr, &len, &info);
            again = blank(asked.size());
            b.shard_explain_slots_attached(asked.data(), asked.size(), again.rec.data(), again.terms.data(), cap, &again.info);
            same_after_prove = len > 0 && !info.valid_linear && again.same(first);
            local = b.local_rows();
        }       // the batcher (and its shard) goes before the communicator
        std::printf("{\"rank\": %u, \"rows\": %zu, \"bad_slot\": %u, \"asked\": [", rank, R, bad_slot);
        for (size_t i = 0; i < asked.size(); i++) std::printf("%s%u", i ? ", " : "", asked[i]);
        std::printf("], ");
        first.print("first");
        std::printf(", ");
        with_values.print("with_values");
        std::printf(", ");
        un.print("untouched");
        std::printf(", ");
        un_nonzero.print("untouched_nonzero");
        auto tf = [](bool v) { return v ? "true" : "false"; };
        std::printf(", \"raised_before_commit\": %d, \"raised_unsharded_members\": %d, \"raised_unsharded\": %d, \"same_as_list\": %s, \"values_same_as_list\": %s, "
                    "\"untouched_same_as_list\": %s, \"same_after_values_removed\": %s, \"same_after_prove\": %s, \"local_rows\": %zu}\n",
                    raised_before_commit, raised_unsharded_members, raised_unsharded, tf(same_as_list), tf(values_same_as_list), tf(untouched_same_as_list),
                    tf(same_after_values_removed), tf(same_after_prove), local);
        ok = 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rank %u error: %s\n", rank, e.what());
    }
    lig_ipc_comm_destroy(&comm);
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
