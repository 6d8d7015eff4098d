// sharded_values_batcher_prog.cpp -- hip_row_batcher::set_linear_values and ::diagnose_attached on a sharded batcher (shard_over +
// set_linear_system -> lig_shard_rows_set_linear_values, lig_shard_rows_diagnose_attached): ONE guest trace held by `world` processes
// (here all on GPU 0, communicator of csrc/comm_ipc.hip).  One structure, two tables: T1 makes the statement true for the guest's
// witness, T0 differs from it in the right-hand sides of two constraints (one on a row of the first rank, one on a row of the last) and
// in one term coefficient.  The sharded batcher is given the system with T0 and then the values T1; what it must reproduce comes from
// the UNSHARDED batcher on the same guest: the envelope of a batcher given the system with coefs = T1, and the records its
// diagnose_attached() returns under T0 -- which name exactly the three constraints the tables differ in.
//   usage: sharded_values_batcher_prog rank world /shm_name
// Prints one JSON line: {"rank", "unsharded_names_the_three", "values_envelope_equal", "after_reset_equal", "attached_zero_under_T1",
//                        "attached_equal_under_T0", "program_refused", "local_rows"}.
// TEST CODE: links oracle/liblig_oracle.so as the guest.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lig_hip_row_batcher.hpp"
#include "../../oracle/lig_oracle.h"

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
    // the structure: one constraint a_s * w[s] = b_s per witness slot; a_s = +1 except for slot `tab_slot`, whose coefficient is the table
    // entry S.  T1: b_s = the guest's witness, entry S = 1 -- the statement holds.
    const size_t S = R * (size_t)l;
    const uint32_t tab_slot = 5, rhs_first = 2 * l + 9, rhs_last = (uint32_t)((R - 1) * l + 11);      // rows 0, 2 and R - 1
    std::vector<uint32_t> term_begin(S + 1), rhs_c(S), rhs_b(S);
    std::vector<lig_lin_term> terms(S);
    std::vector<uint8_t> T1((S + 1) * 32, 0);
    for (size_t s = 0; s < S; s++) {
        term_begin[s] = (uint32_t)s;
        terms[s] = lig_lin_term{(uint32_t)s, s == tab_slot ? (uint32_t)S : (uint32_t)LIG_COEF_ONE};
        rhs_c[s] = (uint32_t)s; rhs_b[s] = (uint32_t)s;
        std::memcpy(&T1[32 * s], &rows[(s / l) * (size_t)k + s % l], 32);
    }
    term_begin[S] = (uint32_t)S;
    T1[32 * S] = 1;
    std::vector<uint8_t> T0 = T1;
    T0[32 * S] = 2;                                   // the term coefficient: 2 w = b is false
    T0[32 * (size_t)rhs_first] ^= 1;                  // (bit 0 of a canonical element: the entry stays below p)
    T0[32 * (size_t)rhs_last] ^= 1;
    auto system_with = [&](const std::vector<uint8_t>& tab) {
        lig_linear_system sys;
        std::memset(&sys, 0, sizeof sys);
        sys.struct_bytes = sizeof sys;
        sys.n_constraints = S; sys.n_terms = S; sys.n_rhs = S; sys.n_coefs = S + 1;
        sys.term_begin = term_begin.data(); sys.terms = terms.data(); sys.rhs_constraint = rhs_c.data(); sys.rhs_coef = rhs_b.data();
        sys.coefs = tab.data();
        return sys;
    };
    const lig_linear_system sys0 = system_with(T0), sys1 = system_with(T1);
    if (lig_linear_check(&sys0, kinds.data(), R, l) != LIG_OK || lig_linear_check(&sys1, kinds.data(), R, l) != LIG_OK) {
        std::fprintf(stderr, "lig_linear_check rejects a system\n");
        return 1;
    }

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
        auto pass1 = [&](ligero::hip_row_batcher& b) {
            for (size_t r = 0; r < R;) {
                if (kinds[r] == 0) { b.linear_callback(at(r)); r += 1; }
                else { b.quadratic_callback(at(r), at(r + 1), at(r + 2)); r += 3; }
            }
            b.mask_callback(k, 2 * (size_t)k, 2 * (size_t)k);
        };
        const uint64_t CAP = 16;
        struct Out { std::vector<lig_diag_linear> lin; std::vector<lig_diag_quad> quad; lig_diag_info info; };
        auto attached = [&](ligero::hip_row_batcher& b) {
            Out o;
            o.lin.assign(CAP, lig_diag_linear{}); o.quad.assign(CAP, lig_diag_quad{});
            std::memset(&o.info, 0, sizeof o.info);
            b.diagnose_attached(o.lin.data(), CAP, o.quad.data(), CAP, &o.info);
            return o;
        };
        auto same = [&](const Out& a, const Out& b) {
            return a.info.n_linear_bad == b.info.n_linear_bad && a.info.n_quad_bad == b.info.n_quad_bad && a.info.n_linear_reported == b.info.n_linear_reported &&
                   a.info.n_quad_reported == b.info.n_quad_reported && !std::memcmp(a.lin.data(), b.lin.data(), a.lin.size() * sizeof(lig_diag_linear)) &&
                   !std::memcmp(a.quad.data(), b.quad.data(), a.quad.size() * sizeof(lig_diag_quad));
        };
        auto zero = [](const Out& o) { return !o.info.n_linear_bad && !o.info.n_quad_bad && !o.info.n_linear_reported && !o.info.n_quad_reported; };
        struct Proved { std::vector<uint8_t> env; lig_proof_info info; };
        auto prove = [&](ligero::hip_row_batcher& b) {
            Proved p;
            size_t len = 0;
            const uint8_t* e = b.prove(nullptr, &len, &p.info);
            p.env.assign(e, e + len);
            return p;
        };
        uint8_t root[32], seed1[32];
        Proved fresh1;
        Out u0;
        {       // the unsharded batcher given the system with coefs = T1 ...
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_system(sys1);
            pass1(b);
            b.commit(root, seed1);
            fresh1 = prove(b);
        }
        {       // ... and given T0: what diagnose_attached() names
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_system(sys0);
            pass1(b);
            b.commit(root, seed1);
            u0 = attached(b);
            (void)prove(b);
        }
        const int names = fresh1.info.valid_linear && !fresh1.env.empty() && u0.info.n_linear_bad == 3 && u0.info.n_linear_reported == 3 && u0.info.n_quad_bad == 0 &&
                          u0.lin[0].constraint == tab_slot && u0.lin[1].constraint == rhs_first && u0.lin[2].constraint == rhs_last;
        int values_equal = 0, reset_equal = 0, zero_t1 = 0, equal_t0 = 0, refused = 0;
        size_t local = 0;
        {
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_system(sys0);
            b.shard_over(rank, world, &comm);
            try { b.set_linear_program(reinterpret_cast<const lig_linear_program*>(&sys0)); }      // (refused before the pointer is looked at)
            catch (const std::logic_error& e) { refused = std::string(e.what()).find("sharded") != std::string::npos; }
            b.set_linear_values(T1.data(), S + 1);          // before the commit: applied with the rank's share of the system
            pass1(b);
            b.commit(root, seed1);
            zero_t1 = zero(attached(b));
            const Proved p1 = prove(b);
            values_equal = p1.info.valid_linear && p1.env == fresh1.env;
            b.reset();                                      // the next proof: the shard restarts and keeps structure and values
            pass1(b);
            b.commit(root, seed1);
            const Proved p2 = prove(b);
            reset_equal = p2.info.valid_linear && p2.env == fresh1.env;
            b.reset();
            b.set_linear_values(nullptr, 0);                // back to the table the system came with
            pass1(b);
            b.commit(root, seed1);
            equal_t0 = same(u0, attached(b));
            const Proved p3 = prove(b);
            equal_t0 = equal_t0 && !p3.info.valid_linear && same(u0, attached(b));      // after prove(): the committed matrix is still there
            local = b.local_rows();
        }       // the batcher (and its shard) goes before the communicator
        ok = names && values_equal && reset_equal && zero_t1 && equal_t0 && refused;
        auto tf = [](int v) { return v ? "true" : "false"; };
        std::printf("{\"rank\": %u, \"unsharded_names_the_three\": %s, \"values_envelope_equal\": %s, \"after_reset_equal\": %s, \"attached_zero_under_T1\": %s, "
                    "\"attached_equal_under_T0\": %s, \"program_refused\": %s, \"local_rows\": %zu}\n", rank, tf(names), tf(values_equal), tf(reset_equal), tf(zero_t1),
                    tf(equal_t0), tf(refused), local);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rank %u error: %s\n", rank, e.what());
    }
    lig_ipc_comm_destroy(&comm);
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
