// sharded_diagnose_batcher_prog.cpp -- hip_row_batcher::diagnose on a sharded batcher (shard_over + set_linear_system): ONE guest trace
// with ONE wrong witness slot, held by `world` processes (here all on GPU 0, communicator of csrc/comm_ipc.hip).  Every rank hands the
// batcher the term list of the WHOLE trace, commits and calls diagnose(): a collective call whose output on every rank must be, byte for
// byte, that of the unsharded batcher on the same guest -- which names exactly the constraint on the changed slot (and, the slot being an
// x of a triple, that triple's column).   usage: sharded_diagnose_batcher_prog rank world /shm_name
// Prints one JSON line: {"rank", "unsharded_names_the_slot", "equal_unsharded", "counts_only_equal", "proved_after", "local_rows"}.
// TEST CODE: links oracle/liblig_oracle.so as the guest.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    if (lig_linear_check(&sys, kinds.data(), R, l) != LIG_OK) { std::fprintf(stderr, "lig_linear_check rejects the system\n"); return 1; }
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
        auto pass1 = [&](ligero::hip_row_batcher& b) {
            for (size_t r = 0; r < R;) {
                if (kinds[r] == 0) { b.linear_callback(at(r)); r += 1; }
                else { b.quadratic_callback(at(r), at(r + 1), at(r + 2)); r += 3; }
            }
            b.mask_callback(k, 2 * (size_t)k, 2 * (size_t)k);
        };
        const uint64_t CAP = 16;
        struct Out { std::vector<lig_diag_linear> lin; std::vector<lig_diag_quad> quad; lig_diag_info info; };
        auto run = [&](ligero::hip_row_batcher& b, uint64_t cap) {
            Out o;
            o.lin.assign(cap, lig_diag_linear{}); o.quad.assign(cap, lig_diag_quad{});
            std::memset(&o.info, 0, sizeof o.info);
            b.diagnose(cap ? o.lin.data() : nullptr, cap, cap ? o.quad.data() : nullptr, cap, &o.info);
            return o;
        };
        auto same = [&](const Out& a, const Out& b) {
            return a.info.n_linear_bad == b.info.n_linear_bad && a.info.n_quad_bad == b.info.n_quad_bad && a.info.n_linear_reported == b.info.n_linear_reported &&
                   a.info.n_quad_reported == b.info.n_quad_reported &&
                   (a.lin.empty() || !std::memcmp(a.lin.data(), b.lin.data(), a.lin.size() * sizeof(lig_diag_linear))) &&
                   (a.quad.empty() || !std::memcmp(a.quad.data(), b.quad.data(), a.quad.size() * sizeof(lig_diag_quad)));
        };
        uint8_t root[32], seed1[32];
        Out u, u0;
        {
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_system(sys);
            pass1(b);
            b.commit(root, seed1);
            u = run(b, CAP);
            u0 = run(b, 0);
            size_t len = 0;
            (void)b.prove(nullptr, &len);
        }
        // what the unsharded batcher must have said, stated from the guest alone: the constraint on the changed slot, and its triple's column
        const int names = u.info.n_linear_bad == 1 && u.info.n_linear_reported == 1 && u.lin[0].constraint == bad_slot && u.info.n_quad_bad == 1 &&
                          u.info.n_quad_reported == 1 && u.quad[0].row_x == bad_row && u.quad[0].row_y == bad_row + 1 && u.quad[0].row_z == bad_row + 2 &&
                          u.quad[0].column == bad_col;
        int equal = 0, counts = 0, proved = 0;
        size_t local = 0;
        {
            ligero::hip_row_batcher b(ctx, meta);
            b.set_linear_system(sys);
            b.shard_over(rank, world, &comm);
            pass1(b);
            b.commit(root, seed1);
            const Out s1 = run(b, CAP), s0 = run(b, 0);
            equal = same(u, s1);
            counts = same(u0, s0);
            size_t len = 0;
            lig_proof_info info;
            (void)b.prove(nullptr, &len, &info);
            const Out s2 = run(b, CAP);                 // after prove(): the committed matrix is still there
            proved = len > 0 && !info.valid_linear && same(u, s2);
            local = b.local_rows();
        }       // the batcher (and its shard) goes before the communicator
        ok = names && equal && counts && proved;
        auto tf = [](int v) { return v ? "true" : "false"; };
        std::printf("{\"rank\": %u, \"unsharded_names_the_slot\": %s, \"equal_unsharded\": %s, \"counts_only_equal\": %s, \"proved_after\": %s, \"local_rows\": %zu}\n", rank,
                    tf(names), tf(equal), tf(counts), tf(proved), local);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rank %u error: %s\n", rank, e.what());
    }
    lig_ipc_comm_destroy(&comm);
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
