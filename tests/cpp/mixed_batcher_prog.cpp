// mixed_batcher_prog.cpp -- hip_proof_meta::wide_slots: a guest whose linear rows are bits with a few machine words (and one value
// above 8 bytes) among them goes through the row-batching shim.  With narrow_rows = narrowest = true alone the OR of a row's slots
// decides and such a row travels 4 or 8 bytes (or 32) wide; with wide_slots it stays a bit row that carries its wide slots as 36-byte
// records (lig_rows_job.wide_per_row).  Both must give the oracle's envelope over the same rows; the bytes each leg ships are
// compared with the arithmetic of the format, worked out here slot by slot.  The oracle plays guest + witness_manager
// (lo_form_rows: rows with their pads), the data slots are then overwritten.
//   usage: mixed_batcher_prog                       one GPU: narrowest alone, with wide_slots (twice: the second proof restarts the
//                                                    trace), and with wide_slots but without narrowest (no effect)
//          mixed_batcher_prog rank world /shm_name   one trace sharded over `world` processes (comm_ipc): narrowest alone, with wide_slots
// Prints one JSON line.
// TEST CODE: links oracle/liblig_oracle.so as the checker.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/lig_hip_row_batcher.hpp"
#include "../../oracle/lig_oracle.h"

static const uint32_t l = 320, k = 512, n = 2048;

// bytes of one row by the rules of the format: OR of the slots (narrowest) / the cheapest base + 36 per misfit (wide_slots)
static unsigned cls(const lo_fr& v) {
    const uint64_t* w = reinterpret_cast<const uint64_t*>(&v);
    if (w[1] | w[2] | w[3]) return 5;
    return w[0] <= 1 ? 0 : w[0] <= 0xff ? 1 : w[0] <= 0xffff ? 2 : w[0] <= 0xffffffffu ? 3 : 4;
}
static size_t base_bytes(unsigned b) { return b == 0 ? (l + 31) / 32 * 4 : ((size_t)l * (1u << (b - 1)) + 3) / 4 * 4; }
static size_t row_bytes(const lo_fr* row, bool mixed) {
    size_t cnt[6] = {0, 0, 0, 0, 0, 0};
    unsigned top = 0;
    for (uint32_t i = 0; i < l; i++) { cnt[cls(row[i])]++; if (cls(row[i]) > top) top = cls(row[i]); }
    if (!mixed) return top == 5 ? (size_t)k * 32 : base_bytes(top);
    size_t best = (size_t)k * 32, misfit = l;
    for (unsigned b = 0; b < 5; b++) { misfit -= cnt[b]; if (base_bytes(b) + 36 * misfit < best) best = base_bytes(b) + 36 * misfit; }
    return best;
}

int main(int argc, char** argv) {
    const bool sharded = argc >= 4;
    const uint32_t rank = sharded ? std::atoi(argv[1]) : 0, world = sharded ? std::atoi(argv[2]) : 1;
    lo_job j;
    std::memset(&j, 0, sizeof j);
    j.l = l; j.k = k; j.n = n; j.t = 192;
    j.n_linear = 320 * 60 + 7;
    j.n_quad = 320 * 2 + 5;
    for (int i = 0; i < 32; i++) j.encoding_seed[i] = (uint8_t)(5 * i + 3);
    lo_synth_key(11, j.witness_key);
    j.generated_at = 4343;
    j.threads = 4;
    const size_t R = lo_job_rows(&j) - 3;
    std::vector<lo_fr> rows((R ? R : 1) * (size_t)k), mc(k), ml(2 * (size_t)k), mq(2 * (size_t)k);
    std::vector<uint8_t> kinds(R ? R : 1);
    lo_form_rows(&j, rows.data(), mc.data(), ml.data(), mq.data());
    lo_row_kinds(&j, kinds.data());
    // the guest's witness.  Linear rows: bits; every third row has two 32-bit and one 64-bit word among them (columns 0, 77, l - 1),
    // every seventh a value of 200 bits as well, every eleventh row is bytes throughout.  x rows: bits with a 32-bit word in column 5
    // over a bit of y; z = x * y.  Pads (slots l..k-1) stay as formed
    uint64_t st = 0x9E3779B97F4A7C15ull;
    auto next = [&] { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    for (size_t r = 0; r < R; r++) {
        lo_fr* row = rows.data() + r * (size_t)k;
        uint64_t* w = reinterpret_cast<uint64_t*>(row);
        if (kinds[r] <= 2) {
            for (uint32_t i = 0; i < l; i++) {
                std::memset(&row[i], 0, sizeof(lo_fr));
                w[4 * i] = kinds[r] == 0 && r % 11 == 10 ? (i == 1 ? 255 : next() & 0xff) : (i == 1 ? 1 : next() & 1);
            }
            if (kinds[r] == 0 && r % 3 == 0) { w[0] = 0xFFFFFFFFull; w[4 * 77] = 0x80000000ull | (next() & 0xffff); w[4 * (l - 1)] = ~0ull; }
            if (kinds[r] == 0 && r % 7 == 0) w[4 * 100 + 3] = 0x80;                                   // 2^199
            if (kinds[r] == 1) w[4 * 5] = 0x12345678ull;
            if (kinds[r] == 2) w[4 * 5] = 1;
        } else if (kinds[r] == 3) {
            const uint64_t* x = reinterpret_cast<const uint64_t*>(rows.data() + (r - 2) * (size_t)k);
            const uint64_t* y = reinterpret_cast<const uint64_t*>(rows.data() + (r - 1) * (size_t)k);
            for (uint32_t i = 0; i < l; i++) {
                std::memset(&row[i], 0, sizeof(lo_fr));
                w[4 * i] = x[4 * i] * y[4 * i];
            }
        }
    }
    lig_ctx* ctx = nullptr;
    if (lig_ctx_create(&ctx, 0, l, k, n) != LIG_OK) { std::fprintf(stderr, "ctx: %s\n", ctx ? lig_last_error(ctx) : "?"); return 1; }
    lig_comm comm;
    if (sharded && lig_ipc_comm_create(ctx, argv[3], rank, world, &comm) != LIG_OK) { std::fprintf(stderr, "comm: %s\n", lig_last_error(ctx)); return 1; }
    int ok = 0;
    try {
        auto at = [&](const std::vector<lo_fr>& v, size_t r) { return reinterpret_cast<const uint64_t*>(v.data() + r * (size_t)k); };
        // the rows this rank ships (the deal of lig_shard_rows_plan; all rows on one GPU)
        std::vector<uint8_t> mine(R, sharded ? 0 : 1);
        if (sharded) {
            uint64_t rounds = 0;
            std::vector<uint64_t> bd((size_t)world * ((R + 511) / 512 + 2) + 2);
            if (lig_shard_rows_plan(kinds.data(), R, world, &rounds, bd.data(), bd.size()) != LIG_OK) throw std::runtime_error("lig_shard_rows_plan failed");
            for (uint64_t g = rank; g < rounds * world; g += world) for (uint64_t r = bd[g]; r < bd[g + 1]; r++) mine[r] = 1;
        }
        size_t want[2] = {0, 0}, mixed_rows = 0;
        for (size_t r = 0; r < R; r++) {
            if (!mine[r]) continue;
            for (int m = 0; m < 2; m++) want[m] += row_bytes(rows.data() + r * (size_t)k, m == 1);
            mixed_rows += row_bytes(rows.data() + r * (size_t)k, true) != row_bytes(rows.data() + r * (size_t)k, false);
        }
        lo_proof P;
        bool have_oracle = false;
        std::vector<lo_fr> rands((R ? R : 1) * (size_t)k);
        // one proof through batcher `b`: commit, the oracle's randomness rows for the seed, prove; true = the oracle's envelope
        auto prove = [&](ligero::hip_row_batcher& b) {
            auto replay = [&](const std::vector<lo_fr>* rd) {
                for (size_t r = 0; r < R;) {
                    if (kinds[r] == 0) { b.linear_callback(at(rows, r), rd ? at(*rd, r) : nullptr); r += 1; }
                    else {
                        b.quadratic_callback(at(rows, r), at(rows, r + 1), at(rows, r + 2), rd ? at(*rd, r) : nullptr, rd ? at(*rd, r + 1) : nullptr,
                                             rd ? at(*rd, r + 2) : nullptr);
                        r += 3;
                    }
                }
                b.mask_callback(k, 2 * (size_t)k, 2 * (size_t)k);
            };
            replay(nullptr);
            uint8_t root[32], seed1[32];
            b.commit(root, seed1);
            lo_fr cs;
            lo_rand_rows(&j, seed1, rands.data(), &cs);
            replay(&rands);
            size_t len = 0;
            lig_proof_info info;
            const uint8_t* proof = b.prove(nullptr, &len, &info);
            if (!have_oracle) {
                if (lo_prove_rows(&j, kinds.data(), R, rows.data(), mc.data(), ml.data(), mq.data(), rands.data(), nullptr, &P) != 0)
                    throw std::runtime_error("oracle prover failed");
                have_oracle = true;
            }
            return len == P.proof_len && !std::memcmp(proof, P.proof, len) && !std::memcmp(root, P.root, 32);
        };
        ligero::hip_proof_meta meta;
        std::memcpy(meta.encoding_seed, j.encoding_seed, 32);
        meta.generated_at = j.generated_at;
        meta.narrow_rows = true;
        meta.narrowest = true;
        size_t shipped[4] = {0, 0, 0, 0};
        bool good = true;
        {
            ligero::hip_row_batcher b(ctx, meta);          // narrowest alone: today's bytes
            if (sharded) b.shard_over(rank, world, &comm);
            good = prove(b) && good;
            shipped[0] = b.shipped_bytes();
        }
        {
            meta.wide_slots = true;
            ligero::hip_row_batcher b(ctx, meta);
            if (sharded) b.shard_over(rank, world, &comm);
            good = prove(b) && good;
            shipped[1] = b.shipped_bytes();
            b.reset();                                     // the next proof of the same program: lig_rows_restart with the same counts
            good = prove(b) && good;
            shipped[2] = b.shipped_bytes();
        }
        if (!sharded) {
            meta.narrowest = false;                        // wide_slots without narrowest: no effect, 8 bytes per slot or full rows
            ligero::hip_row_batcher b(ctx, meta);
            good = prove(b) && good;
            shipped[3] = b.shipped_bytes();
            meta.wide_slots = false;
            ligero::hip_row_batcher b2(ctx, meta);
            good = prove(b2) && good;
            good = good && b2.shipped_bytes() == shipped[3];
        }
        ok = good;
        std::printf("{\"rank\": %u, \"equals_oracle\": %s, \"local_rows\": %zu, \"mixed_rows\": %zu, \"shipped_narrowest\": %zu, \"shipped_mixed\": %zu, "
                    "\"shipped_mixed_again\": %zu, \"shipped_without_narrowest\": %zu, \"want_narrowest\": %zu, \"want_mixed\": %zu}\n",
                    rank, ok ? "true" : "false", (size_t)std::count(mine.begin(), mine.end(), 1), mixed_rows, shipped[0], shipped[1], shipped[2],
                    shipped[3], want[0], want[1]);
        if (have_oracle) lo_proof_free(&P);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rank %u error: %s\n", rank, e.what());
    }
    if (sharded) lig_ipc_comm_destroy(&comm);
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
