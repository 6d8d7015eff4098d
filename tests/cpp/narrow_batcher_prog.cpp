// narrow_batcher_prog.cpp -- hip_proof_meta::narrowest: a guest whose witness rows hold bits and bytes goes through the row-batching
// shim with narrow_rows = narrowest = true; each linear / x / y / z row is shipped in the narrowest width its data slots fit (bit rows
// as LIG_ELEM_BIT, byte rows as 1 byte per slot), and the envelope must be the oracle's prover over the same rows.  The oracle plays
// guest + witness_manager (lo_form_rows: rows with their pads), the data slots are then overwritten.
//   usage: narrow_batcher_prog                       one GPU
//          narrow_batcher_prog rank world /shm_name   one trace sharded over `world` processes (comm_ipc)
// Prints one JSON line: {"rank", "equals_oracle", "shipped_bytes", "full_bytes"}.
// TEST CODE: links oracle/liblig_oracle.so as the checker.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/lig_hip_row_batcher.hpp"
#include "../../oracle/lig_oracle.h"

int main(int argc, char** argv) {
    const bool sharded = argc >= 4;
    const uint32_t rank = sharded ? std::atoi(argv[1]) : 0, world = sharded ? std::atoi(argv[2]) : 1;
    const uint32_t l = 320, k = 512, n = 2048;
    lo_job j;
    std::memset(&j, 0, sizeof j);
    j.l = l; j.k = k; j.n = n; j.t = 192;
    j.n_linear = 320 * 700 + 7;                       // two stage-1 chunks, several exchange rounds when sharded
    j.n_quad = 320 * 2 + 5;
    for (int i = 0; i < 32; i++) j.encoding_seed[i] = (uint8_t)(3 * i + 5);
    lo_synth_key(9, j.witness_key);
    j.generated_at = 4242;
    j.threads = 4;
    const size_t R = lo_job_rows(&j) - 3;
    std::vector<lo_fr> rows((R ? R : 1) * (size_t)k), mc(k), ml(2 * (size_t)k), mq(2 * (size_t)k);
    std::vector<uint8_t> kinds(R ? R : 1);
    lo_form_rows(&j, rows.data(), mc.data(), ml.data(), mq.data());
    lo_row_kinds(&j, kinds.data());
    // the guest's witness: linear rows alternate bytes and bits, the rows of x * y = z are bits; pads (slots l..k-1) stay as formed
    uint64_t st = 0x9E3779B97F4A7C15ull;
    auto next = [&] { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    for (size_t r = 0; r < R; r++) {
        lo_fr* row = rows.data() + r * (size_t)k;
        if (kinds[r] == 0 || kinds[r] == 1 || kinds[r] == 2) {
            const bool bytes = kinds[r] == 0 && r % 2 == 0;
            for (uint32_t i = 0; i < l; i++) {
                std::memset(&row[i], 0, sizeof(lo_fr));
                row[i].v[0] = bytes ? (i == 0 ? 255 : next() & 0xff) : (i == 0 ? 1 : next() & 1);
            }
        } else if (kinds[r] == 3) {
            const lo_fr* x = rows.data() + (r - 2) * (size_t)k;
            const lo_fr* y = rows.data() + (r - 1) * (size_t)k;
            for (uint32_t i = 0; i < l; i++) {
                std::memset(&row[i], 0, sizeof(lo_fr));
                row[i].v[0] = x[i].v[0] * y[i].v[0];
            }
        }
    }
    lig_ctx* ctx = nullptr;
    if (lig_ctx_create(&ctx, 0, l, k, n) != LIG_OK) { std::fprintf(stderr, "ctx: %s\n", ctx ? lig_last_error(ctx) : "?"); return 1; }
    lig_comm comm;
    if (sharded && lig_ipc_comm_create(ctx, argv[3], rank, world, &comm) != LIG_OK) { std::fprintf(stderr, "comm: %s\n", lig_last_error(ctx)); return 1; }
    int ok = 0;
    try {
        ligero::hip_proof_meta meta;
        std::memcpy(meta.encoding_seed, j.encoding_seed, 32);
        meta.generated_at = j.generated_at;
        meta.narrow_rows = true;
        meta.narrowest = true;
        {
            ligero::hip_row_batcher b(ctx, meta);
            if (sharded) b.shard_over(rank, world, &comm);
            auto at = [&](const std::vector<lo_fr>& v, size_t r) { return reinterpret_cast<const uint64_t*>(v.data() + r * (size_t)k); };
            auto replay = [&](const std::vector<lo_fr>* rands) {
                for (size_t r = 0; r < R;) {
                    if (kinds[r] == 0) { b.linear_callback(at(rows, r), rands ? at(*rands, r) : nullptr); r += 1; }
                    else {
                        b.quadratic_callback(at(rows, r), at(rows, r + 1), at(rows, r + 2), rands ? at(*rands, r) : nullptr,
                                             rands ? at(*rands, r + 1) : nullptr, rands ? at(*rands, r + 2) : nullptr);
                        r += 3;
                    }
                }
                b.mask_callback(k, 2 * (size_t)k, 2 * (size_t)k);
            };
            replay(nullptr);
            uint8_t root[32], seed1[32];
            b.commit(root, seed1);
            std::vector<lo_fr> rands((R ? R : 1) * (size_t)k);
            lo_fr cs;
            lo_rand_rows(&j, seed1, rands.data(), &cs);
            replay(&rands);
            size_t len = 0;
            lig_proof_info info;
            const uint8_t* proof = b.prove(nullptr, &len, &info);
            lo_proof P;
            if (lo_prove_rows(&j, kinds.data(), R, rows.data(), mc.data(), ml.data(), mq.data(), rands.data(), nullptr, &P) != 0)
                throw std::runtime_error("oracle prover failed");
            ok = len == P.proof_len && !std::memcmp(proof, P.proof, len) && !std::memcmp(root, P.root, 32);
            std::printf("{\"rank\": %u, \"equals_oracle\": %s, \"local_rows\": %zu, \"shipped_bytes\": %zu, \"full_bytes\": %zu}\n", rank,
                        ok ? "true" : "false", b.local_rows(), b.shipped_bytes(), b.local_rows() * (size_t)k * 32);
            lo_proof_free(&P);
        }       // the batcher (and its shard) goes before the communicator
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rank %u error: %s\n", rank, e.what());
    }
    if (sharded) lig_ipc_comm_destroy(&comm);
    lig_ctx_destroy(ctx);
    return ok ? 0 : 1;
}
