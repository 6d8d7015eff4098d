// upload_plan_prog -- the host-side rules of bringing caller rows from host memory (ligero-prover_amd/csrc/upload_plan.hpp) without a
// GPU and without the library: which queued job the uploader thread takes, presence masks as copy / zero-fill runs, the jobs of a
// chunk schedule, the words of the flag pages of a trace and of a shard.
// Build: g++ -std=c++17 -fsanitize=address,undefined tests/cpp/upload_plan_prog.cpp   (tests/test_upload_plan.py)
#include <algorithm>
#include <cstdio>
#include <random>
#include <utility>

#include "../../ligero-prover_amd/csrc/upload_plan.hpp"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

// ---- the pick rule
static std::atomic<int> g_failed{0}, g_pending{0};
static uint32_t g_arrived[8];
static UploadJob job(int prio, const volatile uint32_t* wait = nullptr, uint32_t wait_val = 0, const std::atomic<int>* abort = nullptr) {
    UploadJob j{nullptr, nullptr, 0, g_arrived, 1, &g_failed};
    j.wait = wait; j.wait_val = wait_val; j.abort = abort; j.prio = prio;
    return j;
}
static size_t pick(const std::vector<UploadJob>& jobs) {
    std::deque<QueuedUpload> q;
    for (const UploadJob& j : jobs) q.push_back({j, &g_pending});
    const size_t i = lig::upload_pick(q);
    return i == q.size() ? (size_t)-1 : i;
}
static void test_pick() {
    const size_t none = (size_t)-1;
    const uint32_t unmet = 4, met = 5;                                      // words a proof would write; the jobs below wait for 5
    std::atomic<int> abort_off{0}, abort_on{1};
    CHECK(pick({}) == none);
    CHECK(pick({job(0, &unmet, 5), job(1, &unmet, 5)}) == none);            // every job waits on an unmet word
    CHECK(pick({job(0), job(0), job(0)}) == 0);                             // the oldest ready job among equals
    CHECK(pick({job(1), job(1)}) == 0);
    CHECK(pick({job(0, &unmet, 5), job(0), job(0)}) == 1);
    CHECK(pick({job(0, &unmet, 5), job(0, &met, 5), job(0)}) == 1);
    CHECK(pick({job(0), job(0), job(1), job(1)}) == 2);                     // a later ready urgent job beats an earlier ready one; the scan stops there
    CHECK(pick({job(0), job(1, &unmet, 5)}) == 0);                          // an unready urgent job does not
    CHECK(pick({job(0, &unmet, 5), job(1, &unmet, 5), job(0), job(1, &met, 5)}) == 3);
    CHECK(pick({job(0, &unmet, 5, &abort_off)}) == none);
    CHECK(pick({job(0, &unmet, 5, &abort_on)}) == 0);                       // an abort flag makes a waiting job ready (it is dropped, its word published)
    CHECK(pick({job(0), job(1, &unmet, 5, &abort_on)}) == 1);
    const uint32_t one = 1, big = 0xfffffffeu;                              // sequence numbers wrap: the compare is on the signed difference
    CHECK(pick({job(0, &one, 0xffffffffu)}) == 0);
    CHECK(pick({job(0, &big, 1)}) == none);
    CHECK(lig::upload_ready(job(0, &one, 1)) && !lig::upload_ready(job(0, &one, 2)));
}

// ---- presence runs
static void check_runs(const std::vector<uint8_t>& mask, bool all_present_as_null = false) {
    const size_t row_bytes = 96, n = mask.size();
    std::vector<uint8_t> dst_buf(n * row_bytes + 1), src_buf(n * row_bytes + 1);
    uint8_t* dst = dst_buf.data();
    const uint8_t* src = src_buf.data();
    const std::vector<UploadSeg> segs = lig::presence_runs(all_present_as_null ? nullptr : mask.data(), n, row_bytes, dst, src);
    size_t row = 0, shipped = 0;                                            // rows tiled so far, present rows before `row`
    for (size_t i = 0; i < segs.size(); i++) {
        const UploadSeg& g = segs[i];
        CHECK(g.dst == dst + row * row_bytes);                              // in order, no gap, no overlap
        CHECK(g.bytes && g.bytes % row_bytes == 0);
        const size_t rows = g.bytes / row_bytes;
        CHECK(row + rows <= n);
        if (row + rows > n) return;
        for (size_t r = row; r < row + rows; r++) CHECK((mask[r] != 0) == (g.src != nullptr));      // a source exactly where the mask is set
        if (g.src) { CHECK(g.src == src + shipped * row_bytes); shipped += rows; }                     // consecutive over the present rows
        if (i) CHECK((segs[i - 1].src != nullptr) != (g.src != nullptr));                              // adjacent runs differ in kind
        row += rows;
    }
    CHECK(row == n);
    CHECK(shipped == (size_t)std::count_if(mask.begin(), mask.end(), [](uint8_t m) { return m != 0; }));
    CHECK(segs.empty() == (n == 0));
}
static void test_runs() {
    check_runs({});
    check_runs(std::vector<uint8_t>(7, 1));
    check_runs(std::vector<uint8_t>(7, 1), true);                           // no mask: every row is shipped
    check_runs(std::vector<uint8_t>(7, 0));
    check_runs({1});
    check_runs({0});
    check_runs({1, 0, 1, 0, 1, 0, 1});
    check_runs({0, 1, 0, 1, 0, 1});
    check_runs({2, 255, 0, 0, 1});                                          // any non-zero byte means present
    std::vector<uint8_t> head(40, 1), tail(40, 0);
    for (size_t i = 30; i < 40; i++) { head[i] = (uint8_t)(i & 1); tail[i - 30] = (uint8_t)(i & 1); }
    for (size_t i = 10; i < 40; i++) tail[i] = 1;
    check_runs(head);                                                       // a long run at either end
    check_runs(tail);
    std::mt19937 rng(20240607);
    for (int it = 0; it < 200; it++) {
        std::vector<uint8_t> m(1 + rng() % 64);
        const uint32_t density = rng() % 5;                                 // from mostly absent to mostly present
        for (uint8_t& v : m) v = (rng() % 4) < density;
        check_runs(m);
    }
}

// ---- chunk jobs
static void test_chunk_jobs() {
    uint8_t dev[64], host[64];
    uint32_t arrived[6] = {0}, consumed[6] = {0};
    std::atomic<int> failed{0}, abort{0};
    const std::vector<lig::UploadChunk> chunks = {{dev, host, 16}, {dev + 16, host + 16, 0}, {dev + 16, host + 16, 32}, {dev, host + 48, 8}, {dev + 8, host + 56, 0}};
    for (int with_consumed = 0; with_consumed < 2; with_consumed++) {
        const std::vector<UploadJob> jobs = with_consumed ? lig::chunk_jobs(chunks, arrived, 7, &failed, consumed, &abort, 1) : lig::chunk_jobs(chunks, arrived, 7, &failed);
        CHECK(jobs.size() == chunks.size());                                // one job per chunk, the empty ones too: their word is waited for
        for (size_t ci = 0; ci < jobs.size() && ci < chunks.size(); ci++) {
            const UploadJob& j = jobs[ci];
            CHECK(j.dst == chunks[ci].dst && j.src == chunks[ci].src && j.bytes == chunks[ci].bytes && !j.segs);
            CHECK(j.flag == arrived + ci && j.seq == 7 && j.failed == &failed);
            CHECK(j.prio == with_consumed && j.abort == (with_consumed ? &abort : nullptr));
            if (with_consumed && ci >= 2) CHECK(j.wait == consumed + ci - 2 && j.wait_val == 7);
            else CHECK(j.wait == nullptr);
        }
    }
    CHECK(lig::chunk_jobs({}, arrived, 1, &failed).empty());
}

// ---- flag pages.  chunk_schedule of prover_common.hpp, restated: `big` rows per chunk, a short first and / or last one
static size_t schedule_chunks(size_t R, size_t big, size_t head, size_t tail) {
    size_t n = 0, b = 0;
    if (head && R > head + tail) { n++; b = head; }
    const size_t stop = (tail && R > b + tail) ? R - tail : R;
    while (b < stop) { b = std::min(stop, b + big); n++; }
    return n + (b < R);
}
static void check_layout(const lig::FlagLayout& f, size_t n_rows, size_t n_rands) {
    const std::pair<size_t, size_t> regions[4] = {{f.rows, n_rows}, {f.rands, n_rands}, {f.consumed, n_rands}, {f.push, 1}};
    for (int a = 0; a < 4; a++) {
        CHECK(regions[a].first + regions[a].second <= f.words);             // inside the page
        for (int b = a + 1; b < 4; b++)                                     // pairwise disjoint (an empty region overlaps nothing)
            CHECK(!regions[a].second || !regions[b].second || regions[a].first + regions[a].second <= regions[b].first || regions[b].first + regions[b].second <= regions[a].first);
    }
}
static void test_flags() {
    CHECK(schedule_chunks(1307, 512, 128, 96) == 5 && schedule_chunks(1307, 512, 192, 0) == 4);      // the trace of tests/test_gpu_upload_modes.py
    const size_t CHUNK = 512, S2_HEAD = 192;
    const std::pair<size_t, size_t> traces[5] = {{0, 0}, {1, 1}, {5, 1307}, {3, 512}, {40, 20000}};  // (stage-1 chunks, rows)
    for (const auto& t : traces) {
        const size_t n_chunks = schedule_chunks(t.second, CHUNK, S2_HEAD, 0);
        const lig::FlagLayout f = lig::trace_flags(t.first, t.second, CHUNK, n_chunks);
        CHECK(f.rows == 0 && f.rands == t.first && f.consumed == t.first + n_chunks);
        CHECK(f.words == t.first + 2 * (t.second / CHUNK + 3) + 8 && f.push == f.words - 1);
        CHECK(f.consumed + n_chunks <= f.words);                            // the runtime check of stage 2 holds
        check_layout(f, t.first, n_chunks);
        CHECK(lig::trace_flags(t.first, t.second, CHUNK, 0).words == f.words);      // the page is sized before the stage-2 schedule is known
    }
    for (size_t rounds : {1, 2, 3, 17}) {
        const lig::FlagLayout f = lig::shard_flags(rounds);
        CHECK(f.rows == 0 && f.rands == rounds && f.consumed == 2 * rounds && f.words == 3 * rounds + 8);
        check_layout(f, rounds, rounds);
    }
}

int main() {
    test_pick();
    test_runs();
    test_chunk_jobs();
    test_flags();
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("upload plan ok\n");
    return 0;
}
