// upload.hip -- host rows -> device without a HIP stream of the prover in the path: the process-wide uploader thread.
//
// What was measured (tools/time_rows2.py, tools/h2d_under_load.py; profiles/r03_h2d_pipeline.md): the PCIe link delivers
// 57 GB/s to this process whatever the GPU is doing (550 MB = one 2^24-constraint trace in 9.7 ms, idle or under two proving
// contexts), and a foreign stream's upload does not slow the proofs down.  The prover's own chunked upload did: HIP maps the
// streams of a process onto GPU_MAX_HW_QUEUES = 4 hardware queues, every event recorded behind a copy (and every wait for one)
// is a barrier packet in such a queue, and while it waits for a 2 ms .. 10 ms transfer the kernels of whichever proof stream
// shares the queue do not start (stage 2 of a proof 4.9 -> 10-16 ms; two alternating contexts: 12.8 ms per proof, slower
// than one).  Priorities (own queue pool) and a shared copy stream move the problem around (A/B table in the profile).
// So: one uploader thread per device copies chunk after chunk on a stream of its own and waits for each copy ON THE HOST
// (no event, no packet behind the copy), then publishes the chunk's arrival in pinned host memory; the encode stream of the
// trace waits for that word with a stream memory operation (hipStreamWaitValue32 -- a wait in ITS OWN queue, where it has to
// wait anyway).  Uploads of all contexts go through the one thread: one at a time, in the order of the calls -- two contexts
// that alternate keep the link busy without ever sharing it.
#include "prover_common.hpp"
#include "upload.hpp"
#include <condition_variable>
#include <mutex>

hipError_t lig_internal_copy_job(const UploadJob& j, hipStream_t st) {
    if (!j.segs) return j.bytes ? hipMemcpyAsync(j.dst, j.src, j.bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    hipError_t e = hipSuccess;
    for (const UploadSeg& g : *j.segs) {
        if (!g.bytes || e != hipSuccess) continue;
        e = g.src ? hipMemcpyAsync(g.dst, g.src, g.bytes, hipMemcpyHostToDevice, st) : hipMemsetAsync(g.dst, 0, g.bytes, st);
    }
    return e;
}
int FlagPage::ensure(lig_ctx* c, size_t n_words) {
    if (host) return LIG_OK;
    const size_t bytes = (n_words * 4 + 4095) & ~(size_t)4095;
    HIP_TRY(c, hipHostMalloc((void**)&host, bytes, hipHostMallocDefault));
    std::memset((void*)host, 0, bytes);
    HIP_TRY(c, hipHostGetDevicePointer((void**)&dev, (void*)host, 0));
    words = n_words;
    return LIG_OK;
}

namespace {
struct Uploader {
    std::atomic<uint64_t> cur_bytes{0}, cur_since_us{0}, done_jobs{0};      // diagnostics
    std::atomic<int> phase{0};                                              // 0 idle, 1 copy call, 2 waiting for the copy, 3 publishing
    std::atomic<bool> broken{false};                                        // a transfer timed out: no further jobs
    bool fault_done = false;                                                // LIG_FAULT_UPLOAD: the injected fault has been spent
    std::atomic<uint32_t> abandoned{0};                                     // transfers given up on that may still be in flight on `st` (cleared by settle())
    std::atomic<uint32_t> retries{0};                                       // calls that re-made a timed-out upload with stream-ordered copies
    // The copy this thread stopped waiting for is still queued on `st` and cannot be cancelled.  settle(): has it finished by now?  (Bounded
    // poll from the calling thread; hipStreamQuery is thread-safe.)  Until it has, its source rows and its destination must stay alive.
    bool settle(double seconds) {
        if (!abandoned.load(std::memory_order_acquire)) return true;
        const auto t0 = clk::now();
        for (;;) {
            const hipError_t e = hipStreamQuery(st);
            if (e != hipErrorNotReady) { (void)hipGetLastError(); abandoned.store(0, std::memory_order_release); return true; }
            if (std::chrono::duration<double>(clk::now() - t0).count() > seconds) return false;
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
    }
    std::mutex mu;
    std::condition_variable cv;
    std::deque<QueuedUpload> q;
    std::thread th;
    hipStream_t st = nullptr;
    int device = 0;
    bool ok = false;
    void run() {
        if (hipSetDevice(device) != hipSuccess) return;
        for (;;) {
            QueuedUpload j;
            {
                std::unique_lock<std::mutex> lk(mu);
                for (;;) {
                    const size_t it = lig::upload_pick(q);
                    if (it != q.size()) { j = q[it]; q.erase(q.begin() + it); break; }
                    if (q.empty()) cv.wait(lk, [&] { return !q.empty(); });
                    else cv.wait_for(lk, std::chrono::microseconds(20));       // every queued job waits for the GPU: poll
                }
            }
            const bool dead = broken.load(std::memory_order_acquire);             // jobs queued behind a transfer that timed out fail at once
            const bool skip = dead || (j.job.abort && j.job.abort->load(std::memory_order_acquire));
            cur_bytes.store(j.job.bytes, std::memory_order_relaxed);
            cur_since_us.store((uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(clk::now().time_since_epoch()).count(), std::memory_order_relaxed);
            phase.store(1, std::memory_order_release);
            const hipError_t e = dead ? hipErrorLaunchTimeOut : skip ? hipSuccess : lig_internal_copy_job(j.job, st);
            phase.store(2, std::memory_order_release);
            // bounded: a transfer that does not complete (seen with several processes on one GPU, profiles/r05_rows_entry_hang.md) must
            // not hang every stream that waits for its word -- after LIG_UPLOAD_TIMEOUT_S the job is reported as failed (the word is
            // published; lig_rows_commit / _prove let their streams drain, wait -- bounded -- for the abandoned copy to leave the bus and
            // make the upload again with stream-ordered copies: rows_retry_*) and this thread takes no more jobs: callers fall back on
            // stream-ordered copies from then on (lig_internal_uploader_available turns false)
            hipError_t e2 = e;
            // tests (LIG_FAULT_UPLOAD): one transfer "never completes" -- 1: the first one of witness rows, 2: the first one of randomness rows
            const int fu = lig::knobs().fault_upload;
            const bool injected = fu && !skip && !fault_done && (fu == 2) == (j.job.prio == 1);
            if (injected) fault_done = true;
            if (e == hipSuccess) {
                const auto t_wait = clk::now();
                const double limit = (double)lig::knobs().upload_timeout_s;
                for (unsigned spins = 0;; spins++) {
                    e2 = injected ? hipErrorNotReady : hipStreamQuery(st);
                    if (e2 != hipErrorNotReady) break;
                    if (spins < 20000) std::this_thread::yield(); else std::this_thread::sleep_for(std::chrono::microseconds(20));
                    if ((spins & 1023) == 1023 && std::chrono::duration<double>(clk::now() - t_wait).count() > limit) { e2 = hipErrorLaunchTimeOut; abandoned.fetch_add(1, std::memory_order_acq_rel); broken.store(true, std::memory_order_release); break; }
                }
                if (e2 == hipErrorNotReady) e2 = hipSuccess;
            }
            phase.store(3, std::memory_order_release);
            // (a failed copy publishes too: no stream may hang on the flag; lig_rows_commit reports the error once stage 1 has drained)
            if (e2 != hipSuccess) { (void)hipGetLastError(); j.job.failed->store((int)e2, std::memory_order_release); }
            __atomic_store_n(j.job.flag, j.job.seq, __ATOMIC_RELEASE);
            j.pending->fetch_sub(1, std::memory_order_acq_rel);
            done_jobs.fetch_add(1, std::memory_order_relaxed);
            phase.store(0, std::memory_order_release);
        }
    }
};
Uploader* g_uploader[64] = {nullptr};
std::mutex g_uploader_mu;
Uploader* uploader_of(int device) { return device >= 0 && device < 64 ? g_uploader[device] : nullptr; }
}  // namespace
extern "C" bool lig_internal_uploader_available(lig_ctx* c) {
    if (c->device < 0 || c->device >= 64) return false;
    std::lock_guard<std::mutex> lk(g_uploader_mu);
    Uploader*& u = g_uploader[c->device];
    if (!u) {
        int can = 0;
        (void)hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, c->device);
        u = new Uploader();                         // lives for the process: its thread sleeps on the condition variable
        u->device = c->device;
        // The uploader's stream must not share a HARDWARE queue with a stream that may hold a pending hipStreamWaitValue32 for the word this
        // thread publishes: HIP maps the streams of a process onto GPU_MAX_HW_QUEUES (4) hardware queues per priority class, a pending stream
        // wait occupies its queue, and a small host-to-device copy is a blit KERNEL in the copying stream's queue (tools/queue_share_probe.hip,
        // profiles/r05_queue_share_probe.txt) -- behind the wait it would never run.  (A latent deadlock found while hunting the round-4 hang
        // of the sharded rows entry; not its cause, profiles/r05_rows_entry_hang.md.)  Queues are pooled per priority class, the library's
        // proof streams are normal priority: the uploader takes the highest.
        int lo = 0, hi = 0;
        const bool prio = lig::knobs().upload_prio && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo;
        u->ok = can && (prio ? hipStreamCreateWithPriority(&u->st, hipStreamNonBlocking, hi) : hipStreamCreateWithFlags(&u->st, hipStreamNonBlocking)) == hipSuccess;
        if (u->ok) { u->th = std::thread([u] { u->run(); }); u->th.detach(); }
    }
    return u->ok && !u->broken.load(std::memory_order_acquire);
}
std::string lig_internal_uploader_state(int device) {
    Uploader* u = uploader_of(device);
    if (!u) return "uploader: none";
    size_t queued = 0;
    { std::lock_guard<std::mutex> lk(u->mu); queued = u->q.size(); }
    const uint64_t now = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(clk::now().time_since_epoch()).count();
    const int ph = u->phase.load();
    static const char* names[4] = {"idle", "in the copy call", "waiting for the copy", "publishing"};
    return "uploader: " + std::string(names[ph & 3]) + (ph ? " (" + std::to_string(u->cur_bytes.load()) + " bytes, for " + std::to_string((now - u->cur_since_us.load()) / 1000) + " ms)" : "") +
           ", " + std::to_string(queued) + " queued, " + std::to_string(u->done_jobs.load()) + " done";
}
bool lig_internal_upload_settle(int device, double seconds) {
    Uploader* u = uploader_of(device);
    return !u || u->settle(seconds);
}
void lig_internal_upload_count_retry(int device) { g_uploader[device]->retries.fetch_add(1, std::memory_order_relaxed); }
extern "C" int lig_upload_health(lig_ctx* c, uint32_t* retries, uint32_t* unsettled) {
    CHECK_CTX(c);
    Uploader* u = uploader_of(c->device);
    if (u && u->abandoned.load(std::memory_order_acquire)) (void)u->settle(0.0);      // one query: has it finished in the meantime?
    if (retries) *retries = u ? u->retries.load(std::memory_order_relaxed) : 0;
    if (unsettled) *unsettled = u ? u->abandoned.load(std::memory_order_acquire) : 0;
    return LIG_OK;
}
extern "C" void lig_internal_uploader_submit(int device, const std::vector<UploadJob>& jobs, std::atomic<int>* pending) {
    Uploader* u = g_uploader[device];
    pending->fetch_add((int)jobs.size(), std::memory_order_acq_rel);
    {
        std::lock_guard<std::mutex> lk(u->mu);
        for (const UploadJob& j : jobs) u->q.push_back({j, pending});
    }
    u->cv.notify_one();
}
