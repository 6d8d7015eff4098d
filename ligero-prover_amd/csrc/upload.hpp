// upload.hpp -- the uploader thread's interface (upload.hip) and what a trace or a shard holds of its transfers: one pinned flag page,
// one lane per kind of rows.  The rules themselves (jobs, pick order, flag words) are in upload_plan.hpp, host only.
#pragma once
#include <thread>

#include "ctx_internal.hpp"
#include "upload_plan.hpp"

extern "C" bool lig_internal_uploader_available(lig_ctx* c);          // false: no stream memory operations on this device (callers fall back to stream copies)
extern "C" void lig_internal_uploader_submit(int device, const std::vector<UploadJob>& jobs, std::atomic<int>* pending);   // *pending += jobs, -1 per finished job
std::string lig_internal_uploader_state(int device);                  // diagnostics: queue length, the copy in progress and for how long
// A transfer the uploader thread gave up on is still queued on its stream and cannot be cancelled: bounded wait for it to leave the bus.
// true = it has (or there was none); false = still pending: what it reads and writes must stay alive (lig_upload_health reports it)
bool lig_internal_upload_settle(int device, double seconds);
void lig_internal_upload_count_retry(int device);                     // a call re-made a timed-out upload with stream-ordered copies
// the copies of a job, enqueued on `st`: a piece without a source is a zero fill; stops at the first error
hipError_t lig_internal_copy_job(const UploadJob& j, hipStream_t st);

// pinned, zeroed flag words (a whole number of 4 KiB pages) and their device alias; ensure() keeps a page it already has
struct FlagPage {
    volatile uint32_t* host = nullptr; uint32_t* dev = nullptr; size_t words = 0;
    int ensure(lig_ctx* c, size_t n_words);
    void release() { if (host) (void)hipHostFree((void*)host); host = nullptr; dev = nullptr; words = 0; }
};
// the transfers of one kind of rows of one object: seq = sequence number of the last upload (what its streams wait for), pending = jobs
// the uploader thread still has to make, failed = hipError_t of a copy that failed (the chunk is published all the same: no stream may hang)
struct UploadLane {
    uint32_t seq = 0;
    std::atomic<int> pending{0}, failed{0};
    // every copy has been made: the host rows and the device buffers are no longer touched by the thread
    void drain() const { while (pending.load(std::memory_order_acquire) > 0) std::this_thread::yield(); }
    int take_error() { return failed.exchange(0); }
};
