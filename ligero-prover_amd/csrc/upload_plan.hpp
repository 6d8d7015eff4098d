// upload_plan.hpp -- the host-side rules of bringing caller rows from host memory, written once for the trace (prover.hip) and the shard
// (shard.hip): what an upload job is, which queued job the uploader thread takes next, how a presence mask becomes copies and zero
// fills, the jobs of a chunk schedule, where the words of a flag page lie.  Host only: nothing but the standard library, so that a plain
// host compiler builds it (tests/cpp/upload_plan_prog.cpp).  The thread, the copies and the pinned page itself are in upload.hip.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <memory>
#include <vector>

// ---- host rows -> device through the library's uploader thread (upload.hip; one thread per device, shared by every trace and
// shard): no copy, event or barrier packet of such a transfer sits in a HIP queue of a proof.  A job copies `bytes`, waits for
// the copy ON THE HOST, then publishes `seq` in *flag (pinned host memory; streams wait for it with hipStreamWaitValue32).
// `wait` (optional): the copy may only start once *wait >= wait_val -- a word in pinned host memory that a stream of the proof writes
// (hipStreamWriteValue32) when it is done with the destination buffer (the double-buffered randomness rows of stage 2)
// `segs` (optional, instead of dst / src / bytes): several pieces under one arrival word; a piece without a source is zero-filled on
// the device (rows a sparse randomness matrix does not ship)
struct UploadSeg { uint8_t* dst; const uint8_t* src; size_t bytes; };
struct UploadJob { uint8_t* dst; const uint8_t* src; size_t bytes; volatile uint32_t* flag; uint32_t seq; std::atomic<int>* failed;
                   const volatile uint32_t* wait = nullptr; uint32_t wait_val = 0; const std::atomic<int>* abort = nullptr;
                   int prio = 0;        // 1: a proof is waiting for it NOW (randomness rows) -- ahead of the prefetch of a next trace's witness rows
                   std::shared_ptr<std::vector<UploadSeg>> segs = nullptr; };
struct QueuedUpload { UploadJob job; std::atomic<int>* pending; };      // pending: -1 when the job is finished

namespace lig {
// the destination of a job is free (wrap-safe compare of the sequence numbers), or the job is to be dropped
inline bool upload_ready(const UploadJob& u) {
    return !u.wait || (int32_t)(__atomic_load_n(u.wait, __ATOMIC_ACQUIRE) - u.wait_val) >= 0 || (u.abort && u.abort->load(std::memory_order_acquire));
}
// The job the uploader thread takes next: the first whose destination is free -- a job that waits for its buffer must not hold up the
// other contexts' uploads queued behind it (jobs of one trace stay in order: their wait words become true in order).  q.size(): none.
inline size_t upload_pick(const std::deque<QueuedUpload>& q) {
    size_t it = q.size();
    for (size_t i = 0; i < q.size(); i++) {
        if (!upload_ready(q[i].job)) continue;
        if (it == q.size()) it = i;                                         // the oldest ready job ...
        if (q[i].job.prio > q[it].job.prio) { it = i; break; }              // ... unless a ready one is urgent
    }
    return it;
}
// n_rows rows at dst, row i shipped iff present[i] (null: all): runs of present rows are copied from where they follow each other in
// src, the others have no source (zero-filled on the device)
inline std::vector<UploadSeg> presence_runs(const uint8_t* present, uint64_t n_rows, size_t row_bytes, uint8_t* dst, const uint8_t* src) {
    std::vector<UploadSeg> segs;
    for (uint64_t i = 0; i < n_rows;) {
        uint64_t e = i + 1;
        const bool p = !present || present[i] != 0;
        while (e < n_rows && (!present || (present[e] != 0) == p)) e++;
        segs.push_back(UploadSeg{dst + i * row_bytes, p ? src : nullptr, (size_t)(e - i) * row_bytes});
        if (p) src += (e - i) * row_bytes;
        i = e;
    }
    return segs;
}
// One job per chunk of a schedule (a chunk of zero bytes too: its arrival word has to be published, streams wait for it): chunk ci
// publishes `seq` in arrived0[ci]; with consumed0, chunk ci >= 2 waits until the proof has written `seq` to consumed0[ci - 2] (its half
// of a double buffer is free again)
struct UploadChunk { uint8_t* dst; const uint8_t* src; size_t bytes; };
inline std::vector<UploadJob> chunk_jobs(const std::vector<UploadChunk>& chunks, volatile uint32_t* arrived0, uint32_t seq, std::atomic<int>* failed,
                                         const volatile uint32_t* consumed0 = nullptr, const std::atomic<int>* abort = nullptr, int prio = 0) {
    std::vector<UploadJob> jobs;
    for (size_t ci = 0; ci < chunks.size(); ci++) {
        UploadJob j{chunks[ci].dst, chunks[ci].src, chunks[ci].bytes, arrived0 + ci, seq, failed};
        if (consumed0 && ci >= 2) { j.wait = consumed0 + ci - 2; j.wait_val = seq; }
        j.abort = abort; j.prio = prio;
        jobs.push_back(j);
    }
    return jobs;
}
// word offsets in the pinned flag page: [rows: witness chunks arrived | rands: randomness chunks arrived | consumed], the last word
// (push) counts the rows of lig_rows_push_rands that have arrived
struct FlagLayout { size_t rows, rands, consumed, push, words; };
inline FlagLayout trace_flags(size_t s1_chunks, size_t R, size_t chunk, size_t n_chunks) {     // n_chunks: of the stage-2 schedule
    const size_t words = s1_chunks + 2 * (R / chunk + 3) + 8;
    return {0, s1_chunks, s1_chunks + n_chunks, words - 1, words};
}
inline FlagLayout shard_flags(size_t rounds) { return {0, rounds, 2 * rounds, 3 * rounds + 7, 3 * rounds + 8}; }
}  // namespace lig
