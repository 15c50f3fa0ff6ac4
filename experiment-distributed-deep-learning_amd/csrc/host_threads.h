// host_threads.h — host thread primitives of the keyed host-staging pipeline (host_stage.h): a
// memcpy pool, a one-worker job lane and the NUMA placement of their threads. No HIP runtime call
// in this unit, so tests/host_threads_check.cpp runs it under the host sanitizers without a GPU.
#pragma once

#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "common.h"

namespace ddl {

// The CPUs of the NUMA node the PCI function domain:bus:dev.0 hangs off, intersected with this
// thread's affinity; empty when unknown, or when binding would not narrow the set. The keyed host
// path's memcpy reads pinned host memory, which the HIP runtime places on the GPU's node: threads
// on the other socket pack the C5 set at half the rate (tools/numa_probe.py).
std::vector<int> numa_local_cpus(int domain, int bus, int dev);
void bind_this_thread(const std::vector<int> &cpus);  // empty: left where it is

// Parallel host memcpy for the host-staging pipeline (pageable <-> pinned): one memcpy thread
// moves ~10 GB/s, less than the PCIe link, so large chunks are split over a few workers.
class CopyPool {
public:
    struct Piece {
        void *dst;
        const void *src;
        size_t bytes;
    };
    // cpus non-empty: every worker binds itself to that CPU set (the GPU's NUMA node)
    explicit CopyPool(int threads, std::vector<int> cpus = {});
    ~CopyPool();
    CopyPool(const CopyPool &) = delete;
    CopyPool &operator=(const CopyPool &) = delete;
    // Copies every piece; returns when all are done (the caller's thread takes a share).
    void run(const std::vector<Piece> &pieces);
    // fn(lo, hi) over [0, n) cut into one range per thread (the caller's thread takes the first);
    // returns when every range is done
    void parallel(size_t n, const std::function<void(size_t, size_t)> &fn);
    int threads() const { return (int)threads_.size(); }

private:
    void worker_();
    void submit_and_wait_(std::vector<std::function<void()>> &tasks);  // tasks[0] on the caller
    std::vector<int> cpus_;
    std::vector<std::thread> threads_;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    std::vector<std::function<void()>> queue_;
    size_t outstanding_ = 0;
    bool stop_ = false;
};

// One worker thread running jobs in submission order: the host unpack of staged chunks, so the
// engine thread packs chunk i (CopyPool) while chunk i - kHostSlots is unpacked (its own CopyPool)
// — the two host memcpys overlap instead of alternating on the engine thread. wait(seq) blocks
// until job `seq` (1-based, from submit) has run; a job's Error is rethrown by the next wait.
class AsyncLane {
public:
    explicit AsyncLane(std::vector<int> cpus = {});
    ~AsyncLane();
    AsyncLane(const AsyncLane &) = delete;
    AsyncLane &operator=(const AsyncLane &) = delete;
    uint64_t submit(std::function<void()> job);
    void wait(uint64_t seq);
    void drain() noexcept;  // every job submitted so far has run (errors dropped)

private:
    void worker_();
    std::vector<int> cpus_;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    std::deque<std::function<void()>> q_;
    uint64_t submitted_ = 0, done_ = 0;
    bool stop_ = false;
    bool failed_ = false;
    Error err_{0, ""};
    std::thread thread_;
};

}  // namespace ddl
