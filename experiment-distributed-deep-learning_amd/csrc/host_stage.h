// host_stage.h — the keyed handler's host path: the staging pipeline of host-resident requests
// (HostStager) and the opt-in hipHostRegister cache of their tensors (HostRegistrations). Only the
// handler's engine thread runs plans; user threads reach the cache through its two locked entries.
#pragma once

#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "host_threads.h"

namespace ddl {

// Waits for an event by polling, without holding a core for a whole long round (host_stage.cpp).
hipError_t wait_plan(hipEvent_t e);

// Opt-in registration cache (config "host_register_cache_bytes"): pageable host tensors of keyed
// requests are hipHostRegister'ed once and kept (least recently used out past the cap), so a
// training loop's CPU gradients take the pinned paths (direct DMA in, device unpack out).
class HostRegistrations {
public:
    // the streams whose work may DMA from / to a registered range (read when an entry goes)
    HostRegistrations(int device, const hipStream_t *h2d, const hipStream_t *d2h, const hipStream_t *compute)
        : device_(device), streams_{h2d, d2h, compute} {}
    ~HostRegistrations() { teardown(); }
    void teardown() noexcept;  // unregisters what is left; its owner has synced the streams
    // a host group holds this while its plans are posted: release_all (ddl_set_config on the
    // user's thread) then waits, and its stream sync covers every plan already posted with a
    // device alias of a registered range
    std::unique_lock<std::mutex> lock() { return std::unique_lock<std::mutex>(reg_mu_); }
    // lock() held. Registers the page ranges of (pointer, bytes) that are not pinned yet: ranges
    // sharing a page are merged (a page cannot be registered twice), overlapping entries join the union
    void ensure(const std::vector<std::pair<const void *, size_t>> &ranges);
    // Unregisters every range (ddl_set_config "host_register_cache_bytes" 0): waits for the streams first.
    void release_all();
    // The host range [ptr, ptr + bytes) is about to be freed (ddl_host_unregister): every cached
    // registration overlapping it goes — now if no host plan is being posted, otherwise before the
    // next lookup of the cache (the engine thread drains the queue first), so a later tensor at the
    // same address is never taken for the old, still-registered pages.
    void unregister_range(const void *ptr, size_t bytes);

private:
    // the one place an entry leaves: the streams synced (once per `synced`), unregistered, accounted
    void release_(uintptr_t a, bool &synced);
    void drop_overlapping_(uintptr_t lo, uintptr_t hi);  // reg_mu_ held
    void drain_unregisters_();  // reg_mu_ held: the queued unregister_range calls
    int device_;
    const hipStream_t *streams_[3];
    std::mutex unreg_mu_;
    std::vector<std::pair<uintptr_t, uintptr_t>> unreg_q_;
    std::mutex reg_mu_;  // reg_: the engine thread registers, ddl_set_config may release
    std::map<uintptr_t, std::pair<size_t, uint64_t>> reg_;  // page-aligned start -> (bytes, last use)
    size_t reg_bytes_ = 0;
    uint64_t reg_tick_ = 0;
};

struct HostSeg {
    const char *src;
    char *dst;
    size_t bytes;
    char *ddst = nullptr;  // the device's address of dst (device unpack; HostStager::mapped_dsts)
    int op = 0;            // ddl_allreduce_op of the request (allreduce plans)
};

// Everything the host path allocates: pinned and device slots, its two copy streams and their
// events, the copy threads and the unpack lane, the allgather staging buffer, the registrations.
class HostStager {
public:
    // `compute`: the handler's stream (the collectives); `copier`: its engine thread's SegmentCopier
    HostStager(int device, QueueClass qc, hipStream_t compute, SegmentCopier &copier)
        : device_(device), qc_(qc), stream_(compute), copier_(copier) {}
    ~HostStager();
    // Host-resident requests (the reference's deployment case, MPIRingTokenCommunication.cc:
    // 548-733 copies CPU tensors into its MPI buffer): the plan's segments are staged through
    // pinned slots in chunks — host pack (CopyPool) -> H2D -> `coll` on the device slot
    // (stream_) -> D2H -> host unpack — with kHostSlots chunks in flight so the copies overlap
    // the collective. `upload` false: nothing is packed (a broadcast's non-root ranks).
    // `padded`: segment i starts at the 256-byte-rounded running offset (the fusion kernels'
    // layout), so plans with and without `device_unpack` cut the same chunks — and issue the
    // same collectives — on ranks that differ in which outputs are pinned; otherwise back to
    // back (broadcast, as the reference packs).
    // `device_unpack` (every destination pinned and mapped on the device, mapped_dsts): the
    // unpack kernel writes each chunk's result straight into the outputs over PCIe (d2h_), in
    // place of the D2H copy and the host unpack; the host never waits for a chunk to come back
    // (measured 43 GB/s each way with the uploads running, vs 32 when the pack kernel also
    // reads the tensors over PCIe: profiles/r02/host/zero_copy_probe.jsonl).
    // AVG segments (HostSeg::op, with `dtype` and `divisor` = the communicator's size > 1): a
    // device-unpack plan's kernel stores their quotients into the pinned outputs; a staged plan
    // divides their slices of a chunk in place in the device slot (the same kernel, on stream_
    // after the chunk's collective) before the chunk's D2H copy. The chunk cuts do not change.
    void run(const std::vector<HostSeg> &segs, size_t es, bool upload,
             const std::function<void(void *dev, size_t elems)> &coll, bool padded = false,
             bool device_unpack = false, int dtype = 0, int divisor = 1);
    // true when every segment's destination range is 16-byte-aligned pinned host memory that the
    // device reaches at the same address, inside one allocation
    // fills every segment's ddst; false unless all of them are mapped
    // (the queries of a plan's 4096 tensors run on the copy threads: ~3 HIP calls each)
    bool mapped_dsts(std::vector<HostSeg> &segs);
    CopyPool &pool();          // the copy threads, rebuilt when host_copy_threads changed
    void bind_to_gpu_node();   // the calling thread and the copy threads started later (host_numa_bind)
    void *gather_buffer(size_t bytes);  // pinned host allgather staging of at least `bytes`
    HostRegistrations &registrations() { return regs_; }

private:
    void pieces_(const std::vector<HostSeg> &segs, const std::vector<size_t> &starts, size_t off, size_t len,
                 char *pinned, bool pack, std::vector<CopyPool::Piece> &out);
    size_t slots_(size_t total);  // chunk size for `total` bytes; (re)allocates the slots
    int device_;
    QueueClass qc_;
    hipStream_t stream_;
    SegmentCopier &copier_;
    std::vector<int> local_cpus_;  // the GPU's NUMA node's CPUs (empty: no binding)
    static constexpr int kHostSlots = 4;
    void *pin_[kHostSlots] = {};    // pinned host staging slots (uploads)
    void *pout_[kHostSlots] = {};   // pinned download slots: a chunk's D2H lands here, apart from the
                                    // upload slot, so its host unpack overlaps the next packs
    void *dslot_[kHostSlots] = {};  // device slots
    size_t host_slot_bytes_ = 0;
    hipStream_t h2d_ = nullptr, d2h_ = nullptr;
    hipEvent_t hev_[3 * kHostSlots] = {};  // per slot: input landed, collective done, output landed
    bool slot_used_[kHostSlots] = {};        // hev_[3k + 2] marks the slot's last device use
    std::unique_ptr<CopyPool> pool_;
    // the host unpack of staged chunks (its own copy threads, host_copy_threads of them); the lane
    // is destroyed first (its jobs use out_pool_)
    std::unique_ptr<CopyPool> out_pool_;
    std::unique_ptr<AsyncLane> lane_;
    void *pin_gather_ = nullptr;
    size_t pin_gather_bytes_ = 0;
    HostRegistrations regs_{device_, &h2d_, &d2h_, &stream_};
};

// Test hook (ddl_testing_host_coll_fault): the next host plan's staging loop fails at chunk
// `chunk` (-1: off) — its device collective is not posted — to check that no unpack job of the
// chunks before outlives the plan.
void set_testing_host_coll_fault(long long chunk);

}  // namespace ddl
