// host_stage.cpp — see host_stage.h.
#include "host_stage.h"

#include <atomic>
#include <chrono>
#include <thread>

#include "engine.h"

namespace ddl {

namespace {
std::atomic<long long> g_host_coll_fault{-1};

constexpr size_t round256(size_t b) { return (b + 255) & ~size_t(255); }

// Offsets of the segments in the staged stream: back to back, or 256-byte-rounded (padded).
size_t seg_starts(const std::vector<HostSeg> &segs, bool padded, std::vector<size_t> &starts) {
    starts.resize(segs.size());
    size_t total = 0;
    for (size_t i = 0; i < segs.size(); ++i) {
        starts[i] = total;
        total += padded ? round256(segs[i].bytes) : segs[i].bytes;
    }
    return total;
}

// Host range [p, p + bytes) is pinned (page-locked) host memory inside one allocation. With
// `alias` the range must also be mapped into the device's address space, 16-byte aligned (the
// unpack kernel's vector path; byte stores over PCIe would crawl): *alias = the device address of
// p — p itself for torch pin_memory / hipHostMalloc, the mapping's address for a hipHostRegister'ed
// range. A failed query (pageable memory) leaves no sticky error behind.
bool mapped_host_range(const void *p, size_t bytes, char **alias = nullptr) {
    if (bytes == 0) {
        if (alias) *alias = static_cast<char *>(const_cast<void *>(p));
        return true;
    }
    if (!p || (alias && (reinterpret_cast<uintptr_t>(p) & 15u) != 0)) return false;
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (a.type != hipMemoryTypeHost) return false;
    void *start = nullptr;
    size_t size = 0;
    if (hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, const_cast<void *>(p)) != hipSuccess ||
        hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, const_cast<void *>(p)) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(start), q = reinterpret_cast<uintptr_t>(p);
    if (!start || q < s0 || q + bytes > s0 + size) return false;
    if (alias) {
        if (!a.devicePointer || (reinterpret_cast<uintptr_t>(a.devicePointer) & 15u) != 0) return false;
        *alias = static_cast<char *>(a.devicePointer);
    }
    return true;
}
}  // namespace

void set_testing_host_coll_fault(long long chunk) { g_host_coll_fault = chunk; }

// Queries with yields for the first 200 us (a plan about to land — small rounds keep their
// latency), then sleeps between queries (each sleep ~20-70 us with the kernel's timer slack), so
// the completion thread does not spin beside the engine thread, the host copies and the
// framework's own threads. Also the unpack lane's wait for a D2H: hipEventSynchronize from a
// helper thread held up the engine thread's own HIP calls on the same streams (r04 s2: ~27 ms per
// pageable C5 batch outside every timed section of the staging loop; 3.9 ms once polled).
hipError_t wait_plan(hipEvent_t e) {
    using clk = std::chrono::steady_clock;
    const clk::time_point t0 = clk::now();
    for (;;) {
        const hipError_t q = hipEventQuery(e);
        if (q != hipErrorNotReady) return q;
        if (clk::now() - t0 < std::chrono::microseconds(200)) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

HostStager::~HostStager() {
    if (lane_) lane_->drain();  // unpack jobs read the pinned download slots freed below
    if (pin_gather_) (void)hipHostFree(pin_gather_);
    for (hipStream_t st : {h2d_, d2h_})
        if (st) (void)hipStreamSynchronize(st);
    for (int k = 0; k < kHostSlots; ++k) {
        if (pin_[k]) (void)hipHostFree(pin_[k]);
        if (pout_[k]) (void)hipHostFree(pout_[k]);
        if (dslot_[k]) (void)hipFree(dslot_[k]);
    }
    for (hipEvent_t e : hev_)
        if (e) (void)hipEventDestroy(e);
    regs_.teardown();
    for (hipStream_t st : {h2d_, d2h_})
        if (st) (void)hipStreamDestroy(st);
}

void HostStager::bind_to_gpu_node() {
    int dom = 0, bus = 0, dev = 0;
    if (hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, device_) != hipSuccess ||
        hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, device_) != hipSuccess ||
        hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, device_) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    local_cpus_ = numa_local_cpus(dom, bus, dev);
    bind_this_thread(local_cpus_);
}

void *HostStager::gather_buffer(size_t bytes) {
    if (pin_gather_bytes_ < bytes) {
        retire_host(pin_gather_);  // no hipHostFree on a data path (engine.h retire_host)
        pin_gather_ = nullptr;
        pin_gather_bytes_ = 0;
        DDL_HIP(hipHostMalloc(&pin_gather_, bytes + bytes / 2, hipHostMallocDefault));
        pin_gather_bytes_ = bytes + bytes / 2;
    }
    return pin_gather_;
}

void HostStager::pieces_(const std::vector<HostSeg> &segs, const std::vector<size_t> &starts, size_t off, size_t len,
                         char *pinned, bool pack, std::vector<CopyPool::Piece> &out) {
    // segment i holds [starts[i], starts[i] + bytes) of the staged stream (padding between
    // segments is neither packed nor unpacked)
    const size_t end = off + len;
    for (size_t i = (size_t)(std::upper_bound(starts.begin(), starts.end(), off) - starts.begin()) - 1;
         i < segs.size() && starts[i] < end; ++i) {
        const size_t lo = std::max(off, starts[i]), hi = std::min(end, starts[i] + segs[i].bytes);
        if (hi <= lo) continue;  // empty segment, or `off` past its data
        if (pack) out.push_back(CopyPool::Piece{pinned + (lo - off), segs[i].src + (lo - starts[i]), hi - lo});
        else out.push_back(CopyPool::Piece{segs[i].dst + (lo - starts[i]), pinned + (lo - off), hi - lo});
    }
}

bool HostStager::mapped_dsts(std::vector<HostSeg> &segs) {
    if (segs.empty()) return true;
    // the first query alone: a pageable output (the common staged case) answers in one call
    if (!mapped_host_range(segs[0].dst, segs[0].bytes, &segs[0].ddst)) return false;
    std::atomic<bool> all{true};
    pool().parallel(segs.size() - 1, [&](size_t lo, size_t hi) {
        for (size_t i = lo + 1; i < hi + 1 && all.load(std::memory_order_relaxed); ++i)
            if (!mapped_host_range(segs[i].dst, segs[i].bytes, &segs[i].ddst)) all = false;
    });
    return all.load();
}

size_t HostStager::slots_(size_t total) {
    size_t chunk = (size_t)config().host_chunk_bytes.load() & ~size_t(255);  // a multiple of es
    if (chunk < 4096) chunk = 4096;
    if (chunk > total) chunk = round256(total);
    if (host_slot_bytes_ < chunk) {
        for (hipStream_t st : {h2d_, d2h_, stream_})
            if (st) DDL_HIP(hipStreamSynchronize(st));
        for (int k = 0; k < kHostSlots; ++k) {  // outgrown slots kept until ddl_finalize (engine.h retire_*)
            retire_host(pin_[k]);
            retire_host(pout_[k]);
            retire_device(dslot_[k]);
            pin_[k] = pout_[k] = dslot_[k] = nullptr;
            slot_used_[k] = false;
        }
        host_slot_bytes_ = 0;
        for (int k = 0; k < kHostSlots; ++k) {
            DDL_HIP(hipHostMalloc(&pin_[k], chunk, hipHostMallocDefault));
            DDL_HIP(hipHostMalloc(&pout_[k], chunk, hipHostMallocDefault));
            DDL_HIP(hipMalloc(&dslot_[k], chunk));
        }
        host_slot_bytes_ = chunk;
    }
    if (!h2d_) {
        h2d_ = create_engine_stream(qc_);
        d2h_ = create_engine_stream(qc_);
        for (hipEvent_t &e : hev_) DDL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    return chunk;
}

CopyPool &HostStager::pool() {
    // rebuilt when the setting changed (only the engine thread runs host plans, so no plan is
    // using the old pool here); r02's thread-count sweep ran every setting on the first pool
    const int want = (int)std::max(0ll, config().host_copy_threads.load());
    if (!pool_ || pool_->threads() != want) {
        if (lane_) lane_->drain();  // no unpack job may still use out_pool_
        pool_.reset();
        pool_.reset(new CopyPool(want, local_cpus_));
        out_pool_.reset();
        out_pool_.reset(new CopyPool(want, local_cpus_));
    }
    if (!lane_) lane_.reset(new AsyncLane(local_cpus_));
    return *pool_;
}

void HostStager::run(const std::vector<HostSeg> &segs, size_t es, bool upload,
                     const std::function<void(void *, size_t)> &coll, bool padded, bool device_unpack, int dtype,
                     int divisor) {
    bool avg = false;
    if (divisor > 1)
        for (const HostSeg &sg : segs) avg = avg || (sg.op == DDL_ALLREDUCE_OP_AVG && sg.bytes);
    std::vector<size_t> starts;
    const size_t total = seg_starts(segs, padded || device_unpack, starts);
    if (total == 0) return;
    const size_t chunk = slots_(total);
    pool();
    if (device_unpack) config().host_zero_copy_plans.fetch_add(1);
    // chunk boundaries (the same on every rank)
    const std::vector<size_t> cut = host_chunk_cuts(total, chunk);
    const size_t nchunks = cut.size() - 1;
    std::vector<CopyPool::Piece> pieces;
    // timeline statistics (config "host_pack_us" / "host_wait_us" / "host_unpack_us"): where the
    // engine thread spends a host plan — packing chunks, waiting for a slot's DMA / device work,
    // unpacking chunks
    using clk = std::chrono::steady_clock;
    auto ns_since = [](clk::time_point t0) {  // summed in ns: a 4 KiB chunk's unpack is < 1 us
        return (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(clk::now() - t0).count();
    };
    // staged outputs: chunk j's D2H lands in the download slot pout_[j % kHostSlots] and its host
    // unpack runs on the unpack lane (out_pool_'s copy threads) — concurrently with the engine
    // thread's packs of the next chunks into the upload slots. Before the D2H of chunk j + kHostSlots
    // reuses the download slot, the engine thread waits for chunk j's unpack (host_unpack_us).
    std::vector<uint64_t> unpacked(nchunks, 0);  // lane job of chunk j
    const int dev = device_;
    auto unpack_async = [&](size_t j) {
        const int k = (int)(j % kHostSlots);
        std::vector<CopyPool::Piece> pc;
        pieces_(segs, starts, cut[j], cut[j + 1] - cut[j], static_cast<char *>(pout_[k]), false, pc);
        const hipEvent_t landed = hev_[3 * k + 2];  // re-recorded only after this job (wait_unpack)
        CopyPool *op = out_pool_.get();
        unpacked[j] = lane_->submit([dev, landed, op, ns_since, pc = std::move(pc)] {
            DeviceGuard g(dev);
            // D2H of chunk j landed (polled: see wait_plan). The lane's two phases are timed apart
            // (config "host_lane_d2h_wait_us" / "host_lane_copy_us" / "host_lane_copy_bytes",
            // VERDICT r5 next #4): the wait says how long the DMA kept the lane, the copy what
            // rate the pinned download slot -> pageable output memcpy reaches
            clk::time_point t0 = clk::now();
            const hipError_t q = wait_plan(landed);
            config().host_lane_d2h_wait_ns.fetch_add(ns_since(t0));
            DDL_REQUIRE(q == hipSuccess, DDL_STATUS_HIP_ERROR, "D2H of a staged chunk: " << hipGetErrorString(q));
            t0 = clk::now();
            op->run(pc);
            config().host_lane_copy_ns.fetch_add(ns_since(t0));
            long long bytes = 0;
            for (const CopyPool::Piece &p : pc) bytes += (long long)p.bytes;
            config().host_lane_copy_bytes.fetch_add(bytes);
            config().host_lane_jobs.fetch_add(1);
        });
    };
    auto wait_unpack = [&](size_t j) {
        const clk::time_point t0 = clk::now();
        lane_->wait(unpacked[j]);
        config().host_unpack_ns.fetch_add(ns_since(t0));
    };
    std::vector<CopySeg> dst;  // the pieces handed to the copier
    // no unpack job may outlive the plan: if posting throws midway (a collective, a
    // HIP call, a failed unpack), the lane finishes the jobs already submitted — they write into
    // the requests' outputs — before the error reaches complete_() and done(), after which the
    // caller may free those outputs; drain() also clears the lane's error, so it cannot surface in
    // a later plan's wait
    try {
        for (size_t i = 0; i < nchunks; ++i) {
            const int k = (int)(i % kHostSlots);
            const size_t off = cut[i], n = cut[i + 1] - off;
            // the device slot's last user may still be in flight (a device unpack)
            if (slot_used_[k]) DDL_HIP(hipStreamWaitEvent(h2d_, hev_[3 * k + 2], 0));
            if (upload) {
                // the pinned slot's last upload must have left it (device-unpack plans do not wait
                // for their D2H on the host)
                clk::time_point t0 = clk::now();
                if (slot_used_[k]) DDL_HIP(hipEventSynchronize(hev_[3 * k]));
                config().host_wait_ns.fetch_add(ns_since(t0));
                t0 = clk::now();
                pieces.clear();
                pieces_(segs, starts, off, n, static_cast<char *>(pin_[k]), true, pieces);
                pool_->run(pieces);  // packs chunk i while the device works on chunks i-1, i-2, ...
                DDL_HIP(hipMemcpyAsync(dslot_[k], pin_[k], n, hipMemcpyHostToDevice, h2d_));
                config().host_pack_ns.fetch_add(ns_since(t0));
            }
            DDL_HIP(hipEventRecord(hev_[3 * k], h2d_));
            DDL_HIP(hipStreamWaitEvent(stream_, hev_[3 * k], 0));
            const clk::time_point t_coll = clk::now();
            const long long fault = g_host_coll_fault.load();
            if (fault >= 0 && (long long)i >= fault) {  // test hook (ddl_testing_host_coll_fault)
                g_host_coll_fault = -1;
                fail(DDL_STATUS_COMM_ERROR, "test fault: host plan collective of chunk " + std::to_string(i));
            }
            coll(dslot_[k], n / es);
            if (avg && !device_unpack) {
                // staged outputs: the AVG slices of this chunk become their quotients in the slot
                dst.clear();
                for (size_t j = (size_t)(std::upper_bound(starts.begin(), starts.end(), off) - starts.begin()) - 1;
                     j < segs.size() && starts[j] < off + n; ++j) {
                    const size_t lo = std::max(off, starts[j]), hi = std::min(off + n, starts[j] + segs[j].bytes);
                    if (hi <= lo || segs[j].op != DDL_ALLREDUCE_OP_AVG) continue;
                    dst.push_back(CopySeg{static_cast<char *>(dslot_[k]) + (lo - off), hi - lo, DDL_ALLREDUCE_OP_AVG});
                }
                copier_.run(CopyLaunch{SegmentCopier::kDivInPlace, nullptr, stream_, dtype, 0, divisor}, dst.data(),
                            (int)dst.size());
            }
            config().host_coll_ns.fetch_add(ns_since(t_coll));
            DDL_HIP(hipEventRecord(hev_[3 * k + 1], stream_));
            DDL_HIP(hipStreamWaitEvent(d2h_, hev_[3 * k + 1], 0));
            if (device_unpack) {
                // the unpack kernel writes the chunk's pieces straight into the pinned outputs over
                // PCIe; it lays piece j at the rounded sum of the pieces before it, which is its
                // offset in the padded stream (chunks start at multiples of 256, so a cut never
                // falls inside a segment's padding)
                dst.clear();
                size_t flat = 0;
                for (size_t j = (size_t)(std::upper_bound(starts.begin(), starts.end(), off) - starts.begin()) - 1;
                     j < segs.size() && starts[j] < off + n; ++j) {
                    const size_t lo = std::max(off, starts[j]), hi = std::min(off + n, starts[j] + segs[j].bytes);
                    if (hi <= lo) continue;
                    DDL_REQUIRE(flat == lo - off, DDL_STATUS_ERROR_UNKNOWN, "device-unpack chunk layout");
                    dst.push_back(CopySeg{segs[j].ddst + (lo - starts[j]), hi - lo, segs[j].op});  // the device's address of the output
                    flat += round256(hi - lo);
                }
                copier_.run(CopyLaunch{1, dslot_[k], d2h_, dtype, 0, divisor}, dst.data(), (int)dst.size());
            } else {
                if (i >= (size_t)kHostSlots) wait_unpack(i - kHostSlots);  // download slot k free again
                const clk::time_point t_post = clk::now();
                DDL_HIP(hipMemcpyAsync(pout_[k], dslot_[k], n, hipMemcpyDeviceToHost, d2h_));
                config().host_d2h_post_ns.fetch_add(ns_since(t_post));
            }
            DDL_HIP(hipEventRecord(hev_[3 * k + 2], d2h_));
            slot_used_[k] = true;
            if (!device_unpack) {
                const clk::time_point t_sub = clk::now();
                unpack_async(i);
                config().host_unpack_submit_ns.fetch_add(ns_since(t_sub));
            }
        }
        if (device_unpack) {
            // the plan's event (recorded on stream_ next) covers the last unpack, hence every unpack
            DDL_HIP(hipStreamWaitEvent(stream_, hev_[3 * ((nchunks - 1) % kHostSlots) + 2], 0));
            return;
        }
        for (size_t j = nchunks > (size_t)kHostSlots ? nchunks - kHostSlots : 0; j < nchunks; ++j) wait_unpack(j);
    } catch (...) {
        lane_->drain();
        // device-unpack plans: copier kernels of the chunks already posted on d2h_ write into the
        // caller's pinned outputs; they must finish before done(error) lets the caller free those
        // (ADVICE r5). The H2D / compute work of posted chunks reads the caller's inputs and the
        // slots: drained too, so the next plan starts from idle streams.
        (void)hipStreamSynchronize(h2d_);
        (void)hipStreamSynchronize(stream_);
        (void)hipStreamSynchronize(d2h_);
        throw;
    }
}

void HostRegistrations::teardown() noexcept {
    for (auto &e : reg_) (void)hipHostUnregister(reinterpret_cast<void *>(e.first));
    reg_.clear();
}

void HostRegistrations::release_all() {
    std::lock_guard<std::mutex> g(reg_mu_);
    DeviceGuard dg(device_);
    {
        std::lock_guard<std::mutex> q(unreg_mu_);
        unreg_q_.clear();  // everything goes anyway
    }
    bool synced = false;
    while (!reg_.empty()) release_(reg_.begin()->first, synced);
}

void HostRegistrations::unregister_range(const void *ptr, size_t bytes) {
    if (!ptr || !bytes) return;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(ptr), hi = lo + bytes;
    std::unique_lock<std::mutex> g(reg_mu_, std::try_to_lock);
    if (!g.owns_lock()) {  // a host plan is being posted: the engine drains the queue before its next lookup
        std::lock_guard<std::mutex> q(unreg_mu_);
        unreg_q_.emplace_back(lo, hi);
        return;
    }
    DeviceGuard dg(device_);
    drain_unregisters_();
    drop_overlapping_(lo, hi);
}

void HostRegistrations::drain_unregisters_() {
    std::vector<std::pair<uintptr_t, uintptr_t>> q;
    {
        std::lock_guard<std::mutex> g(unreg_mu_);
        q.swap(unreg_q_);
    }
    for (const auto &r : q) drop_overlapping_(r.first, r.second);
}

void HostRegistrations::release_(uintptr_t a, bool &synced) {
    if (!synced) {  // plans in flight may still DMA from / to it
        for (const hipStream_t *st : streams_)
            if (*st) DDL_HIP(hipStreamSynchronize(*st));
        synced = true;
    }
    (void)hipHostUnregister(reinterpret_cast<void *>(a));
    (void)hipGetLastError();
    reg_bytes_ -= reg_[a].first;
    config().host_registered_bytes.fetch_sub((long long)reg_[a].first);
    reg_.erase(a);
}

void HostRegistrations::drop_overlapping_(uintptr_t lo, uintptr_t hi) {
    std::vector<uintptr_t> drop;
    for (auto &e : reg_)
        if (e.first < hi && lo < e.first + e.second.first) drop.push_back(e.first);
    bool synced = false;
    for (uintptr_t a : drop) {
        release_(a, synced);
        config().host_unregistered_ranges.fetch_add(1);
    }
}

void HostRegistrations::ensure(const std::vector<std::pair<const void *, size_t>> &ranges) {
    constexpr uintptr_t kPage = 4096;
    drain_unregisters_();  // ranges freed since the last lookup are not hits
    const size_t cap = (size_t)config().host_register_cache_bytes.load();
    // 1) the page ranges of the tensors not pinned already, merged where they share pages (small
    //    tensors of one heap page; hipHostRegister refuses a page registered twice)
    std::vector<std::pair<uintptr_t, uintptr_t>> want;
    for (const auto &r : ranges) {
        if (!r.first || r.second == 0) continue;
        const uintptr_t lo = reinterpret_cast<uintptr_t>(r.first) & ~(kPage - 1);
        const uintptr_t hi = (reinterpret_cast<uintptr_t>(r.first) + r.second + kPage - 1) & ~(kPage - 1);
        auto it = reg_.upper_bound(lo);  // inside an entry already: touch it
        if (it != reg_.begin() && std::prev(it)->first <= lo && hi <= std::prev(it)->first + std::prev(it)->second.first) {
            std::prev(it)->second.second = ++reg_tick_;
            config().host_register_hits.fetch_add(1);
            continue;
        }
        if (mapped_host_range(r.first, r.second)) continue;  // pinned already (the framework's own)
        want.emplace_back(lo, hi);
    }
    std::sort(want.begin(), want.end());
    std::vector<std::pair<uintptr_t, uintptr_t>> merged;
    for (const auto &w : want) {
        if (!merged.empty() && w.first < merged.back().second) merged.back().second = std::max(merged.back().second, w.second);
        else merged.push_back(w);
    }
    bool synced = false;
    for (auto m : merged) {
        // 2) entries overlapping it (a tensor that grew, moved or shares a page) join the union
        std::vector<uintptr_t> drop;
        for (auto &e : reg_)
            if (e.first < m.second && m.first < e.first + e.second.first) {
                drop.push_back(e.first);
                m.first = std::min(m.first, e.first);
                m.second = std::max(m.second, (uintptr_t)(e.first + e.second.first));
            }
        const size_t bytes = m.second - m.first;
        if (bytes > cap) continue;
        for (uintptr_t a : drop) release_(a, synced);
        while (reg_bytes_ + bytes > cap && !reg_.empty()) {  // least recently used out
            auto lru = reg_.begin();
            for (auto e = reg_.begin(); e != reg_.end(); ++e)
                if (e->second.second < lru->second.second) lru = e;
            release_(lru->first, synced);
        }
        if (hipHostRegister(reinterpret_cast<void *>(m.first), bytes, hipHostRegisterMapped) != hipSuccess) {
            (void)hipGetLastError();  // e.g. registered by someone else: staged as before
            config().host_register_failures.fetch_add(1);
            continue;
        }
        reg_[m.first] = std::make_pair(bytes, ++reg_tick_);
        reg_bytes_ += bytes;
        config().host_registered_bytes.fetch_add((long long)bytes);
    }
}

}  // namespace ddl
