// engine.cpp — communicators, registry, config, logging, errors.
#include "engine.h"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>

#include "handler.h"

namespace ddl {

// ---- errors / logging --------------------------------------------------------------------
namespace {
thread_local std::string t_last_error;
}

void set_error(const std::string &msg) { t_last_error = msg; }
const char *last_error() { return t_last_error.c_str(); }

Config &config() {
    static Config *c = [] {
        Config *cfg = new Config();
        if (const char *e = std::getenv("DDL_ALGO")) cfg->algo = std::atoll(e);
        if (const char *e = std::getenv("DDL_SLICE_BYTES")) cfg->slice_bytes = std::atoll(e);
        if (const char *e = std::getenv("DDL_RINGS")) cfg->rings = std::atoll(e);
        if (const char *e = std::getenv("DDL_MAX_SLICES")) cfg->max_slices = std::atoll(e);
        if (const char *e = std::getenv("DDL_FUSION_THRESHOLD")) cfg->fusion_threshold_bytes = std::atoll(e);
        // RCCL channel bounds for a deployment that sets them per job (0..256, as ddl_set_config)
        if (const char *e = std::getenv("DDL_RCCL_MIN_CTAS")) cfg->rccl_min_ctas = std::max(0ll, std::min(256ll, std::atoll(e)));
        if (const char *e = std::getenv("DDL_RCCL_MAX_CTAS")) cfg->rccl_max_ctas = std::max(0ll, std::min(256ll, std::atoll(e)));
        if (const char *e = std::getenv("DDL_QUEUE_ISOLATION")) cfg->queue_isolation = std::atoll(e) ? 1 : 0;
        if (const char *e = std::getenv("DDL_LOG_LEVEL")) cfg->log_level = std::atoll(e);
        if (const char *e = std::getenv("DDL_CYCLE_TIME_US")) cfg->cycle_time_us = std::atoll(e);
        if (const char *e = std::getenv("DDL_TUNE")) cfg->tune = std::atoll(e);
        return cfg;
    }();
    return *c;
}

uint64_t Config::shared_hash() const {
    const long long v[] = {algo.load(), slice_bytes.load(), rings.load(), max_slices.load(),
                           fusion_threshold_bytes.load(), tune.load(), fusion_pipeline_bytes.load(),
                           reference_order.load(), host_chunk_bytes.load(), rccl_min_ctas.load(),
                           rccl_max_ctas.load()};
    uint64_t h = 1469598103934665603ull;  // FNV-1a over the values' bytes
    for (long long x : v)
        for (int b = 0; b < 8; ++b) {
            h ^= (uint64_t)((unsigned long long)x >> (8 * b)) & 0xff;
            h *= 1099511628211ull;
        }
    h |= 1;  // never 0 ("no agreement yet")
    return h == kCfgMismatch ? h - 2 : h;
}

int log_level() { return (int)config().log_level.load(); }
int config_capture_mode() { return (int)config().capture_mode.load(); }
int config_compute_cu_mask() { return (int)config().compute_cu_mask.load(); }

void log_line(int level, const std::string &msg) {
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    const char *tag = level <= 0 ? "ERROR" : (level == 1 ? "INFO" : "DEBUG");
    std::fprintf(stderr, "[ddl %s tid=%zu] %s\n", tag,
                 (size_t)std::hash<std::thread::id>()(std::this_thread::get_id()) % 100000, msg.c_str());
}

// ---- device guard ---------------------------------------------------------------------------
DeviceGuard::DeviceGuard(int device) {
    if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
    if (prev_ != device) DDL_HIP(hipSetDevice(device));
}
DeviceGuard::~DeviceGuard() {
    int cur = -1;
    if (prev_ >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev_) (void)hipSetDevice(prev_);
}

// ---- communicator -----------------------------------------------------------------------------
Communicator::Communicator(int rank, int size, int device, ncclComm_t nccl, std::shared_ptr<TestHooks> hooks,
                           long long tag, std::vector<int> world_ranks, QueueClass qc)
    : rank_(rank), size_(size), device_(device), nccl_(nccl), hooks_(std::move(hooks)), tag_(tag),
      world_ranks_(std::move(world_ranks)),
      qclass_(nccl && size > 1 && config().queue_isolation.load() ? qc : QueueClass::kPooled) {
    // the world (created kPooled) keeps its keyed path apart, at the greatest priority
    keyed_qclass_ = qclass_ == QueueClass::kPooled && nccl_ && size_ > 1 && config().queue_isolation.load()
                        ? QueueClass::kHigh
                        : qclass_;
    DeviceGuard g(device_);
    std::unique_ptr<Transport> t;
    if (size_ > 1) {
        if (hooks_) {
            DDL_REQUIRE(hooks_->make_transport, DDL_STATUS_INVALID_ARGUMENT, "test hooks without a transport");
            t = hooks_->make_transport(hooks_, tag_, world_ranks_, rank_, size_);
            cb_ = t.get();
        } else {
            t.reset(new RcclTransport(nccl_));
        }
    }
    exec_.reset(new RingExecutor(rank_, size_, device_, std::move(t), qclass_));
}

Communicator::~Communicator() {
    handler_.reset();  // stops the handler thread (its SHUT_DOWN lap uses control_)
    keyed_data_.reset();
    control_.reset();
    exec_.reset();
    for (void *s : slots_)
        if (s) (void)hipFree(s);
    if (tune_a_) (void)hipFree(tune_a_);
    if (tune_b_) (void)hipFree(tune_b_);
    for (hipStream_t s : {h2d_, ring_, d2h_, ctl_stream_})
        if (s) (void)hipStreamDestroy(s);
    if (nccl_) (void)rccl().CommDestroy(nccl_);
}

// One user collective on a communicator with a token ring: waits while a keyed round is being
// placed at or before this collective's number (round_freeze / round_release), then counts itself
// as entered; on leaving (enqueued, or failed on every rank alike) as done. The gate's mutex is
// held only for those two steps: a collective that synchronises with the other ranks (tuning,
// the config agreement, the test transport) never blocks the handler's placement of a round —
// which counts it already (entered), so every rank runs it before the round.
class Communicator::UserCollective {
public:
    explicit UserCollective(Communicator &c) : c_(c) {
        if (c_.size_ <= 1 || !c_.keyed_data_) return;
        std::unique_lock<std::mutex> lk(c_.gate_mu_);
        c_.gate_cv_.wait(lk, [&] { return c_.aborted_ || !c_.frozen_ || c_.user_seq_ < c_.release_; });
        DDL_REQUIRE(!c_.aborted_, c_.aborted_,
                    "the communicator's keyed request handler stopped (" << c_.abort_msg_
                                                                         << "): user collectives can no longer be "
                                                                            "ordered against keyed rounds");
        ++c_.user_seq_;
        active_ = true;
    }
    ~UserCollective() {
        if (!active_) return;
        {
            std::lock_guard<std::mutex> g(c_.gate_mu_);
            ++c_.user_done_;
        }
        c_.gate_cv_.notify_all();
    }

private:
    Communicator &c_;
    bool active_ = false;
};

long long Communicator::round_freeze() {
    std::lock_guard<std::mutex> g(gate_mu_);
    frozen_ = true;
    release_ = user_seq_;
    return user_seq_;
}

void Communicator::round_release(long long at) {
    {
        std::lock_guard<std::mutex> g(gate_mu_);
        DDL_REQUIRE(at >= user_seq_, DDL_STATUS_COMM_ERROR,
                    "keyed round placed after user collective " << at << " but " << user_seq_ << " have started");
        release_ = at;
        round_log_.push_back(at);
        if (round_log_.size() > 4096) round_log_.erase(round_log_.begin(), round_log_.begin() + 2048);
    }
    gate_cv_.notify_all();
}

void Communicator::round_enter(long long at) {
    std::unique_lock<std::mutex> g(gate_mu_);
    gate_cv_.wait(g, [&] { return aborted_ || user_done_ >= at; });
    DDL_REQUIRE(!aborted_, aborted_, "keyed round not entered: " << abort_msg_);
    DDL_REQUIRE(user_seq_ == at && user_done_ == at, DDL_STATUS_COMM_ERROR,
                "keyed round placed after user collective " << at << " but " << user_seq_ << " have started");
}

void Communicator::round_unfreeze() {
    {
        std::lock_guard<std::mutex> g(gate_mu_);
        frozen_ = false;
    }
    gate_cv_.notify_all();
}

void Communicator::round_abort(int status, const std::string &why) {
    {
        std::lock_guard<std::mutex> g(gate_mu_);
        if (!aborted_) {
            aborted_ = status ? status : DDL_STATUS_COMM_ERROR;
            abort_msg_ = why;
        }
        frozen_ = false;
    }
    gate_cv_.notify_all();
}

long long Communicator::user_collectives() const {
    std::lock_guard<std::mutex> g(const_cast<std::mutex &>(gate_mu_));
    return user_seq_;
}

std::vector<long long> Communicator::round_log() const {
    std::lock_guard<std::mutex> g(const_cast<std::mutex &>(gate_mu_));
    return round_log_;
}

void Communicator::transport(int *kind, int *ranks) const {
    *kind = size_ <= 1 ? 0 : (hooks_ ? 2 : 1);
    *ranks = size_;
    if (*kind == 1) rccl_check(rccl().CommCount(nccl_, ranks), "ncclCommCount");
}

void check_config_agreement(int rank, const std::vector<uint64_t> &hashes) {
    bool same = true;
    for (uint64_t h : hashes) same = same && h == hashes[0];
    if (same) return;
    std::ostringstream os;
    os << "shared tunables differ between ranks (algo, slice_bytes, rings, max_slices, fusion_threshold_bytes, "
          "tune, fusion_pipeline_bytes, reference_order, host_chunk_bytes, rccl_min_ctas, rccl_max_ctas must be "
          "set alike on every rank); "
          "config hash per rank:";
    for (size_t q = 0; q < hashes.size(); ++q)
        os << " " << q << (q == (size_t)rank ? "*" : "") << "=" << std::hex << hashes[q] << std::dec;
    fail(DDL_STATUS_CONFIG_MISMATCH, os.str());
}

void Communicator::agree_config(hipStream_t stream) {
    if (size_ <= 1) return;
    const uint64_t mine = config().shared_hash();
    if (mine == agreed_hash_) return;
    DDL_REQUIRE(!stream_capturing(stream), DDL_STATUS_INVALID_ARGUMENT,
                "the shared tunables changed (or this is the communicator's first collective): the ranks must "
                "agree on them outside a graph capture — run one collective before capturing");
    std::vector<uint64_t> all(size_, 0);
    all[rank_] = mine;
    if (hooks_) {
        std::vector<ddl_p2p_op> ops;
        for (int d = 1; d < size_; ++d) {
            const int to = (rank_ + d) % size_, from = (rank_ + size_ - d) % size_;
            ops.push_back(ddl_p2p_op{1, to, 4002, &all[rank_], sizeof(uint64_t)});
            ops.push_back(ddl_p2p_op{0, from, 4002, &all[from], sizeof(uint64_t)});
        }
        cb_->host_group(ops);
    } else {
        if (!ctl_stream_) ctl_stream_ = create_engine_stream(qclass_);
        rccl_allgather_u64(nccl_, all.data(), size_, rank_, ctl_stream_);
    }
    check_config_agreement(rank_, all);
    agreed_hash_ = mine;
}

void Communicator::allreduce(const void *send, void *recv, size_t n, int dtype, int op, hipStream_t stream,
                             size_t order_bytes) {
    check_allreduce_op(op, dtype);
    DDL_REQUIRE(dtype_size(dtype) != 0, DDL_STATUS_UNSUPPORTED_DTYPE, "unsupported dtype " << dtype);
    DDL_REQUIRE(n == 0 || (send && recv), DDL_STATUS_INVALID_ARGUMENT, "null buffer");
    UserCollective uc(*this);
    std::lock_guard<std::mutex> g(mu_);
    DeviceGuard dg(device_);
    RingConfig cfg = ring_config(n, dtype, stream);
    cfg.order_bytes = order_bytes;
    exec_->allreduce(send, recv, n, dtype, stream, cfg, op);
}

void Communicator::allreduce_batch(const void *const *send, void *const *recv, const size_t *n, int count, int dtype,
                                   int op, hipStream_t stream) {
    check_allreduce_op(op, dtype);
    DDL_REQUIRE(dtype_size(dtype) != 0, DDL_STATUS_UNSUPPORTED_DTYPE, "unsupported dtype " << dtype);
    DDL_REQUIRE(count >= 0 && (count == 0 || (send && recv && n)), DDL_STATUS_INVALID_ARGUMENT, "null bucket arrays");
    size_t largest = 0;
    for (int b = 0; b < count; ++b) {
        DDL_REQUIRE(n[b] == 0 || (send[b] && recv[b]), DDL_STATUS_INVALID_ARGUMENT, "null buffer in bucket " << b);
        largest = std::max(largest, n[b]);
    }
    UserCollective uc(*this);
    std::lock_guard<std::mutex> g(mu_);
    DeviceGuard dg(device_);
    const RingConfig cfg = ring_config(largest, dtype, stream);
    exec_->allreduce_batch(send, recv, n, count, dtype, stream, cfg, op);
}

void Communicator::rccl_allreduce(const void *send, void *recv, size_t n, int dtype, hipStream_t stream) {
    UserCollective uc(*this);
    std::lock_guard<std::mutex> g(mu_);
    DeviceGuard dg(device_);
    if (size_ == 1) {
        if (send != recv && n) DDL_HIP(hipMemcpyAsync(recv, send, n * dtype_size(dtype), hipMemcpyDeviceToDevice, stream));
        return;
    }
    DDL_REQUIRE(nccl_ != nullptr, DDL_STATUS_INVALID_ARGUMENT, "no RCCL communicator (test transport)");
    ncclDataType_t t;
    switch (dtype) {
        case DDL_FLOAT: t = ncclFloat32; break;
        case DDL_DOUBLE: t = ncclFloat64; break;
        case DDL_INT32: t = ncclInt32; break;
        case DDL_INT64: t = ncclInt64; break;
        case DDL_UINT64: t = ncclUint64; break;
        case DDL_HALF: t = ncclFloat16; break;
        case DDL_BFLOAT16: t = ncclBfloat16; break;
        default: fail(DDL_STATUS_UNSUPPORTED_DTYPE, "unsupported dtype");
    }
    agree_config(stream);
    rccl_check(rccl().AllReduce(send, recv, n, t, ncclSum, nccl_, stream), "ncclAllReduce");
}

namespace {

}  // namespace

int size_class(size_t bytes) { return bytes ? 63 - __builtin_clzll((unsigned long long)bytes) : -1; }
// The key of a tuned class: a fold-once dtype (the e4m3 wire's granules) times another candidate list — no rings
// at P > 2 — so its classes are kept apart from the summing dtypes' of the same bytes, 256 up.
int tune_class(size_t bytes, int dtype) { return size_class(bytes) + (for_dtype(RingConfig{}, dtype).fold_once ? 256 : 0); }

namespace {

// Candidate schedules for a P-rank communicator (the configured one first). Every rank builds
// the same list: it depends on P, the bucket size and the shared config only.
// With ref_order (or fold_once: the e4m3 wire's granules) every candidate is the schedule that runs
// (effective_config: rings at P > 2 become direct), duplicates dropped, so only those schedules are timed.
std::vector<RingConfig> tune_candidates(int P, size_t bytes, const RingConfig &base) {
    std::vector<RingConfig> c{effective_config(base, P)};
    auto add = [&](int algo, int rings, size_t slice, int max_slices) {
        RingConfig r;
        r.algo = algo;
        r.rings = rings;
        r.slice_bytes = slice;
        r.max_slices = max_slices;
        r.ref_order = base.ref_order;
        r.fold_once = base.fold_once;  // (its rings at P > 2 become direct too: duplicates, dropped below)
        r = effective_config(r, P);
        for (const RingConfig &x : c)
            if (x.algo == r.algo && x.rings == r.rings && x.slice_bytes == r.slice_bytes &&
                x.max_slices == r.max_slices)
                return;
        c.push_back(r);
    };
    const int R = (int)rings_for(P, kMaxRings).size();
    // slices: 512 KiB (deep recv/reduce overlap) .. 64 MiB (one slice per chunk: fewest
    // groups — an RCCL group of 7 send/recv pairs costs ~15-22 us of host enqueue and ~30 us
    // of device latency on MI355X, tools/rccl_group_cost.py)
    add(kAlgoRing, kMaxRings, 2u << 20, 8);
    add(kAlgoRing, kMaxRings, 512u << 10, 16);
    add(kAlgoRing, kMaxRings, 8u << 20, 8);
    add(kAlgoRing, kMaxRings, 64u << 20, 8);
    if (R > 1) add(kAlgoRing, 1, 2u << 20, 8);
    if (P > 2) {
        add(kAlgoDirect, 1, 2u << 20, 8);
        add(kAlgoDirect, 1, 512u << 10, 16);
        add(kAlgoDirect, 1, 8u << 20, 8);
        add(kAlgoDirect, 1, 64u << 20, 8);
        // chunks of up to 4 MiB (a 16 MiB fp16 C4 bucket at P = 8: 2 MiB chunks) also in 8 slices
        // of 256 KiB, so the fold of slice k runs under the reduce-scatter of slice k+1 and only
        // the last eighth of the chunk's fold stays on the bucket's critical path (VERDICT r5
        // next #6; 512 KiB gives 4). More groups cost RCCL group latency: the tuner decides.
        if (bytes <= (size_t)P * (4u << 20)) add(kAlgoDirect, 1, 256u << 10, 16);
        // the same reduce-scatter, the allgather as one ncclAllGather (RCCL's collective
        // kernels instead of K groups of 2(P-1) p2p ops), where the chunks are equal
        if (direct_gather_eligible(bytes, 1, P)) {
            add(kAlgoDirectGather, 1, 2u << 20, 8);
            add(kAlgoDirectGather, 1, 8u << 20, 8);
            add(kAlgoDirectGather, 1, 64u << 20, 8);
        }
    }
    // latency-bound buckets: one group (whole bucket to every peer) instead of two or more;
    // costs (P-1) x the bucket in wire bytes and staging, so only small buckets
    if (bytes <= kOneShotMaxBytes) {
        add(kAlgoOneShot, 1, 0, 1);
        add(kAlgoGatherFold, 1, 0, 1);  // the same fold after one ncclAllGather
    }
    return c;
}

}  // namespace

TuneResult run_tuning(int P, size_t bytes, hipStream_t stream, const RingConfig &base,
                      const std::function<void(const RingConfig &)> &run,
                      const std::function<void(float *, int)> &agree_max) {
    TuneResult res;
    res.candidates = tune_candidates(P, bytes, base);
    const int nc = (int)res.candidates.size();
    const int warm = 2, reps = bytes >= (64u << 20) ? 5 : (bytes >= (4u << 20) ? 10 : 20);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    try {
        DDL_HIP(hipEventCreate(&e0));
        DDL_HIP(hipEventCreate(&e1));
        res.ms.assign(nc, 0.f);
        for (int i = 0; i < nc; ++i) {
            for (int w = 0; w < warm; ++w) run(res.candidates[i]);
            DDL_HIP(hipEventRecord(e0, stream));
            for (int r = 0; r < reps; ++r) run(res.candidates[i]);
            DDL_HIP(hipEventRecord(e1, stream));
            DDL_HIP(hipEventSynchronize(e1));
            float ms = 0;
            DDL_HIP(hipEventElapsedTime(&ms, e0, e1));
            res.ms[i] = ms / reps;
        }
        agree_max(res.ms.data(), nc);
    } catch (...) {
        (void)hipStreamSynchronize(stream);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        throw;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    res.chosen = 0;
    for (int i = 1; i < nc; ++i)
        if (res.ms[i] < res.ms[res.chosen]) res.chosen = i;
    const RingConfig &c = res.candidates[res.chosen];
    DDL_LOG(1, "tuned " << bytes << " B (class " << size_class(bytes) << "): algo " << c.algo << " rings " << c.rings
                        << " slice " << c.slice_bytes << " -> " << res.ms[res.chosen] << " ms (configured: "
                        << res.ms[0] << " ms)");
    return res;
}

// Collective: every rank reaches this for the same bucket size in the same order (buckets are
// issued in the same order on all ranks, as any collective requires), runs the same candidate
// list with the same repetition counts on scratch buffers, and takes the max-over-ranks time of
// each candidate (one ncclAllReduce of nc floats), so all ranks pick the same schedule.
TuneResult Communicator::tune_(size_t n, int dtype, hipStream_t stream, const RingConfig &base) {
    const size_t bytes = n * dtype_size(dtype);
    auto cleanup = [&] { (void)hipStreamSynchronize(stream); };
    if (tune_cap_ < bytes) {  // grow-only scratch, the outgrown pair retired (no hipFree while others run)
        retire_device(tune_a_);
        retire_device(tune_b_);
        tune_a_ = tune_b_ = nullptr;
        tune_cap_ = 0;
        DDL_HIP(hipMalloc(&tune_a_, bytes));
        DDL_HIP(hipMalloc(&tune_b_, bytes));
        tune_cap_ = bytes;
    }
    void *a = tune_a_, *b = tune_b_;
    TuneResult res;
    try {
        DDL_HIP(hipMemsetAsync(a, 0, bytes, stream));
        res = run_tuning(
            size_, bytes, stream, base, [&](const RingConfig &c) { exec_->allreduce(a, b, n, dtype, stream, c); },
            [&](float *ms, int nc) {
                DDL_REQUIRE(nc <= 64, DDL_STATUS_ERROR_UNKNOWN, "too many tuning candidates");
                agree_max_(ms, nc, stream);
            });
    } catch (...) {
        cleanup();
        throw;
    }
    cleanup();
    return res;
}

RingConfig Communicator::ring_config(size_t n, int dtype, hipStream_t stream) {
    const RingConfig base = for_dtype(config().ring(), dtype);  // (fold_once shapes the candidate list, tune_candidates)
    if (size_ <= 1 || n == 0) return base;
    agree_config(stream);
    if (!config().tune.load()) return base;
    if (agreed_hash_ != tuned_hash_) {  // the shared tunables changed: tune again
        tuned_.clear();
        tuned_hash_ = agreed_hash_;
    }
    const int cls = tune_class(n * dtype_size(dtype), dtype);
    auto it = tuned_.find(cls);
    if (it == tuned_.end()) {
        // tuning times candidates and synchronises: inside a graph capture the configured
        // schedule is captured instead (the class is tuned by its first call outside one)
        if (stream_capturing(stream)) return base;
        it = tuned_.emplace(cls, tune_(n, dtype, stream, base)).first;
    }
    return it->second.candidates[it->second.chosen];
}

TuneResult Communicator::tune_result(size_t bytes, int dtype) {
    std::lock_guard<std::mutex> g(mu_);
    auto it = tuned_.find(tune_class(bytes, dtype));
    if (it == tuned_.end() || tuned_hash_ != config().shared_hash()) return TuneResult{};
    return it->second;
}

void Communicator::broadcast(void *buf, size_t n, int dtype, int root, hipStream_t stream) {
    DDL_REQUIRE(dtype_size(dtype) != 0, DDL_STATUS_UNSUPPORTED_DTYPE, "unsupported dtype " << dtype);
    DDL_REQUIRE(root >= 0 && root < size_, DDL_STATUS_INVALID_ARGUMENT, "root " << root << " outside [0, " << size_ << ")");
    DDL_REQUIRE(n == 0 || buf, DDL_STATUS_INVALID_ARGUMENT, "null buffer");
    UserCollective uc(*this);
    std::lock_guard<std::mutex> g(mu_);
    DeviceGuard dg(device_);
    if (n) agree_config(stream);
    exec_->broadcast(buf, n, dtype, root, stream, config().ring());
}

void Communicator::allgatherv(const void *send, void *recv, const size_t *counts, const size_t *displs, int dtype,
                              hipStream_t stream) {
    DDL_REQUIRE(dtype_size(dtype) != 0, DDL_STATUS_UNSUPPORTED_DTYPE, "unsupported dtype " << dtype);
    DDL_REQUIRE(counts && displs, DDL_STATUS_INVALID_ARGUMENT, "null counts/displs");
    DDL_REQUIRE(counts[rank_] == 0 || send, DDL_STATUS_INVALID_ARGUMENT, "null send buffer");
    size_t total = 0;
    for (int q = 0; q < size_; ++q) total += counts[q];
    DDL_REQUIRE(total == 0 || recv, DDL_STATUS_INVALID_ARGUMENT, "null recv buffer");
    UserCollective uc(*this);
    std::lock_guard<std::mutex> g(mu_);
    DeviceGuard dg(device_);
    if (total) agree_config(stream);
    exec_->allgatherv(send, recv, counts, displs, dtype, stream);
}

namespace {

bool host_pinned(const void *p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// Registers a pageable host range for async DMA for the lifetime of the guard.
class HostRegistration {
public:
    HostRegistration(const void *p, size_t bytes) {
        if (!p || !bytes || host_pinned(p)) return;
        DDL_HIP(hipHostRegister(const_cast<void *>(p), bytes, hipHostRegisterDefault));
        p_ = const_cast<void *>(p);
    }
    ~HostRegistration() {
        if (p_) (void)hipHostUnregister(p_);
    }

private:
    void *p_ = nullptr;
};

}  // namespace

void Communicator::allreduce_host(const void *send, void *recv, size_t n, int dtype, int op) {
    check_allreduce_op(op, dtype);
    const size_t es = dtype_size(dtype);
    DDL_REQUIRE(es != 0, DDL_STATUS_UNSUPPORTED_DTYPE, "unsupported dtype " << dtype);
    DDL_REQUIRE(n == 0 || (send && recv), DDL_STATUS_INVALID_ARGUMENT, "null buffer");
    const size_t total = n * es;
    if (total == 0) return;
    UserCollective uc(*this);
    std::lock_guard<std::mutex> g(mu_);
    DeviceGuard dg(device_);
    size_t chunk = (size_t)config().host_chunk_bytes.load();
    chunk = chunk < 4096 ? 4096 : chunk & ~size_t(255);
    if (chunk > total) chunk = (total + 255) & ~size_t(255);
    if (!h2d_) {
        h2d_ = create_engine_stream(qclass_);
        ring_ = create_engine_stream(qclass_);
        d2h_ = create_engine_stream(qclass_);
    }
    if (slot_bytes_ < chunk) {
        for (void *&sl : slots_) {  // outgrown: kept until ddl_finalize (retire_device)
            retire_device(sl);
            sl = nullptr;
        }
        for (void *&sl : slots_) DDL_HIP(hipMalloc(&sl, chunk));
        slot_bytes_ = chunk;
    }
    HostRegistration rs(send, total);
    HostRegistration rr(recv == send ? nullptr : recv, total);
    // per slot: H2D done, ring done, D2H done. kHostSlots chunks in flight: the H2D of chunk i
    // waits only for the D2H of chunk i - kHostSlots, so the copy engines never wait on a
    // cross-stream round trip (2 slots: 14 GiB/s at 4 MiB chunks, 40 at 32 MiB)
    hipEvent_t ev[3 * kHostSlots];
    int made = 0;
    try {
        for (hipEvent_t &e : ev) {
            DDL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            ++made;
        }
        RingConfig cfg = ring_config(chunk / es, dtype, ring_);
        cfg.order_bytes = total;  // the reference reduces the whole host buffer in one call
        const std::vector<size_t> cut = host_chunk_cuts(total, chunk);
        const size_t nchunks = cut.size() - 1;
        for (size_t i = 0; i < nchunks; ++i) {
            const int s = (int)(i % kHostSlots);
            hipEvent_t &h2d_done = ev[3 * s], &ring_done = ev[3 * s + 1], &d2h_done = ev[3 * s + 2];
            const size_t off = cut[i], bytes = cut[i + 1] - off;
            if (i >= (size_t)kHostSlots) DDL_HIP(hipStreamWaitEvent(h2d_, d2h_done, 0));  // slot free again
            DDL_HIP(hipMemcpyAsync(slots_[s], static_cast<const char *>(send) + off, bytes, hipMemcpyHostToDevice, h2d_));
            DDL_HIP(hipEventRecord(h2d_done, h2d_));
            DDL_HIP(hipStreamWaitEvent(ring_, h2d_done, 0));
            exec_->allreduce(slots_[s], slots_[s], bytes / es, dtype, ring_, cfg, op);  // AVG: divided in the slot
            DDL_HIP(hipEventRecord(ring_done, ring_));
            DDL_HIP(hipStreamWaitEvent(d2h_, ring_done, 0));
            DDL_HIP(hipMemcpyAsync(static_cast<char *>(recv) + off, slots_[s], bytes, hipMemcpyDeviceToHost, d2h_));
            DDL_HIP(hipEventRecord(d2h_done, d2h_));
        }
        DDL_HIP(hipStreamSynchronize(d2h_));
    } catch (...) {
        (void)hipStreamSynchronize(h2d_);
        (void)hipStreamSynchronize(ring_);
        (void)hipStreamSynchronize(d2h_);
        for (int k = 0; k < made; ++k) (void)hipEventDestroy(ev[k]);
        throw;
    }
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
}

void Communicator::agree_max_(float *values, int count, hipStream_t stream) {
    if (size_ <= 1) return;
    if (!hooks_) {
        rccl_max_floats(nccl_, values, count, stream);
        return;
    }
    // test transport: every member sends its values to every other member (one group), then
    // each takes the elementwise max — the same numbers on every rank
    std::vector<std::vector<float>> got(size_, std::vector<float>(values, values + count));
    std::vector<ddl_p2p_op> ops;
    for (int d = 1; d < size_; ++d) {
        const int to = (rank_ + d) % size_, from = (rank_ + size_ - d) % size_;
        ops.push_back(ddl_p2p_op{1, to, 4001, values, sizeof(float) * count});
        ops.push_back(ddl_p2p_op{0, from, 4001, got[from].data(), sizeof(float) * count});
    }
    cb_->host_group(ops);
    for (int q = 0; q < size_; ++q)
        for (int i = 0; i < count; ++i) values[i] = std::max(values[i], got[q][i]);
}

namespace {
// One rank's contribution to a split: MPI_Comm_split's (color, key) plus what the new
// communicator needs agreed (the test transport's next tag, the token ring endpoint).
struct SplitRecord {
    int64_t color, key, tag;
    char endpoint[40];
};
static_assert(sizeof(SplitRecord) == 64, "split record is 8 int64 on the wire");
}  // namespace

std::shared_ptr<Communicator> Communicator::split(int color, int key, bool keyed) {
    UserCollective uc(*this);
    std::lock_guard<std::mutex> g(mu_);
    DeviceGuard dg(device_);
    // 1) every rank's record, in rank order, over this communicator's data plane (an allgather,
    //    as MPI_Comm_split does inside MPI)
    std::shared_ptr<ControlChannel> ring;
    SplitRecord mine{};
    mine.color = color < 0 ? -1 : color;
    mine.key = key;
    mine.tag = hooks_ ? hooks_->next_tag.load() : 0;
    if (keyed && color >= 0 && size_ > 1) {
        ring = std::make_shared<ControlChannel>();
        const std::string ep = ring->listen();
        DDL_REQUIRE(ep.size() < sizeof mine.endpoint, DDL_STATUS_ERROR_UNKNOWN, "endpoint too long: " << ep);
        std::memcpy(mine.endpoint, ep.c_str(), ep.size() + 1);
    }
    std::vector<SplitRecord> all(size_);
    all[rank_] = mine;
    if (size_ > 1) {
        void *d = nullptr;
        hipStream_t s = nullptr;
        auto release = [&] {
            if (s) (void)hipStreamSynchronize(s);
            if (s) (void)hipStreamDestroy(s);
        };
        try {
            DDL_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
            d = thread_scratch(sizeof(SplitRecord) * size_);
            char *base = static_cast<char *>(d);
            DDL_HIP(hipMemcpyAsync(base + sizeof(SplitRecord) * rank_, &mine, sizeof mine, hipMemcpyHostToDevice, s));
            std::vector<size_t> cnt(size_, sizeof(SplitRecord) / 8), dsp(size_);
            for (int q = 0; q < size_; ++q) dsp[q] = q * (sizeof(SplitRecord) / 8);
            exec_->allgatherv(base + sizeof(SplitRecord) * rank_, base, cnt.data(), dsp.data(), DDL_INT64, s);
            DDL_HIP(hipMemcpyAsync(all.data(), d, sizeof(SplitRecord) * size_, hipMemcpyDeviceToHost, s));
            DDL_HIP(hipStreamSynchronize(s));
        } catch (...) {
            release();
            throw;
        }
        release();
    }
    // 2) the members of my color, ordered by (key, rank here)
    std::vector<int> members;
    int64_t tag = 0;
    for (int q = 0; q < size_; ++q) {
        tag = std::max(tag, all[q].tag);
        if (color >= 0 && all[q].color == color) members.push_back(q);
    }
    std::stable_sort(members.begin(), members.end(), [&](int a, int b) { return all[a].key < all[b].key; });
    const int me = (int)(std::find(members.begin(), members.end(), rank_) - members.begin());
    const int s = (int)members.size();
    // 3) the data plane of the new communicator
    std::shared_ptr<Communicator> c;
    if (hooks_) {
        // tags only need to differ between communicators that share a pair of ranks: the max
        // over this communicator's ranks is above every tag any member has used
        long long want = tag + 1, cur = hooks_->next_tag.load();
        while (cur < want && !hooks_->next_tag.compare_exchange_weak(cur, want)) {
        }
        DDL_REQUIRE(color >= 0, DDL_STATUS_INVALID_ARGUMENT, "negative color: rank is in no communicator");
        std::vector<int> wr;
        for (int q : members) wr.push_back(world_ranks_.empty() ? q : world_ranks_[q]);
        c = new_communicator(me, s, device_, nullptr, s > 1 ? hooks_ : nullptr, tag, wr);
    } else if (nccl_) {
        int r = 0, n = 0;
        ncclComm_t nc = rccl_split(nccl_, color, key, &r, &n);
        DDL_REQUIRE(nc != nullptr, DDL_STATUS_INVALID_ARGUMENT, "negative color: rank is in no communicator");
        DDL_REQUIRE(r == me && n == s, DDL_STATUS_COMM_ERROR,
                    "ncclCommSplit gave rank " << r << " of " << n << ", the split exchange " << me << " of " << s);
        // queue class (executor.h QueueClass): a user split the least priority's pool; a private
        // keyed communicator (keyed == false, made by enable_keyed) its owner's keyed class
        const QueueClass qc = keyed ? QueueClass::kLow : keyed_qclass_;
        c = new_communicator(r, n, device_, nc, nullptr, 0, std::vector<int>{}, qc);
    } else {
        DDL_REQUIRE(color >= 0, DDL_STATUS_INVALID_ARGUMENT, "negative color: rank is in no communicator");
        c = new_communicator(0, 1, device_, nullptr);
    }
    // 4) its token ring and keyed data plane (collective over the new communicator)
    if (keyed && s > 1) {
        std::vector<std::string> eps;
        for (int q : members) eps.push_back(std::string(all[q].endpoint));
        ring->connect(me, s, eps, 120000);
        c->enable_keyed(ring);
    }
    return c;
}

void Communicator::enable_keyed(std::shared_ptr<ControlChannel> ch) {
    DDL_REQUIRE(size_ == 1 || (ch && ch->connected() && ch->size() == size_ && ch->rank() == rank_),
                DDL_STATUS_INVALID_ARGUMENT, "token ring does not match the communicator");
    control_ = std::move(ch);
    // private data-plane communicator: the handler thread's collectives never interleave with
    // the user's calls on this one
    if (size_ > 1 && !keyed_data_) keyed_data_ = split(0, rank_, false);
}

// The ncclConfig_t of a new communicator: RCCL's defaults but for the CTA bounds the config
// names (0 = undefined). *custom says whether anything differs from ncclCommInitRank's defaults.
static ncclConfig_t rccl_comm_config(bool *custom) {
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    const long long lo = config().rccl_min_ctas.load(), hi = config().rccl_max_ctas.load();
    DDL_REQUIRE(!lo || !hi || lo <= hi, DDL_STATUS_INVALID_ARGUMENT,
                "rccl_min_ctas " << lo << " > rccl_max_ctas " << hi);
    if (lo) cfg.minCTAs = (int)lo;
    if (hi) cfg.maxCTAs = (int)hi;
    *custom = lo || hi;
    return cfg;
}

ncclComm_t rccl_init_rank(int rank, int size, const void *unique_id, size_t len) {
    DDL_REQUIRE(unique_id && len >= sizeof(ncclUniqueId), DDL_STATUS_INVALID_ARGUMENT,
                "unique id of " << sizeof(ncclUniqueId) << " bytes required");
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof id);
    ncclComm_t nc = nullptr;
    bool custom = false;
    ncclConfig_t cfg = rccl_comm_config(&custom);
    if (rccl().CommInitRankConfig) {
        rccl_check(rccl().CommInitRankConfig(&nc, size, id, rank, &cfg), "ncclCommInitRankConfig");
    } else {
        DDL_REQUIRE(!custom, DDL_STATUS_COMM_ERROR,
                    "rccl_min_ctas / rccl_max_ctas need ncclCommInitRankConfig, which " << rccl().path << " lacks");
        rccl_check(rccl().CommInitRank(&nc, size, id, rank), "ncclCommInitRank");
    }
    return nc;
}

ncclComm_t rccl_split(ncclComm_t parent, int color, int key, int *rank, int *size) {
    ncclComm_t nc = nullptr;
    bool custom = false;
    ncclConfig_t cfg = rccl_comm_config(&custom);
    rccl_check(rccl().CommSplit(parent, color < 0 ? NCCL_SPLIT_NOCOLOR : color, key, &nc, &cfg), "ncclCommSplit");
    if (!nc) return nullptr;
    rccl_check(rccl().CommCount(nc, size), "ncclCommCount");
    rccl_check(rccl().CommUserRank(nc, rank), "ncclCommUserRank");
    return nc;
}

void rccl_max_floats(ncclComm_t comm, float *values, int count, hipStream_t stream) {
    DDL_REQUIRE(count > 0 && count <= 1024, DDL_STATUS_INVALID_ARGUMENT, "max of " << count << " floats");
    float *d = static_cast<float *>(thread_scratch(sizeof(float) * count));
    try {
        DDL_HIP(hipMemcpyAsync(d, values, sizeof(float) * count, hipMemcpyHostToDevice, stream));
        rccl_check(rccl().AllReduce(d, d, count, ncclFloat32, ncclMax, comm, stream), "ncclAllReduce(max)");
        DDL_HIP(hipMemcpyAsync(values, d, sizeof(float) * count, hipMemcpyDeviceToHost, stream));
        DDL_HIP(hipStreamSynchronize(stream));
    } catch (...) {
        (void)hipStreamSynchronize(stream);
        throw;
    }
}

void rccl_allgather_u64(ncclComm_t comm, uint64_t *values, int size, int rank, hipStream_t stream) {
    uint64_t *d = static_cast<uint64_t *>(thread_scratch(sizeof(uint64_t) * size));
    try {
        DDL_HIP(hipMemcpyAsync(d + rank, values + rank, sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        rccl_check(rccl().AllGather(d + rank, d, sizeof(uint64_t), ncclInt8, comm, stream), "ncclAllGather(config)");
        DDL_HIP(hipMemcpyAsync(values, d, sizeof(uint64_t) * size, hipMemcpyDeviceToHost, stream));
        DDL_HIP(hipStreamSynchronize(stream));
    } catch (...) {
        (void)hipStreamSynchronize(stream);
        throw;
    }
}

RequestHandler *Communicator::handler_if_created() {
    std::lock_guard<std::mutex> g(handler_mu_);
    return handler_.get();
}

RequestHandler &Communicator::handler() {
    std::lock_guard<std::mutex> g(handler_mu_);
    if (!handler_) handler_.reset(new RequestHandler(this));
    return *handler_;
}

// ---- registry ------------------------------------------------------------------------------
thread_local bool t_handler_thread = false;

// Deferred deletions (a communicator whose last owner was one of its own handler's threads: its
// destructor joins those threads, so it runs on a thread of its own). They are counted, and
// ddl_finalize and process exit wait for them: the destructor's SHUT_DOWN lap,
// ncclCommDestroy and hipStreamDestroy must not race HIP / RCCL teardown or finalize hooks.
// Heap-allocated and never freed, so the exit hook never sees them destroyed.
namespace {
struct Reaper {
    std::mutex mu;
    std::condition_variable cv;
    int pending = 0;
};
Reaper &reaper() {
    static Reaper *r = new Reaper();
    return *r;
}
void wait_deferred_deletions_at_exit() { wait_deferred_deletions(10000); }
}  // namespace

bool wait_deferred_deletions(long long limit_ms) {
    // on a handler thread (ddl_finalize from a done() callback) the deletions may be joining this
    // very thread: waiting would deadlock, so they are left to finish on their own
    if (t_handler_thread) return true;
    Reaper &r = reaper();
    std::unique_lock<std::mutex> g(r.mu);
    return r.cv.wait_for(g, std::chrono::milliseconds(limit_ms), [&] { return r.pending == 0; });
}

namespace {
struct Retired {
    std::mutex mu;
    std::vector<void *> dev, host;
};
Retired &retired() {
    static Retired *r = new Retired();  // never destroyed: threads may retire at exit
    return *r;
}
struct ThreadScratch {
    std::vector<std::pair<void *, size_t>> per_device;  // index = device ordinal
    ~ThreadScratch() {
        for (auto &p : per_device)
            if (p.first) retire_device(p.first);
    }
};
thread_local ThreadScratch t_scratch;
}  // namespace

void retire_device(void *p) {
    if (!p) return;
    std::lock_guard<std::mutex> g(retired().mu);
    retired().dev.push_back(p);
}

void retire_host(void *p) {
    if (!p) return;
    std::lock_guard<std::mutex> g(retired().mu);
    retired().host.push_back(p);
}

void free_retired() {
    std::vector<void *> dev, host;
    {
        std::lock_guard<std::mutex> g(retired().mu);
        dev.swap(retired().dev);
        host.swap(retired().host);
    }
    for (void *p : dev) (void)hipFree(p);
    for (void *p : host) (void)hipHostFree(p);
}

void *thread_scratch(size_t bytes) {
    int dev = 0;
    DDL_HIP(hipGetDevice(&dev));
    auto &v = t_scratch.per_device;
    if ((size_t)dev >= v.size()) v.resize((size_t)dev + 1, {nullptr, 0});
    auto &slot = v[(size_t)dev];
    if (slot.second < bytes) {
        retire_device(slot.first);  // a stream may still read it: kept until ddl_finalize
        slot = {nullptr, 0};
        const size_t sz = std::max<size_t>(bytes, 16384);
        DDL_HIP(hipMalloc(&slot.first, sz));
        slot.second = sz;
    }
    return slot.first;
}

void CommunicatorDeleter::operator()(Communicator *c) const {
    if (!t_handler_thread) {
        delete c;
        return;
    }
    static const bool at_exit = std::atexit(wait_deferred_deletions_at_exit) == 0;
    (void)at_exit;
    Reaper &r = reaper();
    {
        std::lock_guard<std::mutex> g(r.mu);
        ++r.pending;
    }
    try {
        std::thread([c, &r] {
            delete c;
            std::lock_guard<std::mutex> g(r.mu);
            if (--r.pending == 0) r.cv.notify_all();
        }).detach();
    } catch (const std::exception &e) {
        // no thread to be had: deleting here would join this very thread, so the communicator is
        // left allocated (its handler keeps running until exit) rather than deadlock
        DDL_LOG(0, "communicator " << c << " leaked: no thread for its deferred deletion (" << e.what() << ")");
        std::lock_guard<std::mutex> g(r.mu);
        if (--r.pending == 0) r.cv.notify_all();
    }
}

Registry &Registry::get() {
    static Registry *r = new Registry();  // leaked on purpose: no static-destruction order issues
    return *r;
}

void Registry::add(const std::shared_ptr<Communicator> &c) {
    std::lock_guard<std::mutex> g(mu_);
    comms_[c->id()] = c;
}

std::shared_ptr<Communicator> Registry::find(long long id) {
    std::lock_guard<std::mutex> g(mu_);
    auto it = comms_.find(id);
    DDL_REQUIRE(it != comms_.end(), DDL_STATUS_INVALID_ARGUMENT, "unknown communicator id " << id);
    return it->second;
}

void Registry::detach(long long id) {
    std::shared_ptr<Communicator> keep;
    {
        std::lock_guard<std::mutex> g(mu_);
        auto it = comms_.find(id);
        if (it == comms_.end()) return;
        if (world_ && world_->id() == id) return;  // the world stays until ddl_finalize
        keep = it->second;
        comms_.erase(it);
    }
}

std::shared_ptr<Communicator> Registry::world() {
    std::lock_guard<std::mutex> g(mu_);
    DDL_REQUIRE(world_ != nullptr, DDL_STATUS_NOT_INITIALIZED, "ddl_init has not been called");
    return world_;
}

void Registry::set_world(const std::shared_ptr<Communicator> &c) {
    std::lock_guard<std::mutex> g(mu_);
    DDL_REQUIRE(world_ == nullptr, DDL_STATUS_INVALID_ARGUMENT, "already initialized");
    world_ = c;
    comms_[c->id()] = c;
}

void Registry::clear() {
    std::map<long long, std::shared_ptr<Communicator>> comms;
    std::shared_ptr<Communicator> w;
    {
        std::lock_guard<std::mutex> g(mu_);
        comms.swap(comms_);
        w.swap(world_);
    }
    comms.clear();
    w.reset();
}

std::vector<std::shared_ptr<Communicator>> Registry::all() {
    std::lock_guard<std::mutex> g(mu_);
    std::vector<std::shared_ptr<Communicator>> v;
    for (auto &kv : comms_) v.push_back(kv.second);
    return v;
}

bool Registry::initialized() {
    std::lock_guard<std::mutex> g(mu_);
    return world_ != nullptr;
}

namespace {
std::mutex &finalize_mu() {
    static std::mutex *mu = new std::mutex;
    return *mu;
}
std::vector<void (*)()> &finalize_hooks() {
    static auto *v = new std::vector<void (*)()>;
    return *v;
}
}  // namespace

void add_finalize_hook(void (*fn)()) {
    std::lock_guard<std::mutex> g(finalize_mu());
    finalize_hooks().push_back(fn);
}

void run_finalize_hooks() {
    std::vector<void (*)()> v;
    {
        std::lock_guard<std::mutex> g(finalize_mu());
        v = finalize_hooks();
    }
    for (auto fn : v) fn();
}

}  // namespace ddl
