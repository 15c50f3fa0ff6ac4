// handler.cpp — see handler.h.
#include "handler.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <thread>
#include <tuple>

namespace ddl {

std::vector<Plan> make_plans(const std::vector<size_t> &elements, const std::vector<size_t> &esize,
                             size_t limit) {
    std::vector<Plan> plans;
    const size_t nreq = elements.size();
    if (nreq == 0) return plans;
    DDL_REQUIRE(limit > 0, DDL_STATUS_INVALID_ARGUMENT, "fusion threshold must be > 0");
    std::vector<size_t> begins(nreq);
    size_t all = 0;
    for (size_t i = 0; i < nreq; ++i) {
        begins[i] = all;
        all += elements[i] * esize[i];
    }
    size_t byte_size = 0, pb = 0, pbe = 0;
    while (byte_size < all) {
        size_t pe = nreq - 1, pe_elem = elements[nreq - 1];
        byte_size += limit;
        if (byte_size < all) {
            for (size_t i = pb; i < nreq; ++i) {
                if (i == nreq - 1 || (begins[i] < byte_size && byte_size <= begins[i + 1])) {
                    pe = i;
                    pe_elem = (byte_size - begins[i]) / esize[i];
                    break;
                }
            }
        }
        // a plan must make progress: if the cap is below one element, take one element
        if (pe == pb && pe_elem <= pbe) pe_elem = pbe + 1;
        plans.push_back(Plan{pb, pbe, pe, pe_elem});
        if (pe_elem == elements[pe]) {
            pb = pe + 1;
            pbe = 0;
        } else {
            pb = pe;
            pbe = pe_elem;
        }
        byte_size = begins[pe] + esize[pe] * pe_elem;
    }
    return plans;
}

ReqId req_id(const Request &r) { return ReqId{type_order(r.type), r.key}; }

ReadyEvent::ReadyEvent(hipStream_t s) {
    DDL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    hipError_t r = hipEventRecord(e, s);
    if (r != hipSuccess) {
        (void)hipEventDestroy(e);
        e = nullptr;
        DDL_HIP(r);
    }
}

ReadyEvent::~ReadyEvent() {
    if (e) (void)hipEventDestroy(e);
}

RequestHandler::RequestHandler(Communicator *owner) : owner_(owner) {
    DeviceGuard g(owner_->device());
    if (owner_->size() > 1) {
        ch_ = owner_->control();
        DDL_REQUIRE(ch_ && ch_->connected() && ch_->size() == owner_->size() && ch_->rank() == owner_->rank() &&
                        owner_->keyed_data(),
                    DDL_STATUS_NOT_INITIALIZED,
                    "keyed requests at size > 1 need the communicator's token ring (ddl_control_connect for the "
                    "world; split_communicator builds one for every split)");
        // the private data-plane communicator made with the ring (Communicator::enable_keyed)
        data_ = owner_->keyed_data().get();
    } else {
        data_ = owner_;
    }
    // the fusion pack / unpack kernels overlap other plans' RCCL kernels at size > 1: the same CU
    // mask as the executors' compute streams (config compute_cu_mask; pack / unpack keep their
    // rate on it, tools/cu_mask_probe.py)
    // its hardware-queue class (executor.h QueueClass): apart from the user's streams
    stream_ = create_engine_stream(owner_->keyed_queue_class(), owner_->size() > 1 ? config_compute_cu_mask() : 0);
    fp_.qc = owner_->keyed_queue_class();
    host_.reset(new HostStager(owner_->device(), owner_->keyed_queue_class(), stream_, fp_.copier));
    done_thread_ = std::thread(&RequestHandler::completer_, this);
    thread_ = std::thread(&RequestHandler::main_, this);
}

RequestHandler::~RequestHandler() {
    {
        std::lock_guard<std::mutex> g(mu_);
        stop_ = true;
    }
    cv_.notify_all();
    // a round waiting in round_enter for user collectives that will never be issued now fails
    // (the communicator is going away) instead of blocking the join below
    owner_->round_abort(DDL_STATUS_NOT_INITIALIZED, "the communicator is being destroyed");
    if (thread_.joinable()) thread_.join();
    {  // the rounds already handed over complete (or fail) first, in order
        std::lock_guard<std::mutex> g(done_mu_);
        done_stop_ = true;
    }
    done_cv_.notify_all();
    if (done_thread_.joinable()) done_thread_.join();
    fail_all_(DDL_STATUS_COMM_ERROR);
    for (hipEvent_t e : free_events_) (void)hipEventDestroy(e);
    for (StatBlock &b : free_stat_) (void)hipHostFree(b.p);
    if (gather_) (void)hipFree(gather_);
    if (dims_) (void)hipFree(dims_);
    for (auto &kv : residuals_)  // the error-feedback residuals live as long as the handler
        if (kv.second.ptr) (void)hipFree(kv.second.ptr);
    host_.reset();  // the host path's slots, streams and registrations (its work waits on stream_)
    if (stream_) (void)hipStreamDestroy(stream_);
}

namespace {
void validate(const Request &r, int size) {
    DDL_REQUIRE(dtype_size(r.dtype) != 0 && r.dtype != kDtypeE4m3, DDL_STATUS_UNSUPPORTED_DTYPE,
                "unsupported dtype " << r.dtype);
    switch (r.type) {
        case kReqAllreduce:
            check_allreduce_op(r.op, r.dtype);
            DDL_REQUIRE(r.wire == 0 || (r.dtype == DDL_FLOAT && !r.host &&
                                        (r.wire == DDL_HALF || r.wire == DDL_BFLOAT16 || r.wire == kDtypeE4m3)),
                        DDL_STATUS_INVALID_ARGUMENT, "wire dtype " << r.wire << " on a " << dtype_name(r.dtype) << " request");
            check_wire_ranks(r.wire, size);
            DDL_REQUIRE(r.wire != kDtypeE4m3 || !op_is_minmax(r.op), DDL_STATUS_INVALID_ARGUMENT,
                        "the e4m3 wire takes SUM or AVG");
            DDL_REQUIRE(!r.feedback || r.wire != 0, DDL_STATUS_INVALID_ARGUMENT, "error feedback without a wire dtype");
            DDL_REQUIRE(!r.stochastic || (r.wire == DDL_BFLOAT16 && !r.feedback), DDL_STATUS_INVALID_ARGUMENT,
                        "stochastic rounding takes the bfloat16 wire and no error feedback");
            DDL_REQUIRE(r.n == 0 || (r.in && r.out), DDL_STATUS_INVALID_ARGUMENT, "null buffer");
            DDL_REQUIRE(!r.sumsq || r.dtype == DDL_FLOAT || r.dtype == DDL_BFLOAT16, DDL_STATUS_UNSUPPORTED_DTYPE,
                        "the sum of squares is defined for float32 and bfloat16 requests, not " << dtype_name(r.dtype));
            DDL_REQUIRE(!r.sumsq || (!r.host && !op_is_minmax(r.op)), DDL_STATUS_INVALID_ARGUMENT,
                        "the sum of squares takes a SUM or AVG request in device memory");
            DDL_REQUIRE(std::isfinite(r.prescale) && r.prescale > 0.0f && std::isfinite(r.postscale) && r.postscale > 0.0f,
                        DDL_STATUS_INVALID_ARGUMENT, "scale factors must be finite and positive");
            if (r.prescale != 1.0f || r.postscale != 1.0f) {
                DDL_REQUIRE(r.dtype == DDL_FLOAT || r.dtype == DDL_BFLOAT16, DDL_STATUS_UNSUPPORTED_DTYPE,
                            "scale factors are defined for float32 and bfloat16 requests, not " << dtype_name(r.dtype));
                DDL_REQUIRE(!r.host && !op_is_minmax(r.op), DDL_STATUS_INVALID_ARGUMENT,
                            "scale factors take a SUM or AVG request in device memory");
            }
            break;
        case kReqBroadcast:
            DDL_REQUIRE(r.root >= 0 && r.root < size, DDL_STATUS_INVALID_ARGUMENT,
                        "root " << r.root << " outside [0, " << size << ")");
            DDL_REQUIRE(r.n == 0 || (r.in && r.out), DDL_STATUS_INVALID_ARGUMENT, "null buffer");
            break;
        case kReqAllgather:
            DDL_REQUIRE(r.alloc != nullptr, DDL_STATUS_INVALID_ARGUMENT, "allgather needs an output allocator");
            DDL_REQUIRE(r.row_elems > 0 && r.n == r.first_dim * r.row_elems, DDL_STATUS_INVALID_ARGUMENT,
                        "allgather: elements " << r.n << " != first_dim " << r.first_dim << " x row " << r.row_elems);
            DDL_REQUIRE(r.n == 0 || r.in, DDL_STATUS_INVALID_ARGUMENT, "null buffer");
            break;
        default: fail(DDL_STATUS_INVALID_ARGUMENT, "unknown request type " + std::to_string(r.type));
    }
}
}  // namespace

// A request whose id was agreed before gets its id-table index (under mu_).
void RequestHandler::mark_cached_(const ReqId &id, Request &r) {
    r.cidx = -1;
    if (id.order < 0 || id.order >= 3 || cache_by_key_[id.order].empty()) return;  // (no hashing at size 1)
    auto it = cache_by_key_[id.order].find(id.key);
    if (it == cache_by_key_[id.order].end()) return;
    r.cidx = it->second;
    pend_flag_[it->second] = 1;
}

void RequestHandler::submit(Request r) {
    validate(r, owner_->size());
    {
        std::lock_guard<std::mutex> g(mu_);
        DDL_REQUIRE(!stop_, DDL_STATUS_NOT_INITIALIZED, "handler is shutting down");
        ReqId id = req_id(r);
        DDL_REQUIRE(pending_.find(id) == pending_.end(), DDL_STATUS_DUPLICATE_KEY,
                    "a request with key '" << r.key << "' is already pending");
        mark_cached_(id, r);
        pending_.emplace(std::move(id), std::move(r));
    }
    cv_.notify_all();
}

void RequestHandler::submit_batch(std::vector<Request> &rs) {
    for (const Request &r : rs) validate(r, owner_->size());
    {
        std::lock_guard<std::mutex> g(mu_);
        DDL_REQUIRE(!stop_, DDL_STATUS_NOT_INITIALIZED, "handler is shutting down");
        std::vector<ReqId> ids;
        ids.reserve(rs.size());
        for (const Request &r : rs) ids.push_back(req_id(r));
        std::vector<size_t> order(rs.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = i;
        auto by_id = [&](size_t a, size_t b) { return ids[a] < ids[b]; };
        if (!std::is_sorted(order.begin(), order.end(), by_id)) std::sort(order.begin(), order.end(), by_id);
        // duplicates inside the batch, then against the pending map by one forward walk
        auto pit = pending_.empty() ? pending_.end() : pending_.lower_bound(ids[order[0]]);
        for (size_t i = 0; i < order.size(); ++i) {
            const ReqId &id = ids[order[i]];
            while (pit != pending_.end() && pit->first < id) ++pit;
            DDL_REQUIRE((pit == pending_.end() || id < pit->first) && (i == 0 || ids[order[i - 1]] < id),
                        DDL_STATUS_DUPLICATE_KEY, "a request with key '" << id.key << "' is already pending");
        }
        // sorted insertion with hints: amortised O(1) per request
        auto hint = pending_.end();
        for (size_t i = order.size(); i-- > 0;) {
            const size_t j = order[i];
            mark_cached_(ids[j], rs[j]);
            hint = pending_.emplace_hint(hint, std::move(ids[j]), std::move(rs[j]));
        }
    }
    cv_.notify_all();
}

void RequestHandler::wait_all() {
    std::unique_lock<std::mutex> lk(mu_);
    idle_cv_.wait(lk, [this] { return (pending_.empty() && inflight_ == 0) || stop_; });
}

std::atomic<int> g_control_fault{0};
void set_testing_control_fault(int on) { g_control_fault = on ? 1 : 0; }

void RequestHandler::fail_all_(int status) {
    std::vector<Request> left;
    {
        std::lock_guard<std::mutex> g(mu_);
        left.reserve(pending_.size());
        for (auto &kv : pending_) left.push_back(std::move(kv.second));
        pending_.clear();  // the nodes go back to the pool under mu_
        std::fill(pend_flag_.begin(), pend_flag_.end(), 0);
    }
    for (Request &r : left) {
        if (r.done) r.done(status, r.user);
    }
    idle_cv_.notify_all();
}

void RequestHandler::main_() {
    t_handler_thread = true;  // engine.h: no communicator is destroyed on this thread
    try {
        DDL_HIP(hipSetDevice(owner_->device()));
        // the engine thread takes a share of every host pack / unpack: it and the copy threads
        // run on the GPU's NUMA node (config host_numa_bind, read when the handler starts)
        if (config().host_numa_bind.load()) host_->bind_to_gpu_node();
        ControlChannel *ch = ch_;  // null at size 1
        const int P = owner_->size(), rank = owner_->rank();
        for (;;) {
            if (P == 1 || rank == 0) {
                std::vector<ReqId> keys;
                {
                    std::unique_lock<std::mutex> lk(mu_);
                    cv_.wait(lk, [this] { return stop_ || failed_.load() || !pending_.empty(); });
                    if (failed_.load()) fail(failed_.load(), "a keyed round failed on the device");
                    if (stop_) break;
                    // optional fusion window: let more registrations join this round
                    const long long cycle_us = config().cycle_time_us.load();
                    if (cycle_us > 0)
                        cv_.wait_for(lk, std::chrono::microseconds(cycle_us), [this] { return stop_; });
                    if (stop_) break;
                    if (P == 1) {  // (rank 0 of a ring builds its proposal in root_round_)
                        keys.reserve(pending_.size());
                        const int order = pending_.begin()->first.order;
                        for (auto &kv : pending_)
                            if (kv.first.order == order) keys.push_back(kv.first);
                    }
                }
                if (P == 1) execute_(keys);
                else root_round_();  // negotiation lap times: DDL_LOG level 3 in root_round_
            } else {
                if (failed_.load()) fail(failed_.load(), "a keyed round failed on the device");
                Token t;
                bool got = ch->recv(t, 50);
                if (!got) {
                    std::lock_guard<std::mutex> g(mu_);
                    if (stop_ && pending_.empty()) {
                        // rank 0 shuts the channel down; keep listening a little for it
                        Token s;
                        if (ch->recv(s, 5000) && s.type == TOKEN_SHUT_DOWN) ch->send(s);
                        break;
                    }
                    continue;
                }
                if (t.type == TOKEN_SHUT_DOWN) {
                    ch->send(t);  // the acknowledgement
                    break;
                }
                member_round_(t);
            }
        }
        if (P > 1 && rank == 0) {  // SHUT_DOWN to every member, then their acknowledgements
            Token s;                // (the reference's SHUT_DOWN lap, RingTokenCommunicateHandler.cc:34-48)
            s.type = TOKEN_SHUT_DOWN;
            s.request = TOKEN_REQUEST_SHUTDOWN;
            s.msg = "shut down";
            ch->send(s);
            for (int r = 1; r < P; ++r) {
                Token back;
                try {
                    while (ch->recv_from(r, back, 5000) && back.type != TOKEN_SHUT_DOWN) {
                    }
                } catch (const Error &) {  // a member that already left closed its link
                }
            }
        }
    } catch (const Error &e) {
        DDL_LOG(0, "request handler stopped: " << e.msg);
        // a freeze taken by this round's snapshot is cleared here, and the user collectives waiting
        // behind it (or issued later) fail instead of blocking: with the round's place unknown their
        // order against the keyed data plane is no longer defined
        owner_->round_abort(e.status, e.msg);
        // the other ends see the link close (EOF) and stop as well, instead of waiting for a token
        if (ch_) ch_->close_all();
        fail_all_(e.status);
    } catch (const std::exception &e) {
        DDL_LOG(0, "request handler stopped: " << e.what());
        owner_->round_abort(DDL_STATUS_COMM_ERROR, e.what());
        if (ch_) ch_->close_all();
        fail_all_(DDL_STATUS_COMM_ERROR);
    }
    {
        std::lock_guard<std::mutex> g(mu_);
        stop_ = true;
    }
    idle_cv_.notify_all();
}

void RequestHandler::forget_ids_() {
    cache_req_.clear();
    for (auto &m : cache_by_key_) m.clear();
    pend_flag_.clear();
    for (auto &kv : pending_) kv.second.cidx = -1;
}

// The agreed ids in execution order. A string round teaches the id table the new ids (every
// rank learns the same list in the same order); the pending requests among them get their
// index, so the next round with the same key set goes by index.
std::vector<ReqId> RequestHandler::agreed_ids_(const Agreed &a) {
    std::vector<ReqId> ids;
    std::lock_guard<std::mutex> g(mu_);
    if (a.cached) {
        ids.reserve(a.idx.size());
        for (uint32_t i : a.idx) {
            DDL_REQUIRE(i < cache_req_.size(), DDL_STATUS_COMM_ERROR, "token: id index out of range");
            ids.push_back(cache_req_[i]);
        }
        std::sort(ids.begin(), ids.end());
        return ids;
    }
    ControlChannel &ch = *ch_;
    if (ch.cache.learn(a.wire)) forget_ids_();
    for (size_t j = cache_req_.size(); j < ch.cache.size(); ++j) {  // mirror every new table entry
        ReqId rid = parse_wire_id(ch.cache.at((uint32_t)j));
        cache_by_key_[rid.order][rid.key] = (uint32_t)j;
        pend_flag_.push_back(0);
        auto it = pending_.find(rid);
        if (it != pending_.end()) {
            it->second.cidx = (int64_t)j;
            pend_flag_[j] = 1;
        }
        cache_req_.push_back(std::move(rid));
    }
    ids.reserve(a.wire.size());
    for (const auto &w : a.wire) ids.push_back(parse_wire_id(w));
    return ids;
}

// Rank 0: propose every registered id of one type (SYNC to every member — each intersects and
// answers), then announce the agreed set (COMMUNICATE) and run it.
void RequestHandler::root_round_() {
    ControlChannel &ch = *ch_;
    // one request type per round (the token carries one RequestType): the type of the first
    // registered id, as the reference proposes registeredRequest_.begin() (:184-190)
    std::vector<std::string> strs;
    std::vector<uint32_t> idx;
    bool cached = true;
    int type = kReqAllreduce;
    {
        std::lock_guard<std::mutex> g(mu_);
        if (!pending_.empty()) type = pending_.begin()->second.type;
        for (auto &kv : pending_) {
            if (kv.second.type != type) continue;
            if (kv.second.cidx < 0) cached = false;
            if (cached) idx.push_back((uint32_t)kv.second.cidx);
        }
        if (!cached)
            for (auto &kv : pending_)
                if (kv.second.type == type) strs.push_back(wire_id(kv.first));
        cached = cached && !idx.empty();
    }
    const Agreed a = negotiate_root(ch, cached, idx, strs, type, [this] { return owner_->round_freeze(); });
    run_agreed_(a);
}

void RequestHandler::run_agreed_(const Agreed &a) {
    struct Unfreeze {  // user collectives go on whatever happens to the round
        Communicator *c;
        ~Unfreeze() { c->round_unfreeze(); }
    } unfreeze{owner_};
    owner_->round_release(a.release);
    std::vector<ReqId> ids = agreed_ids_(a);
    owner_->round_enter(a.release);
    execute_(ids, a.cfg_ok ? DDL_STATUS_OK : DDL_STATUS_CONFIG_MISMATCH);
}

// Other ranks: answer the SYNC once the first proposed id is registered here (the reference
// parks the READY token the same way, RingTokenCommunicateHandler.cc:225-250) with the
// intersection, then take COMMUNICATE and run the agreed set (:302-310).
void RequestHandler::member_round_(Token &t) {
    const Agreed a = negotiate_member(
        *ch_, t,
        [this](const std::vector<std::string> &keys) {
            std::vector<ReqId> proposed;
            for (const auto &w : keys) proposed.push_back(parse_wire_id(w));
            std::vector<std::string> mine;
            std::unique_lock<std::mutex> lk(mu_);
            if (!proposed.empty()) cv_.wait(lk, [&] { return stop_ || pending_.count(proposed.front()) > 0; });
            for (size_t i = 0; i < proposed.size(); ++i)
                if (pending_.count(proposed[i])) mine.push_back(keys[i]);
            return mine;
        },
        [this](const std::vector<uint32_t> &proposed) {
            std::vector<uint32_t> mine;
            std::unique_lock<std::mutex> lk(mu_);
            auto held = [&](uint32_t i) { return i < pend_flag_.size() && pend_flag_[i]; };
            if (!proposed.empty()) cv_.wait(lk, [&] { return stop_ || held(proposed.front()); });
            for (uint32_t i : proposed)
                if (held(i)) mine.push_back(i);
            return mine;
        },
        [this] {
            const long long at = owner_->round_freeze();
            // test hook (ddl_testing_control_fault): the control link is lost right after this
            // rank froze its user collectives for the round — the answer below cannot be sent
            if (g_control_fault.exchange(0)) ch_->close_all();
            return at;
        });
    run_agreed_(a);
}

void *RequestHandler::ensure_(void *&buf, size_t &cap, size_t need) {
    if (need > cap) {
        if (buf) {  // may still be read on the device; no hipFree on a data path (engine.h retire_device)
            retire_device(buf);
            buf = nullptr;
            cap = 0;
        }
        const size_t sz = need + need / 2;  // x1.5 growth (MPIRingTokenCommunication.cc:13, 480)
        DDL_HIP(hipMalloc(&buf, sz));
        cap = sz;
    }
    return buf;
}

size_t RequestHandler::record_plan_(size_t &nplans) {
    hipEvent_t e = nullptr;
    {
        std::lock_guard<std::mutex> g(done_mu_);
        if (!free_events_.empty()) {
            e = free_events_.back();
            free_events_.pop_back();
        }
    }
    if (!e) DDL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    round_events_.push_back(e);
    DDL_HIP(hipEventRecord(e, stream_));
    return nplans++;
}

void RequestHandler::wait_inputs_(const Request &r, std::vector<hipEvent_t> &waited) {
    if (!r.ready || std::find(waited.begin(), waited.end(), r.ready->e) != waited.end()) return;
    DDL_HIP(hipStreamWaitEvent(stream_, r.ready->e, 0));
    waited.push_back(r.ready->e);
}

namespace {
// fn(src, dst, bytes) for the element slice of every request (reqs[group[q]]) inside plan p.
// What a request's plans and cuts count: its elements, or with the e4m3 wire its granules of 252.
size_t plan_units(const Request &r) { return r.wire == kDtypeE4m3 ? e4m3_granules(r.n) : r.n; }

template <class Fn>
void plan_slices(const Plan &p, const std::vector<Request> &reqs, const std::vector<size_t> &group, size_t es, Fn fn) {
    for (size_t q = p.req_begin; q <= p.req_end; ++q) {
        const Request &r = reqs[group[q]];
        const size_t b = q == p.req_begin ? p.elem_begin : 0, e = q == p.req_end ? p.elem_end : plan_units(r);
        if (r.wire == kDtypeE4m3) {  // granules b..e of an fp32 tensor: the tail is the request's, not the granule's
            const size_t e0 = b * kE4m3Elems, e1 = std::min(e * kE4m3Elems, r.n);
            fn(static_cast<const char *>(r.in) + e0 * sizeof(float), static_cast<char *>(r.out) + e0 * sizeof(float),
               (e1 - e0) * sizeof(float));
            continue;
        }
        fn(static_cast<const char *>(r.in) + b * es, static_cast<char *>(r.out) + b * es, (e - b) * es);
    }
}
// The op of every slice plan_slices visits, in its order: a request's SUM / AVG is rank-local and
// applied where its segment is written out; it never enters the group key or the plan cuts (the wire
// dtype of a compressed request, Request::wire, and MIN / MAX do: they are communicated).
std::vector<int> plan_ops(const Plan &p, const std::vector<Request> &reqs, const std::vector<size_t> &group) {
    std::vector<int> ops;
    for (size_t q = p.req_begin; q <= p.req_end; ++q) ops.push_back(reqs[group[q]].op);
    return ops;
}
}  // namespace

// Engine thread only. hipMalloc does not wait for the device (profiles/r06/s17); the zeroing is
// posted on stream_, so it runs after every earlier pack of this key and before the next one. A
// residual of another element count is retired, not freed: its last pack may still be running. A key that
// comes back under the other family of wire (e4m3 after a 16-bit wire, or the reverse) restarts from zero.
void *RequestHandler::residual_(const Request &r) {
    const long long epoch = config().wire_feedback_epoch.load();
    const int family = r.wire == kDtypeE4m3 ? kFamilyE4m3 : kFamily16;
    Residual &res = residuals_[r.key];
    if (res.ptr && res.n == r.n && res.epoch == epoch && res.family == family) return res.ptr;
    res.family = family;
    if (res.n != r.n) {
        if (res.ptr) retire_device(res.ptr);
        res.ptr = nullptr;
        res.n = 0;
        DDL_HIP(hipMalloc(&res.ptr, r.n * sizeof(float)));
        res.n = r.n;
    }
    res.epoch = epoch;
    DDL_HIP(hipMemsetAsync(res.ptr, 0, r.n * sizeof(float), stream_));
    return res.ptr;
}

uint64_t RequestHandler::stochastic_stream_(const Request &r) {
    const uint64_t n = stochastic_seq_[r.key]++;
    return stochastic_stream((uint64_t)config().wire_stochastic_seed.load(), (uint64_t)data_->rank(), r.key.data(),
                             r.key.size(), n);
}

double *RequestHandler::stat_take_(size_t n) {
    if (round_stat_blocks_.empty() || round_stat_blocks_.back().cap - round_stat_blocks_.back().used < n) {
        StatBlock b;
        {
            std::lock_guard<std::mutex> g(done_mu_);
            for (size_t k = 0; k < free_stat_.size() && !b.p; ++k)
                if (free_stat_[k].cap >= n) {
                    b = free_stat_[k];
                    free_stat_[k] = free_stat_.back();
                    free_stat_.pop_back();
                }
        }
        if (!b.p) {
            b.cap = std::max<size_t>(n, 4096);
            void *m = nullptr;
            DDL_HIP(hipHostMalloc(&m, b.cap * sizeof(double), hipHostMallocDefault));
            b.p = static_cast<double *>(m);
        }
        b.used = 0;
        round_stat_blocks_.push_back(b);
    }
    StatBlock &b = round_stat_blocks_.back();
    double *p = b.p + b.used;
    b.used += n;
    return p;
}

void RequestHandler::stat_in_place_(size_t req, void *out, size_t bytes, int dtype) {
    double *sq = stat_take_(1);
    CopySeg seg{out, bytes};
    seg.want = true;
    fp_.copier.run(CopyLaunch{SegmentCopier::kSumsqInPlace, nullptr, stream_, dtype, 0, 1, sq}, &seg, 1);
    round_stat_.emplace_back(req, sq);
}

void RequestHandler::scale_in_place_(void *out, size_t bytes, int dtype, int op, int divisor, float factor) {
    const CopySeg seg{out, bytes, op, factor};
    fp_.copier.run(CopyLaunch{SegmentCopier::kDivInPlace, nullptr, stream_, dtype, 0, divisor}, &seg, 1);
}

std::unique_lock<std::mutex> RequestHandler::lock_host_group_(const std::vector<Request> &reqs,
                                                              const std::vector<size_t> &group, size_t es, bool host) {
    if (!host) return {};
    std::unique_lock<std::mutex> rg = host_->registrations().lock();
    if (config().host_register_cache_bytes.load() > 0) {
        std::vector<std::pair<const void *, size_t>> ranges;  // pageable tensors used again and again
        for (size_t i : group) {
            ranges.emplace_back(reqs[i].in, reqs[i].n * es);
            if (reqs[i].out != reqs[i].in) ranges.emplace_back(reqs[i].out, reqs[i].n * es);
        }
        host_->registrations().ensure(ranges);  // registered once, kept
    }
    return rg;
}

void RequestHandler::finish_plan_(const Plan &p, const std::vector<Request> &reqs, const std::vector<size_t> &group,
                                  std::vector<Done> &dones, size_t &nplans) {
    const size_t plan = record_plan_(nplans);
    for (size_t q = p.req_begin; q <= p.req_end; ++q)
        if (q < p.req_end || p.elem_end == plan_units(reqs[group[q]])) dones.push_back(Done{plan, group[q], DDL_STATUS_OK});
}

// allreduceRequests (MPIRingTokenCommunication.cc:105-157): dtype groups in ascending enum order,
// ids lexicographic inside, plans capped at the fusion threshold.
void RequestHandler::allreduce_reqs_(std::vector<Request> &reqs, std::vector<Done> &dones, size_t &nplans) {
    // (wire dtype, compressed, host): dtype groups in ascending enum order; host-resident requests —
    // all of them in the reference, which only has CPU tensors — form their own groups after the
    // device ones. The wire dtype is the request's own dtype unless it is an fp32 request with a
    // wire flag (Request::wire), whose group comes right after the native group of that 16-bit
    // dtype — the same order on every rank, the wire being a property of the key. Groups of
    // uncompressed requests are formed and ordered as without the flag. The reduction kind (0 SUM /
    // AVG, 1 MIN, 2 MAX) is communicated too — it is what the plan's allreduce computes — so MIN and
    // MAX requests form groups of their own after the SUM / AVG group of the same dtype and memory;
    // a round without them forms exactly the groups it formed before. The e4m3 wire's internal dtype id is
    // above every ddl_dtype, so its group comes after all of these.
    auto kind_rank = [](int op) { return op == DDL_ALLREDUCE_OP_MIN ? 1 : op == DDL_ALLREDUCE_OP_MAX ? 2 : 0; };
    std::map<std::tuple<int, int, int, int>, std::vector<size_t>> groups;
    for (size_t i = 0; i < reqs.size(); ++i) {
        if (reqs[i].n == 0) dones.push_back(Done{kNoPlan, i, DDL_STATUS_OK});  // nothing to reduce
        else
            groups[std::make_tuple(reqs[i].wire ? reqs[i].wire : reqs[i].dtype, reqs[i].wire ? 1 : 0,
                                   reqs[i].host ? 1 : 0, kind_rank(reqs[i].op))]
                .push_back(i);
    }
    std::vector<hipEvent_t> waited;
    for (auto &g : groups) {
        const int dt = std::get<0>(g.first);  // what is communicated and summed
        const bool comp = std::get<1>(g.first) != 0;
        const bool host = std::get<2>(g.first) != 0;
        const int kind = reduce_kind(reqs[g.second[0]].op);  // of the whole group: SUM, MIN or MAX
        const int sdt = comp ? DDL_FLOAT : dt;  // what the tensors hold
        // plans, the fusion threshold and the message size count wire bytes (es); the tensors'
        // slices their own (ses)
        // (the e4m3 wire: es one granule, ses the 252 fp32 elements it carries, the plans in granules)
        const bool q8 = dt == kDtypeE4m3;
        const size_t es = dtype_size(dt), ses = q8 ? kE4m3Elems * sizeof(float) : dtype_size(sdt);
        std::vector<size_t> elems, esz;
        for (size_t i : g.second) {
            elems.push_back(plan_units(reqs[i]));
            esz.push_back(es);
        }
        const std::unique_lock<std::mutex> rg = lock_host_group_(reqs, g.second, es, host);
        // the group's requests as fusion segments (wire bytes), with what is rank-local like the op: the
        // factors, the sum of squares (taken by the unpack), and in a compressed group the residual of
        // error feedback (Request::feedback) and the stream key of stochastic rounding
        // (Request::stochastic) — found or made once per round, so all plans and pieces of a request share
        // them; none (and no sequence number spent) where the one-rank shortcut skips the data plane
        const bool fused = !host && !(data_->size() == 1 && config().one_rank_shortcut.load()), wire_opts = comp && fused;
        std::vector<PlanSeg> whole;
        whole.reserve(fused ? g.second.size() : 0);
        for (size_t q = 0; fused && q < g.second.size(); ++q) {
            const Request &r = reqs[g.second[q]];
            whole.push_back(PlanSeg{r.in, r.out, plan_units(r) * es, r.op, r.prescale, r.postscale});
            whole.back().want = r.sumsq != nullptr;
            if (q8) whole.back().elems = r.n;
            if (wire_opts && r.feedback) whole.back().residual = residual_(r);
            if (wire_opts && r.stochastic) whole.back().stream = WireStream{stochastic_stream_(r), 0, 1};
        }
        for (const Plan &p : make_plans(elems, esz, (size_t)config().fusion_threshold_bytes.load())) {
            for (size_t q = p.req_begin; q <= p.req_end; ++q) wait_inputs_(reqs[g.second[q]], waited);
            if (host) {
                // memcpy in -> MPI_Allreduce -> memcpy out (MPIRingTokenCommunication.cc:548-733),
                // the allreduce on the device through pinned chunks
                std::vector<HostSeg> segs;
                size_t message = 0;
                plan_slices(p, reqs, g.second, es, [&](const char *s, char *d, size_t n) {
                    segs.push_back(HostSeg{s, d, n});
                    message += n;
                });
                const std::vector<int> ops = plan_ops(p, reqs, g.second);
                for (size_t k = 0; k < segs.size(); ++k) segs[k].op = ops[k];
                if (data_->size() == 1 && config().one_rank_shortcut.load()) {
                    std::vector<CopyPool::Piece> pieces;
                    for (const HostSeg &sg : segs)
                        if (sg.src != sg.dst) pieces.push_back(CopyPool::Piece{sg.dst, sg.src, sg.bytes});
                    host_->pool().run(pieces);
                } else {
                    // chunks of the padded stream either way, so ranks that differ in which
                    // outputs are pinned still issue the same collectives
                    auto coll = [&](void *d, size_t elems) {
                        data_->allreduce(d, d, elems, dt, kind, stream_, message);
                    };
                    const auto t_check = std::chrono::steady_clock::now();
                    const bool mapped = config().host_zero_copy.load() && host_->mapped_dsts(segs);
                    const auto t_plan = std::chrono::steady_clock::now();
                    config().host_check_ns.fetch_add(
                        std::chrono::duration_cast<std::chrono::nanoseconds>(t_plan - t_check).count());
                    host_->run(segs, es, true, coll, true, mapped, dt, data_->size());
                    config().host_plan_ns.fetch_add(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                                        std::chrono::steady_clock::now() - t_plan)
                                                        .count());
                }
            } else if (data_->size() == 1 && config().one_rank_shortcut.load()) {
                // a one-rank world: the sum is the input; move bytes only where out != in (nothing
                // is communicated, so nothing is compressed either — and a sum of squares is taken in
                // the uncompressed order, in place)
                // the scale factors: (g (x) a) (x) b in one in-place launch behind the copy, each factor
                // skipped when it is 1 (two launches when both are present: two separately rounded products)
                size_t q = p.req_begin;
                plan_slices(p, reqs, g.second, q8 ? sizeof(float) : ses, [&](const char *s, char *d, size_t n) {
                    const Request &r = reqs[g.second[q]];
                    if (s != d && n) DDL_HIP(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, stream_));
                    if (n && r.prescale != 1.0f) scale_in_place_(d, n, sdt, DDL_ALLREDUCE_OP_SUM, 1, r.prescale);
                    if (n && r.postscale != 1.0f) scale_in_place_(d, n, sdt, DDL_ALLREDUCE_OP_SUM, 1, r.postscale);
                    if (reqs[g.second[q]].sumsq && n) stat_in_place_(g.second[q], d, n, sdt);
                    ++q;
                });
            } else if (p.req_begin == p.req_end && !comp) {
                const Request &r = reqs[g.second[p.req_begin]];
                const size_t cnt = p.elem_end - p.elem_begin;
                const char *src = static_cast<const char *>(r.in) + p.elem_begin * es;
                char *dst = static_cast<char *>(r.out) + p.elem_begin * es;
                // a prescale: the slice is moved to `out` (where out != in) and multiplied there by one
                // in-place launch; the allreduce then runs in place over exactly the elements it would
                // have reduced without the factor. NOT the fusion-buffer branch: its allreduce covers the
                // padded buffer, another element count, and the factors are rank-local — ranks that
                // disagree about a prescale must still post the same collective.
                if (r.prescale != 1.0f && cnt) {
                    if (src != dst) DDL_HIP(hipMemcpyAsync(dst, src, cnt * es, hipMemcpyDeviceToDevice, stream_));
                    scale_in_place_(dst, cnt * es, dt, DDL_ALLREDUCE_OP_SUM, 1, r.prescale);
                    src = dst;
                }
                // a postscale: the allreduce of the reduction kind alone, then ONE in-place launch that
                // takes AVG's quotient and the factor together
                const bool post = r.postscale != 1.0f;
                data_->allreduce(src, dst, cnt, dt, post ? kind : r.op, stream_);
                if (post && cnt)
                    scale_in_place_(static_cast<char *>(r.out) + p.elem_begin * es, cnt * es, dt, r.op, data_->size(), r.postscale);
                // no unpack to take it from: one read-only pass over the finished slice
                if (r.sumsq && cnt) stat_in_place_(g.second[p.req_begin], static_cast<char *>(r.out) + p.elem_begin * es, cnt * es, dt);
            } else {
                // a compressed plan always comes here, also with one request: the conversion is
                // the pack's and the unpack's, so the in-place direct path cannot apply.
                // The plan's slices of the requests: tensors, residuals and streams at the slice's first
                // element. A plan that fails after its pack has updated the residuals or has spent its
                // requests' sequence numbers: that is not undone.
                // (a plan of the whole group, the usual one, is run from the group's vector)
                const bool all = p.req_begin == 0 && p.elem_begin == 0 && p.req_end + 1 == whole.size() &&
                                 p.elem_end == plan_units(reqs[g.second[p.req_end]]);
                std::vector<PlanSeg> slices;
                slices.reserve(all ? 0 : p.req_end - p.req_begin + 1);
                for (size_t q = p.req_begin; q <= p.req_end && !all; ++q) {
                    const size_t b = q == p.req_begin ? p.elem_begin : 0, e = q == p.req_end ? p.elem_end : plan_units(reqs[g.second[q]]);
                    slices.push_back(whole[q].piece(b * es, (e - b) * es, es, ses));
                }
                const std::vector<PlanSeg> &segs = all ? whole : slices;
                PlanSumsq ps;
                ps.pinned = [this](size_t n) { return stat_take_(n); };
                fp_.run(segs, dt, sdt, (size_t)config().fusion_pipeline_bytes.load(), data_->size(), stream_,
                        [&](void *buf, size_t elems, size_t message) {
                            data_->allreduce(buf, buf, elems, dt, kind, stream_, message);
                        },
                        &ps);
                for (const PlanSumsq::Piece &pc : ps.pieces) round_stat_.emplace_back(g.second[p.req_begin + pc.seg], pc.value);
            }
            finish_plan_(p, reqs, g.second, dones, nplans);
        }
    }
}

// broadcastRequests (MPIRingTokenCommunication.cc:367-419): dtype groups, plans, broadcast of
// the packed plan from the root. The reference broadcasts every group from the first request's
// root; requests are grouped by (dtype, root) here so mixed roots stay correct.
void RequestHandler::broadcast_reqs_(std::vector<Request> &reqs, std::vector<Done> &dones, size_t &nplans) {
    std::map<std::tuple<int, int, int>, std::vector<size_t>> groups;  // (dtype, root, host)
    for (size_t i = 0; i < reqs.size(); ++i) {
        if (reqs[i].n == 0) dones.push_back(Done{kNoPlan, i, DDL_STATUS_OK});
        else groups[std::make_tuple(reqs[i].dtype, reqs[i].root, reqs[i].host ? 1 : 0)].push_back(i);
    }
    const int me = data_->rank();
    std::vector<hipEvent_t> waited;
    for (auto &g : groups) {
        const int dt = std::get<0>(g.first), root = std::get<1>(g.first);
        const bool host = std::get<2>(g.first) != 0;
        const size_t es = dtype_size(dt);
        std::vector<size_t> elems, esz;
        for (size_t i : g.second) {
            elems.push_back(reqs[i].n);
            esz.push_back(es);
        }
        const std::unique_lock<std::mutex> rg = lock_host_group_(reqs, g.second, es, host);
        for (const Plan &p : make_plans(elems, esz, (size_t)config().fusion_threshold_bytes.load())) {
            for (size_t q = p.req_begin; q <= p.req_end; ++q) wait_inputs_(reqs[g.second[q]], waited);
            if (host) {
                // root: pack in -> H2D -> broadcast -> D2H -> unpack to out; others only receive
                std::vector<HostSeg> segs;
                plan_slices(p, reqs, g.second, es,
                            [&](const char *s, char *d, size_t n) { segs.push_back(HostSeg{s, d, n}); });
                host_->run(segs, es, me == root,
                           [&](void *d, size_t elems) { data_->broadcast(d, elems, dt, root, stream_); });
            } else if (p.req_begin == p.req_end) {
                const Request &r = reqs[g.second[p.req_begin]];
                const size_t cnt = p.elem_end - p.elem_begin;
                char *out = static_cast<char *>(r.out) + p.elem_begin * es;
                if (me == root && r.in != r.out)
                    DDL_HIP(hipMemcpyAsync(out, static_cast<const char *>(r.in) + p.elem_begin * es, cnt * es,
                                           hipMemcpyDeviceToDevice, stream_));
                data_->broadcast(out, cnt, dt, root, stream_);
            } else {
                std::vector<const void *> srcs;
                std::vector<void *> dsts;
                std::vector<size_t> bytes;
                plan_slices(p, reqs, g.second, es, [&](const char *s, char *d, size_t n) {
                    srcs.push_back(s);
                    dsts.push_back(d);
                    bytes.push_back(n);
                });
                const size_t total = SegmentCopier::flat_bytes(bytes.data(), (int)bytes.size());
                void *fb = fp_.ensure(0, total, stream_);
                if (me == root)
                    fp_.copier.copy(0, fb, const_cast<void *const *>(srcs.data()), bytes.data(), (int)srcs.size(),
                                    stream_);
                data_->broadcast(fb, total / es, dt, root, stream_);
                fp_.copier.copy(1, fb, dsts.data(), bytes.data(), (int)dsts.size(), stream_);
            }
            finish_plan_(p, reqs, g.second, dones, nplans);
        }
    }
}

// allgatherRequests (MPIRingTokenCommunication.cc:160-364), per dtype group: allgather every
// rank's first dims (u64), allocate each output (first dim = sum over ranks), then one
// allgatherv of the packed requests and an unpack into the outputs in rank order. A single
// request gathers straight into its output (rank-major blocks are the concatenation).
void RequestHandler::allgather_reqs_(std::vector<Request> &reqs, std::vector<Done> &dones, size_t &nplans) {
    std::map<std::pair<int, int>, std::vector<size_t>> groups;  // (dtype, host)
    for (size_t i = 0; i < reqs.size(); ++i) groups[std::make_pair(reqs[i].dtype, reqs[i].host ? 1 : 0)].push_back(i);
    const int P = data_->size(), me = data_->rank();
    std::vector<hipEvent_t> waited;
    for (auto &g : groups) {
        const int dt = g.first.first;
        const bool host = g.first.second != 0;
        const size_t es = dtype_size(dt), m = g.second.size();
        // 1) first dims of every rank: fd[q * m + j]
        std::vector<uint64_t> fd(P * m);
        for (size_t j = 0; j < m; ++j) fd[me * m + j] = reqs[g.second[j]].first_dim;
        if (P > 1) {
            ensure_(dims_, dims_bytes_, fd.size() * 8);
            std::vector<size_t> cnt(P, m), dsp(P);
            for (int q = 0; q < P; ++q) dsp[q] = q * m;
            DDL_HIP(hipMemcpyAsync(static_cast<char *>(dims_) + me * m * 8, fd.data() + me * m, m * 8,
                                   hipMemcpyHostToDevice, stream_));
            data_->allgatherv(static_cast<char *>(dims_) + me * m * 8, dims_, cnt.data(), dsp.data(), DDL_UINT64,
                              stream_);
            DDL_HIP(hipMemcpyAsync(fd.data(), dims_, fd.size() * 8, hipMemcpyDeviceToHost, stream_));
            DDL_HIP(hipStreamSynchronize(stream_));
        }
        // 2) outputs
        std::vector<size_t> total_rows(m, 0);
        for (size_t j = 0; j < m; ++j) {
            Request &r = reqs[g.second[j]];
            for (int q = 0; q < P; ++q) total_rows[j] += fd[q * m + j];
            const size_t bytes = total_rows[j] * r.row_elems * es;
            r.out = r.alloc(total_rows[j], bytes, r.user);
            DDL_REQUIRE(bytes == 0 || r.out, DDL_STATUS_ERROR_UNKNOWN, "allgather output allocation failed for '" << r.key << "'");
        }
        for (size_t j = 0; j < m; ++j) wait_inputs_(reqs[g.second[j]], waited);
        // 3) data
        if (host) {
            // host tensors: this rank's rows packed back to back through a pinned buffer, one
            // allgatherv on the device, then every rank's rows unpacked into the host outputs
            std::vector<size_t> blk(P, 0);
            for (int q = 0; q < P; ++q)
                for (size_t j = 0; j < m; ++j) blk[q] += fd[q * m + j] * reqs[g.second[j]].row_elems * es;
            size_t all = 0;
            std::vector<size_t> cnt(P), dsp(P);
            for (int q = 0; q < P; ++q) {
                cnt[q] = blk[q] / es;
                dsp[q] = all / es;
                all += blk[q];
            }
            if (all) {
                void *fb = fp_.ensure(0, std::max<size_t>(blk[me], 256), stream_);
                ensure_(gather_, gather_bytes_, all);
                char *pin = static_cast<char *>(host_->gather_buffer(all));
                size_t off = 0;
                for (size_t j = 0; j < m; ++j) {
                    const Request &r = reqs[g.second[j]];
                    const size_t b = fd[me * m + j] * r.row_elems * es;
                    std::memcpy(pin + off, r.in, b);
                    off += b;
                }
                DDL_HIP(hipMemcpyAsync(fb, pin, blk[me], hipMemcpyHostToDevice, stream_));
                data_->allgatherv(fb, gather_, cnt.data(), dsp.data(), dt, stream_);
                DDL_HIP(hipMemcpyAsync(pin, gather_, all, hipMemcpyDeviceToHost, stream_));
                DDL_HIP(hipStreamSynchronize(stream_));
                std::vector<size_t> row_off(m, 0);
                off = 0;
                for (int q = 0; q < P; ++q)
                    for (size_t j = 0; j < m; ++j) {
                        const Request &r = reqs[g.second[j]];
                        const size_t b = fd[q * m + j] * r.row_elems * es;
                        std::memcpy(static_cast<char *>(r.out) + row_off[j] * r.row_elems * es, pin + off, b);
                        row_off[j] += fd[q * m + j];
                        off += b;
                    }
            }
        } else if (m == 1) {
            const Request &r = reqs[g.second[0]];
            std::vector<size_t> cnt(P), dsp(P);
            size_t acc = 0;
            for (int q = 0; q < P; ++q) {
                cnt[q] = fd[q] * r.row_elems;
                dsp[q] = acc;
                acc += cnt[q];
            }
            if (acc) data_->allgatherv(r.in, r.out, cnt.data(), dsp.data(), dt, stream_);
        } else {
            // rank q's block: its m requests, each 256-byte aligned (the copier's flat layout)
            std::vector<size_t> blk(P, 0);
            std::vector<size_t> seg_bytes(P * m);
            for (int q = 0; q < P; ++q)
                for (size_t j = 0; j < m; ++j) {
                    seg_bytes[q * m + j] = fd[q * m + j] * reqs[g.second[j]].row_elems * es;
                    blk[q] += (seg_bytes[q * m + j] + 255) & ~size_t(255);
                }
            size_t all = 0;
            std::vector<size_t> cnt(P), dsp(P);
            for (int q = 0; q < P; ++q) {
                cnt[q] = blk[q] / es;
                dsp[q] = all / es;
                all += blk[q];
            }
            if (all) {
                void *fb = fp_.ensure(0, std::max<size_t>(blk[me], 256), stream_);
                ensure_(gather_, gather_bytes_, all);
                std::vector<const void *> srcs(m);
                for (size_t j = 0; j < m; ++j) srcs[j] = reqs[g.second[j]].in;
                fp_.copier.copy(0, fb, const_cast<void *const *>(srcs.data()), seg_bytes.data() + me * m, (int)m,
                                stream_);
                data_->allgatherv(fb, gather_, cnt.data(), dsp.data(), dt, stream_);
                std::vector<void *> dsts(P * m);
                std::vector<size_t> row_off(m, 0);  // rows of request j written so far
                for (int q = 0; q < P; ++q)
                    for (size_t j = 0; j < m; ++j) {
                        const Request &r = reqs[g.second[j]];
                        dsts[q * m + j] = static_cast<char *>(r.out) + row_off[j] * r.row_elems * es;
                        row_off[j] += fd[q * m + j];
                    }
                fp_.copier.copy(1, gather_, dsts.data(), seg_bytes.data(), (int)(P * m), stream_);
            }
        }
        const size_t plan = record_plan_(nplans);
        for (size_t j = 0; j < m; ++j) dones.push_back(Done{plan, g.second[j], DDL_STATUS_OK});
    }
}

void RequestHandler::execute_(const std::vector<ReqId> &ids, int forced) {
    if (ids.empty()) return;
    // phase times of the round at log level 2 (take / enqueue / wait + done, microseconds)
    using clk = std::chrono::steady_clock;
    const bool timed = log_level() >= 2;
    const clk::time_point t0 = timed ? clk::now() : clk::time_point();
    std::vector<Request> reqs;
    reqs.reserve(ids.size());
    {
        std::lock_guard<std::mutex> g(mu_);
        // the agreed ids come in (type, key) order, the pending map's order: one forward walk
        // (a compare or two per id) instead of a lookup per id
        const bool sorted = std::is_sorted(ids.begin(), ids.end());
        auto it = sorted ? pending_.lower_bound(ids.front()) : pending_.end();
        for (const auto &k : ids) {
            if (sorted) {
                while (it != pending_.end() && it->first < k) ++it;
            } else {
                it = pending_.find(k);
            }
            DDL_REQUIRE(it != pending_.end() && !(k < it->first), DDL_STATUS_COMM_ERROR,
                        "agreed request '" << k.key << "' is not registered");
            if (it->second.cidx >= 0) pend_flag_[it->second.cidx] = 0;
            reqs.push_back(std::move(it->second));
            it = pending_.erase(it);
        }
        inflight_ += reqs.size();
    }
    std::vector<Done> dones;
    size_t nplans = 0;
    int status = forced;
    const clk::time_point t1 = timed ? clk::now() : clk::time_point();
    round_events_.clear();
    round_stat_.clear();
    round_stat_blocks_.clear();
    if (forced == DDL_STATUS_OK) try {
        for (const Request &r : reqs)
            DDL_REQUIRE(r.type == reqs[0].type, DDL_STATUS_COMM_ERROR, "agreed requests of mixed types");
        switch (reqs[0].type) {
            case kReqAllreduce: allreduce_reqs_(reqs, dones, nplans); break;
            case kReqBroadcast: broadcast_reqs_(reqs, dones, nplans); break;
            case kReqAllgather: allgather_reqs_(reqs, dones, nplans); break;
            default: fail(DDL_STATUS_ERROR_UNKNOWN, "unknown request type");
        }
    } catch (const Error &e) {
        DDL_LOG(0, "collective of agreed requests failed: " << e.msg);
        status = e.status;
    }
    Round rd;
    rd.reqs = std::move(reqs);
    rd.dones = std::move(dones);
    rd.events.swap(round_events_);
    rd.stat.swap(round_stat_);
    rd.stat_blocks.swap(round_stat_blocks_);
    rd.status = status;
    rd.nplans = nplans;
    rd.t0 = t0;
    rd.t1 = t1;
    if (timed) rd.t2 = clk::now();
    const bool pipelined = config().pipeline_rounds.load() != 0;
    size_t bytes = 0;
    for (const Request &r : rd.reqs) bytes += r.n * dtype_size(r.dtype);
    bool idle;
    {
        std::lock_guard<std::mutex> g(done_mu_);
        idle = rounds_queued_ == rounds_done_;  // no earlier round waiting or completing
    }
    // nothing earlier in flight and the round is to be waited for anyway (unpipelined, failed)
    // or small (its data plane takes microseconds): complete it here — done() order holds and
    // the hand-off to the completion thread (a thread wake-up each way) is saved
    if (idle && (!pipelined || status != DDL_STATUS_OK || bytes <= kInlineRoundBytes)) {
        complete_(rd);
        if (status != DDL_STATUS_OK && status != forced) fail(status, "keyed collective failed");
        return;
    }
    unsigned long long seq;
    {
        std::lock_guard<std::mutex> g(done_mu_);
        rounds_.push_back(std::move(rd));
        seq = ++rounds_queued_;
    }
    done_cv_.notify_all();
    // pipelined: back to negotiating while the device runs this round; otherwise (and after a
    // failed enqueue, whose done() calls must have fired before the handler stops) wait for it
    if (status != DDL_STATUS_OK || !pipelined) {
        std::unique_lock<std::mutex> lk(done_mu_);
        done_cv_.wait(lk, [&] { return rounds_done_ >= seq; });
    }
    if (status != DDL_STATUS_OK && status != forced) fail(status, "keyed collective failed");
}

// done() in plan order as each request's last element lands (MPIRTC.cc:593-597, 690-725).
void RequestHandler::complete_(Round &rd) {
    using clk = std::chrono::steady_clock;
    int status = rd.status;
    std::vector<char> fired(rd.reqs.size(), 0);
    size_t synced = kNoPlan;  // dones are in plan order: wait for each plan's event once
    // a request's sum of squares: its pieces' values added in increasing element offset, from the
    // first piece's value (+0.0 without a piece). The values were copied to pinned memory on the
    // plans' streams ahead of the plan events waited for below, the last piece's plan last.
    std::vector<std::vector<const double *>> pieces;
    if (!rd.stat.empty()) {
        pieces.resize(rd.reqs.size());
        for (const auto &sp : rd.stat) pieces[sp.first].push_back(sp.second);
    }
    auto write_sumsq = [&](size_t req) {
        const Request &r = rd.reqs[req];
        if (!r.sumsq) return;
        double v = 0.0;
        if (req < pieces.size())
            for (size_t k = 0; k < pieces[req].size(); ++k) v = k == 0 ? *pieces[req][k] : v + *pieces[req][k];
        *r.sumsq = v;
    };
    for (const Done &d : rd.dones) {
        if (status == DDL_STATUS_OK && d.plan != kNoPlan && d.plan != synced) {
            hipError_t he = wait_plan(rd.events[d.plan]);
            if (he != hipSuccess) status = DDL_STATUS_HIP_ERROR;
            synced = d.plan;
        }
        const Request &r = rd.reqs[d.req];
        fired[d.req] = 1;
        if (status == DDL_STATUS_OK) write_sumsq(d.req);
        if (r.done) r.done(status == DDL_STATUS_OK ? d.status : status, r.user);
    }
    for (size_t i = 0; i < rd.reqs.size(); ++i)
        if (!fired[i] && rd.reqs[i].done)
            rd.reqs[i].done(status == DDL_STATUS_OK ? DDL_STATUS_ERROR_UNKNOWN : status, rd.reqs[i].user);
    if (status == DDL_STATUS_OK) {  // waited for: safe to record again
        std::lock_guard<std::mutex> g(done_mu_);
        free_events_.insert(free_events_.end(), rd.events.begin(), rd.events.end());
        free_stat_.insert(free_stat_.end(), rd.stat_blocks.begin(), rd.stat_blocks.end());
    } else {
        for (hipEvent_t e : rd.events) (void)hipEventDestroy(e);
        for (StatBlock &b : rd.stat_blocks) retire_host(b.p);  // a copy into it may still be pending
        if (rd.status == DDL_STATUS_OK) {  // a device failure the engine thread has not seen
            {
                std::lock_guard<std::mutex> g(mu_);
                int expected = 0;
                failed_.compare_exchange_strong(expected, status);
            }
            cv_.notify_all();
        }
    }
    rd.events.clear();
    rd.stat.clear();
    rd.stat_blocks.clear();
    const size_t n = rd.reqs.size();
    rd.reqs.clear();  // the requests' input-ready events go with them
    {
        std::lock_guard<std::mutex> g(mu_);
        inflight_ -= n;
    }
    idle_cv_.notify_all();
    if (log_level() >= 2 && rd.t0 != clk::time_point()) {
        auto us = [](clk::time_point a, clk::time_point b) {
            return std::chrono::duration_cast<std::chrono::microseconds>(b - a).count();
        };
        DDL_LOG(2, "round: " << n << " requests, " << rd.nplans << " plans; take " << us(rd.t0, rd.t1) << " us, enqueue "
                             << us(rd.t1, rd.t2) << " us, wait + done " << us(rd.t2, clk::now()) << " us");
    }
}

void RequestHandler::completer_() {
    t_handler_thread = true;  // done() callbacks run here (engine.h)
    (void)hipSetDevice(owner_->device());
    for (;;) {
        Round rd;
        {
            std::unique_lock<std::mutex> lk(done_mu_);
            done_cv_.wait(lk, [this] { return done_stop_ || !rounds_.empty(); });
            if (rounds_.empty()) break;  // stopping, and every handed-over round has completed
            rd = std::move(rounds_.front());
            rounds_.pop_front();
        }
        complete_(rd);
        {
            std::lock_guard<std::mutex> g(done_mu_);
            ++rounds_done_;
        }
        done_cv_.notify_all();
    }
}

}  // namespace ddl
