// handler.h — keyed asynchronous collective requests (allreduce, broadcast, allgather) with
// cross-rank negotiation and fusion.
//
// Replaces the reference's request path below the TF op:
//   TensorAllreduceRequest (collective/request/TensorAllreduceRequest.h:13-41)
//   RingTokenCommunicateHandler (controller/rtc/RingTokenCommunicateHandler.cc:13-410):
//     per-communicator background thread, ring-token negotiation of which keys every rank
//     has registered, communication of the agreed set in lexicographic (type, key) order;
//   MPIRingTokenCommunication::allreduceRequests (rtc/mpi/MPIRingTokenCommunication.cc:105-157,
//     495-749): dtype classification (ascending enum), plans capped at the fusion threshold,
//     memcpy in -> MPI_Allreduce -> memcpy out, done() as each tensor's last element lands.
//
// MI355X-first changes: a round is 3 hops over a star around rank 0 instead of 3 laps of a ring
// (READY+SYNC merged: a member answers the proposal once it has the proposal's first key, with
// its intersection; rank 0 intersects the answers and announces the result); one-request plans
// run the ring directly on the tensor (no staging copy); multi-request plans are packed by
// one gather kernel into an HBM fusion buffer and scattered by one kernel; the data plane
// runs on a private RCCL communicator so user-level ddl_allreduce calls never interleave.
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory_resource>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "engine.h"
#include "fusion.h"
#include "host_stage.h"
#include "negotiate.h"

namespace ddl {

// Input-ready event recorded on the submitter's stream; shared by the requests of one batch.
struct ReadyEvent {
    hipEvent_t e = nullptr;
    explicit ReadyEvent(hipStream_t s);
    ~ReadyEvent();
    ReadyEvent(const ReadyEvent &) = delete;
    ReadyEvent &operator=(const ReadyEvent &) = delete;
};

struct Request {
    int type = kReqAllreduce;
    std::string key;
    const void *in = nullptr;
    void *out = nullptr;
    size_t n = 0;  // elements of `in`
    int dtype = 0;
    int op = 0;                       // allreduce: SUM / AVG / MIN / MAX (the wire flag decoded into `wire`)
    int wire = 0;                     // allreduce: wire dtype of a compressed fp32 request (0: its own dtype)
    bool feedback = false;            // allreduce: DDL_ALLREDUCE_WIRE_FEEDBACK, or with the e4m3 `wire` _E4M3_FEEDBACK (rank-local)
    bool stochastic = false;          // allreduce: DDL_ALLREDUCE_WIRE_STOCHASTIC (only with the bf16 `wire`; rank-local)
    double *sumsq = nullptr;          // allreduce: where the sum of squares of `out` goes before done() (host; rank-local)
    // allreduce: DDL_ALLREDUCE_SCALE's factors (1 = absent; fp32 device SUM / AVG requests). Rank-local like
    // the op and `sumsq`: in no group key, plan cut, pipeline cut or negotiation.
    float prescale = 1.0f;            //   every element times this on its way into the reduction
    float postscale = 1.0f;           //   every result (behind AVG's quotient) times this on its way into `out`
    int root = 0;                     // broadcast: TensorBroadcastRequest::rootRank()
    size_t first_dim = 0;             // allgather: rows of `in` (n = first_dim * row_elems)
    size_t row_elems = 1;             //   elements per row (the shape without its first dim)
    ddl_alloc_fn alloc = nullptr;     //   output allocation once the gathered first dim is known
    bool host = false;                // in / out are host memory (the reference's CPU tensors)
    int64_t cidx = -1;                // index in the control channel's id table, once agreed before
    std::shared_ptr<ReadyEvent> ready;
    ddl_done_fn done = nullptr;
    void *user = nullptr;
};

ReqId req_id(const Request &r);

struct Plan {  // makeCollectiveCommunicatePlan's (requestBegin, elementBegin, requestEnd, elementEnd)
    size_t req_begin, elem_begin, req_end, elem_end;
};

// Plans over requests (in order) capped at `limit` bytes. Same walk as the reference
// (MPIRingTokenCommunication.cc:495-546) except that a plan ending exactly on a request
// boundary advances to requestEnd + 1 (the reference advances requestBegin by one, which
// re-plans requests when a multi-request plan ends on a boundary; unreachable with its odd
// 2^31-1 cap and even element sizes, reachable with a configurable cap).
std::vector<Plan> make_plans(const std::vector<size_t> &elements, const std::vector<size_t> &esize,
                             size_t limit);

class RequestHandler {
public:
    explicit RequestHandler(Communicator *owner);
    ~RequestHandler();
    hipStream_t stream() const { return stream_; }  // the engine thread's (pack / unpack)

    void submit(Request r);
    // the host registration cache (host_stage.h HostRegistrations), from the user's threads
    void release_registrations() { host_->registrations().release_all(); }
    void unregister_range(const void *ptr, size_t bytes) { host_->registrations().unregister_range(ptr, bytes); }
    // All-or-nothing registration of several requests under one lock (one wake-up).
    void submit_batch(std::vector<Request> &rs);
    void wait_all();

private:
    void main_();
    void root_round_();
    void member_round_(Token &first);
    // Runs the agreed requests; `forced` != OK takes them out and fails them with that status
    // (a round whose ranks' shared tunables differ) without stopping the handler.
    void execute_(const std::vector<ReqId> &ids, int forced = DDL_STATUS_OK);
    // root_round_ / member_round_ after the agreement: places the round among the user collectives
    // (Communicator::round_release / round_enter), executes it, lifts the freeze
    void run_agreed_(const Agreed &a);
    std::vector<ReqId> agreed_ids_(const Agreed &a);  // learns new ids (string rounds)
    void forget_ids_();                                 // the id table was cleared
    void mark_cached_(const ReqId &id, Request &r);
    // Pinned host memory for the piece values of the sums of squares (DDL_ALLREDUCE_SUMSQ): the
    // engine thread hands out doubles of the round it is enqueuing (stat_take_), the round carries its
    // blocks to the completion, which returns them to free_stat_ (done_mu_) once the round's events
    // have been waited for. No allocation in steady state; blocks are freed with the handler.
    struct StatBlock {
        double *p = nullptr;
        size_t cap = 0, used = 0;
    };
    double *stat_take_(size_t n);
    // the in-place, read-only sum of squares (SegmentCopier::kSumsqInPlace) of reqs[req]'s slice on stream_
    void stat_in_place_(size_t req, void *out, size_t bytes, int dtype);
    // one in-place launch of the scaled scatter on stream_ over a finished fp32 slice: AVG's quotient by
    // `divisor` where `op` is AVG, then `factor` (SegmentCopier::kDivInPlace with a factor)
    void scale_in_place_(void *out, size_t bytes, int dtype, int op, int divisor, float factor);
    struct Done {
        size_t plan;  // index into the round's plan events (kNoPlan: nothing to wait for)
        size_t req;
        int status;
    };
    static constexpr size_t kNoPlan = (size_t)-1;
    // One executed round: its requests, their done() order, the plan events they wait for.
    // The engine thread enqueues the round's data plane and hands it to the completion thread,
    // which waits for each plan's event and fires done() in plan order, rounds in FIFO order;
    // meanwhile the engine thread negotiates the next round (pipeline_rounds = 1). The
    // reference's recv thread blocks in MPI_Allreduce instead (MPIRingTokenCommunication.cc:
    // 548-733); pipeline_rounds = 0 waits the same way.
    struct Round {
        std::vector<Request> reqs;
        std::vector<Done> dones;
        std::vector<hipEvent_t> events;
        // the sums of squares asked for: (request, its piece's value in pinned memory), a request's
        // pieces in increasing element offset; the pinned blocks the values live in
        std::vector<std::pair<size_t, const double *>> stat;
        std::vector<StatBlock> stat_blocks;
        int status = 0;
        size_t nplans = 0;
        std::chrono::steady_clock::time_point t0, t1, t2;  // take / enqueue phase bounds (log)
    };
    // a round of at most this many bytes, with no earlier round in flight, completes on the
    // engine thread even when pipelined (its data plane is microseconds: the hand-off costs more)
    static constexpr size_t kInlineRoundBytes = 256u << 10;
    size_t record_plan_(size_t &nplans);  // records the round's next plan event on stream_
    void complete_(Round &rd);            // waits the plan events, fires done(), frees the events
    void completer_();                    // the completion thread
    void wait_inputs_(const Request &r, std::vector<hipEvent_t> &waited);
    void *ensure_(void *&buf, size_t &cap, size_t need);
    // A host group (`host`) holds the registration lock while its plans are posted; with the
    // cache on, its tensors (reqs[i] for i in `group`) are registered first. Not held otherwise.
    std::unique_lock<std::mutex> lock_host_group_(const std::vector<Request> &reqs, const std::vector<size_t> &group,
                                                  size_t es, bool host);
    // Records plan p's event; done() is due for every request of `group` whose last element it carries.
    void finish_plan_(const Plan &p, const std::vector<Request> &reqs, const std::vector<size_t> &group,
                      std::vector<Done> &dones, size_t &nplans);
    void allreduce_reqs_(std::vector<Request> &reqs, std::vector<Done> &dones, size_t &nplans);
    void broadcast_reqs_(std::vector<Request> &reqs, std::vector<Done> &dones, size_t &nplans);
    void allgather_reqs_(std::vector<Request> &reqs, std::vector<Done> &dones, size_t &nplans);
    void fail_all_(int status);

    Communicator *owner_;
    ControlChannel *ch_ = nullptr;        // the owner's token ring (size > 1)
    // the data plane: the owner's private keyed communicator at size > 1, the owner itself at
    // size 1. Not owning: the owner holds keyed_data_ and destroys this handler first; an owning
    // pointer to the owner was a cycle that kept a detached size-1 split (and these threads) alive
    Communicator *data_ = nullptr;
    hipStream_t stream_ = nullptr;
    // multi-request plans: pack -> allreduce -> unpack, pipelined in sub-plans above
    // fusion_pipeline_bytes (fusion.h); its buffer 0 also packs broadcast / allgather plans
    FusionPipe fp_;
    // Error feedback (DDL_ALLREDUCE_WIRE_FEEDBACK, DDL_ALLREDUCE_WIRE_E4M3_FEEDBACK): what the wire's rounding removed from this rank's
    // contribution to a key, added back at the key's next request. One fp32 array per key that ever
    // asked for feedback, owned here and freed with the handler (a replaced one is retired, never
    // freed on a data path). Touched by the engine thread only (allreduce_reqs_ posts the packs).
    struct Residual {
        void *ptr = nullptr;
        size_t n = 0;         // elements
        long long epoch = 0;  // config wire_feedback_epoch when it was last (re)started
        int family = 0;       // kFamily16 (fp16 and bf16 share it) or kFamilyE4m3: the rule that last wrote it
    };
    static constexpr int kFamily16 = 1, kFamilyE4m3 = 2;
    std::unordered_map<std::string, Residual> residuals_;
    // the residual of request r for a pack posted on stream_: made, or restarted from zero (another
    // element count, another epoch, the other family of wire), by work posted on stream_ ahead of that pack
    void *residual_(const Request &r);
    // Stochastic rounding (DDL_ALLREDUCE_WIRE_STOCHASTIC): a key's sequence number n — how many requests of
    // the key with the bit this handler has packed before — one of the four things a request's stream key S
    // is mixed from (ddl_amd.h). One entry per key that ever carried the bit, kept until the handler goes.
    // Touched by the engine thread only.
    std::unordered_map<std::string, uint64_t> stochastic_seq_;
    // the stream key of request r's next pack; advances the key's sequence number
    uint64_t stochastic_stream_(const Request &r);
    // host-resident requests: made once stream_ exists, destroyed (both threads joined) before it
    std::unique_ptr<HostStager> host_;
    void *gather_ = nullptr;  // allgather receive side
    size_t gather_bytes_ = 0;
    void *dims_ = nullptr;    // allgather first-dim exchange
    size_t dims_bytes_ = 0;
    std::vector<hipEvent_t> round_events_;  // plan events of the round being enqueued (engine thread)
    std::vector<std::pair<size_t, const double *>> round_stat_;  // and its sums of squares (Round::stat)
    std::vector<StatBlock> round_stat_blocks_;

    std::mutex mu_;
    std::condition_variable cv_;       // new registrations / stop
    std::condition_variable idle_cv_;  // completions
    // the pending map's nodes come from a pool, allocated and freed under mu_ only: a 4096-request
    // batch's sorted inserts and its take walk ran 2-3x faster than with the process heap
    // (CPU micro-benchmark; r05 s22 on the box)
    std::pmr::unsynchronized_pool_resource pending_mem_;
    std::pmr::map<ReqId, Request> pending_{&pending_mem_};  // (type name, key) order
    // id table mirror (indices of the ring's cache): parsed ids, key -> index per type,
    // and which indices are pending here — a cached round is intersected by index
    std::vector<ReqId> cache_req_;
    std::unordered_map<std::string, uint32_t> cache_by_key_[3];
    std::vector<uint8_t> pend_flag_;
    size_t inflight_ = 0;
    bool stop_ = false;
    std::atomic<int> failed_{0};  // a completion failed: the engine thread stops with this status
    std::thread thread_;
    // completion thread state (done_mu_): executed rounds waiting for their events, free plan
    // events (returned once waited for, so none is re-recorded while still pending)
    std::mutex done_mu_;
    std::condition_variable done_cv_;
    std::deque<Round> rounds_;
    std::vector<hipEvent_t> free_events_;
    std::vector<StatBlock> free_stat_;
    unsigned long long rounds_queued_ = 0, rounds_done_ = 0;
    bool done_stop_ = false;
    std::thread done_thread_;
};

// Test hook (ddl_testing_control_fault): the next keyed round a member joins closes that member's
// control link right after its snapshot froze the user collectives (a link lost mid-round).
void set_testing_control_fault(int on);

}  // namespace ddl
