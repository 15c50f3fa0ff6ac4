// fusion.h — the data plane of one multi-request fusion plan: pack -> allreduce -> unpack.
//
// The reference copies every request of a plan into one MPI buffer, reduces it and copies it back
// (executeCommunicatePlan_, MPIRingTokenCommunication.cc:548-733). Here the copies are the pack /
// unpack kernels (SegmentCopier, pack.hip), and a plan above `cap` bytes (config
// fusion_pipeline_bytes) is cut into sub-plans J of at most that size (segments split at 256-byte
// multiples) over two fusion buffers:
//   side:    pack 0, pack 1, unpack 0, pack 2, unpack 1, ...   (unpack j waits allreduce j)
//   stream:          ar 0,   ar 1,     ar 2, ...               (ar j waits pack j)
// so the pack of j+1 and the unpack of j-1 run under the allreduce of j. Buffer j%2 is reused by
// pack j+2, issued on `side` after unpack j. Each sub-plan is an allreduce of its own; it is told
// the whole plan's message size, so with reference_order every sub-plan folds in the order MPICH
// uses for the whole plan and the cut changes no bit.
// A compressed plan (fp32 tensors over an fp16 / bf16 wire, ddl_allreduce_wire) is the same
// pipeline over the wire stream: the converting pack / unpack kernels, cuts at 256-byte multiples
// of the wire bytes (a tensor's offset is twice the wire offset), the allreduce in the wire dtype.
//
// One FusionPipe per engine thread: the keyed handler owns one (handler.cpp) and the thread world
// one per virtual rank (executor.cpp, ddl_testing_thread_fused_allreduce), so the same code runs
// under the production executor on one GPU.
#pragma once

#include <functional>
#include <vector>

#include "common.h"

namespace ddl {

// The sums of squares of a plan's results (DDL_ALLREDUCE_SUMSQ). A segment is cut into pieces by
// the sub-plans (tiles restart at every piece); every piece's value — the canonical sum of
// include/ddl_amd.h over the piece — lands in pinned host memory by an async copy behind the unpack
// that computed it, on that unpack's stream. The segment's value is its pieces' values added in
// increasing offset, starting from the first piece's: `pieces` lists them in that order per segment,
// readable once the plan's work has run.
struct PlanSumsq {
    const unsigned char *want = nullptr;     // one per segment: 0 = not wanted
    std::function<double *(size_t)> pinned;  // n doubles of pinned host memory that outlive the plan's work
    struct Piece {
        size_t seg, elem;     // the segment and the piece's first element in it
        const double *value;  // in the pinned memory
    };
    std::vector<Piece> pieces;  // out: the wanted, non-empty pieces
};

class FusionPipe {
public:
    FusionPipe() = default;
    ~FusionPipe();
    FusionPipe(const FusionPipe &) = delete;
    FusionPipe &operator=(const FusionPipe &) = delete;

    // Fusion buffer i (0 or 1) of at least `need` bytes; an outgrown buffer is retired, not freed
    // (common.h retire_device): earlier uses of it may still be in flight.
    void *ensure(int i, size_t need, hipStream_t stream);
    // elems of the plan's dtype in `buf`, reduced in place on the pipe's stream; `message_bytes`
    // = the whole plan's unpadded bytes (the reference's MPI_Allreduce message)
    using Allreduce = std::function<void(void *buf, size_t elems, size_t message_bytes)>;
    // pack -> allreduce -> unpack of srcs[i] -> dsts[i] (bytes[i] each) on `stream`, pipelined in
    // sub-plans above `cap` bytes (0: never). `ops` (one ddl_allreduce_op per segment, or null =
    // all SUM) with `divisor` = the communicator's size: the unpack of every (sub-)plan holding an
    // AVG segment is the dividing unpack (pack.hip k_seg<DivOp>), which stores the quotients of those
    // segments; the cuts, the packs and the allreduces do not depend on the ops. (A MIN / MAX plan
    // holds one kind only; its caller's `ar` reduces with that kind and the unpack copies.)
    // `src_dtype` != 0 and != dtype (DDL_FLOAT over a 16-bit `dtype`: wire compression): the tensors
    // hold src_dtype elements, `bytes`, `cap`, the cuts and the allreduce are those of the WIRE stream
    // in `dtype` (a tensor's offset at a cut is the wire offset scaled by the element sizes), and
    // the pack / unpack are the converting kernels (SegmentCopier::run_cvt).
    // `residuals` (a compressed plan only; one per segment, null entries = no feedback): the error
    // feedback residuals of DDL_ALLREDUCE_WIRE_FEEDBACK, fp32 arrays indexed like the tensors — a
    // sub-plan's piece takes its residual at the tensor's own element offset. The pack adds them in
    // and rewrites them (k_seg<CvtPackOp<WIRE, true>>); cuts, allreduces and unpacks do not depend on them.
    // `sumsq` (fp32 tensors only; null or no wanted segment: every launch as without it): the unpack of
    // every (sub-)plan holding a wanted piece is k_seg_sumsq (pack.hip); cuts, packs and allreduces do
    // not depend on it.
    void run(const std::vector<const void *> &srcs, const std::vector<void *> &dsts,
             const std::vector<size_t> &bytes, int dtype, size_t cap, hipStream_t stream, const Allreduce &ar,
             const std::vector<int> *ops = nullptr, int divisor = 1, int src_dtype = 0,
             const std::vector<void *> *residuals = nullptr, PlanSumsq *sumsq = nullptr,
             // the scale factors (DDL_ALLREDUCE_SCALE; fp32 tensors only), one per segment, null = none: every
             // piece of a segment is packed with the segment's prescale and unpacked with its postscale
             // (SegmentCopier::run: a launch without a factor other than 1 is the kernel it was); cuts and
             // allreduces do not depend on them
             const std::vector<float> *prescale = nullptr, const std::vector<float> *postscale = nullptr,
             // stochastic rounding (DDL_ALLREDUCE_WIRE_STOCHASTIC; a compressed bf16 plan), one
             // WireStream per segment, null = none: `first` is the index in its request of the segment's first
             // element, and a sub-plan's piece starts where it is cut, so every element keeps the random bits of
             // its index in the request whatever the cuts; a launch without a stochastic segment is the pack it
             // was; cuts, allreduces and unpacks do not depend on them
             const std::vector<WireStream> *streams = nullptr);
    size_t subplans() const { return last_subplans_; }  // of the last run

    SegmentCopier copier;
    // hardware-queue class of the side stream (executor.h QueueClass; set by the owning handler)
    QueueClass qc = QueueClass::kPooled;

private:
    hipEvent_t event_(size_t i);
    void *buf_[2] = {nullptr, nullptr};
    size_t cap_[2] = {0, 0};
    hipStream_t side_ = nullptr;
    std::vector<hipEvent_t> events_;
    size_t last_subplans_ = 0;
};

}  // namespace ddl
