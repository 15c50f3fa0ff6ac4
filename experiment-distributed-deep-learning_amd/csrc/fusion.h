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
// The e4m3 wire (dtype kDtypeE4m3 over DDL_FLOAT tensors) is a compressed plan whose wire element is one
// 256-byte granule of 252 tensor elements: the cuts fall between granules (a tensor's offset is 1008 / 256
// times the wire offset), a piece knows its true element count (PlanSeg::elems: the tail), and `ar` is told granules.
//
// One FusionPipe per engine thread: the keyed handler owns one (handler.cpp) and the thread world
// one per virtual rank (executor.cpp, ddl_testing_thread_fused_allreduce), so the same code runs
// under the production executor on one GPU.
#pragma once

#include <functional>
#include <vector>

#include "common.h"

namespace ddl {

// One segment of a fusion plan: src -> dst through the pack, the allreduce and the unpack. The options are
// the copier's (common.h CopySeg); cuts and allreduces depend on the bytes alone.
struct PlanSeg {
    const void *src; void *dst; size_t bytes;  // bytes on the wire side
    // AVG: the unpack stores quotients. (A MIN / MAX plan holds that one kind: `ar` reduces with it, the unpack copies.)
    int op = DDL_ALLREDUCE_OP_SUM;
    float prescale = 1.0f, postscale = 1.0f;  // every piece is packed with the one, unpacked with the other
    void *residual = nullptr;  // error feedback (a compressed plan, the e4m3 wire's too): an fp32 array indexed like the tensor
    WireStream stream{};  // stochastic rounding (a compressed bf16 plan); `first`: the first element's index in its request
    bool want = false;  // the sum of squares of the result (PlanSumsq)
    size_t elems = 0;  // the e4m3 wire only (bytes: whole granules): the fp32 elements of the tensors behind them
    // `len` wire bytes at wire offset `off` (es / ses: the wire's / the tensors' element size; the e4m3 wire: a
    // granule's 256 bytes / the 1008 bytes of its elements): src, dst, residual, stream and elems there
    PlanSeg piece(size_t off, size_t len, size_t es, size_t ses) const;
    CopySeg pack() const { return CopySeg{const_cast<void *>(src), bytes, DDL_ALLREDUCE_OP_SUM, prescale, residual, stream, false, elems}; }
    CopySeg unpack() const { return CopySeg{dst, bytes, op, postscale, nullptr, WireStream{}, want, elems}; }
};

// A plan above `cap` bytes (a non-zero multiple of 256) as sub-plans of at most that size: a piece fills its
// sub-plan up to cap, so every cut is a multiple of 256 bytes from the segment start. seg[k], elem[k]: piece k's
// segment and first element in it (of the tensors, also with the e4m3 wire); flat: the sub-plan's fusion-buffer bytes. No HIP call (fusion_cuts.cpp).
struct SubPlan {
    std::vector<PlanSeg> segs;
    std::vector<size_t> seg, elem;
    size_t flat = 0;
};
std::vector<SubPlan> cut_plan(const std::vector<PlanSeg> &segs, size_t cap, size_t es, size_t ses);

// The sums of squares of a plan's wanted segments. A segment is cut into pieces by the sub-plans (tiles restart
// at every piece); every piece's value — the canonical sum of include/ddl_amd.h over the piece — lands in pinned
// host memory by an async copy behind the unpack that computed it, on that unpack's stream. The segment's value is
// its pieces' values added in increasing offset, starting from the first piece's: `pieces` lists them in that
// order per segment, readable once the plan's work has run.
struct PlanSumsq {
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

    // Fusion buffer i (0 or 1) of at least `need` bytes; an outgrown buffer is retired, not freed (common.h
    // retire_device): earlier uses of it may still be in flight.
    void *ensure(int i, size_t need, hipStream_t stream);
    // elems of the plan's dtype in `buf`, reduced in place on the pipe's stream; `message_bytes`
    // = the whole plan's unpadded bytes (the reference's MPI_Allreduce message)
    using Allreduce = std::function<void(void *buf, size_t elems, size_t message_bytes)>;
    // pack -> allreduce -> unpack of the segments on `stream`, pipelined in sub-plans above `cap` bytes (0: never; an
    // uncut plan is run from the caller's vector). `divisor`: the communicator's size. `src_dtype` != 0 and != dtype
    // (DDL_FLOAT over a 16-bit `dtype`: wire compression): the tensors hold src_dtype elements; bytes, `cap`, the cuts
    // and the allreduce are those of the WIRE stream in `dtype`, and the pack / unpack are the converting kernels.
    // `sumsq`: where the wanted segments' values go (null: nothing is wanted).
    void run(const std::vector<PlanSeg> &segs, int dtype, int src_dtype, size_t cap, int divisor, hipStream_t stream,
             const Allreduce &ar, PlanSumsq *sumsq = nullptr);
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
    std::vector<CopySeg> launch_;  // the segments of the launch being posted, kept between launches
    size_t last_subplans_ = 0;
};

}  // namespace ddl
