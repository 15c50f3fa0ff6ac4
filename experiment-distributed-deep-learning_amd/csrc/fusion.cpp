// fusion.cpp — see fusion.h.
#include "fusion.h"

#include "deptrace.h"
#include "engine.h"

namespace ddl {

FusionPipe::~FusionPipe() {
    // best effort at teardown
    for (hipEvent_t e : events_) (void)hipEventDestroy(e);
    if (side_) (void)hipStreamDestroy(side_);
    for (void *b : buf_)
        if (b) (void)hipFree(b);
}

void *FusionPipe::ensure(int i, size_t need, hipStream_t stream) {
    void *&buf = buf_[i];
    size_t &cap = cap_[i];
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

hipEvent_t FusionPipe::event_(size_t i) {
    while (events_.size() <= i) {
        hipEvent_t e;
        DDL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        events_.push_back(e);
    }
    return events_[i];
}

void FusionPipe::run(const std::vector<const void *> &srcs, const std::vector<void *> &dsts,
                     const std::vector<size_t> &bytes, int dt, size_t cap, hipStream_t stream, const Allreduce &ar,
                     const std::vector<int> *ops, int divisor, int src_dt, const std::vector<void *> *residuals,
                     PlanSumsq *sumsq, const std::vector<float> *prescale, const std::vector<float> *postscale,
                     const std::vector<WireStream> *streams) {
    const size_t es = dtype_size(dt);
    DDL_REQUIRE(es != 0, DDL_STATUS_UNSUPPORTED_DTYPE, "unsupported dtype " << dt);
    const bool cvt = src_dt != 0 && src_dt != dt;
    const size_t ses = cvt ? dtype_size(src_dt) : es;  // the tensors' element size
    DDL_REQUIRE(ses != 0, DDL_STATUS_UNSUPPORTED_DTYPE, "unsupported source dtype " << src_dt);
    // gather (dir 0) / scatter (dir 1) of one (sub-)plan: the converting kernels with a wire dtype
    // (`res`: the pack's residuals of a plan with error feedback)
    // (`want`, `sq`: the unpack's sums of squares, SegmentCopier::run; `scl`: the pack's prescale
    // factors, the unpack's postscale factors; `sts`: the pack's stochastic-rounding streams)
    auto copy = [&](int dir, void *fb, void *const *segs, const size_t *b, int n, hipStream_t s, const int *o,
                    void *const *res = nullptr, const unsigned char *want = nullptr, double *sq = nullptr,
                    const float *scl = nullptr, const WireStream *sts = nullptr) {
        if (cvt)
            copier.run_cvt(dir, fb, segs, b, n, s, src_dt, dt, divisor, o, dir == 0 ? res : nullptr, want, sq, scl,
                           dir == 0 ? sts : nullptr);
        else if (dir == 0) copier.run(0, fb, segs, b, n, s, dt, 1, nullptr, nullptr, nullptr, scl);
        else copier.run(1, fb, segs, b, n, s, dt, divisor, o, want, sq, scl);
    };
    DDL_REQUIRE((!prescale || prescale->size() == bytes.size()) && (!postscale || postscale->size() == bytes.size()),
                DDL_STATUS_INVALID_ARGUMENT, "fusion plan: one scale factor per segment");
    // the statistic only where some segment asks for it: otherwise every launch below is as without it
    bool stat = false;
    for (size_t i = 0; sumsq && sumsq->want && i < bytes.size(); ++i) stat = stat || sumsq->want[i];
    if (sumsq) sumsq->pieces.clear();
    DDL_REQUIRE(!ops || ops->size() == bytes.size(), DDL_STATUS_INVALID_ARGUMENT, "fusion plan: one op per segment");
    DDL_REQUIRE(!residuals || (cvt && residuals->size() == bytes.size()), DDL_STATUS_INVALID_ARGUMENT,
                "fusion plan: one residual per segment of a compressed plan");
    DDL_REQUIRE(!streams || (cvt && streams->size() == bytes.size()), DDL_STATUS_INVALID_ARGUMENT,
                "fusion plan: one stochastic-rounding stream per segment of a compressed plan");
    DDL_REQUIRE(srcs.size() == bytes.size() && dsts.size() == bytes.size(), DDL_STATUS_INVALID_ARGUMENT,
                "fusion plan: " << srcs.size() << " sources, " << dsts.size() << " destinations, " << bytes.size()
                                << " sizes");
    const size_t total = SegmentCopier::flat_bytes(bytes.data(), (int)bytes.size());
    // the reference's MPI buffer holds the requests back to back (no padding): its byte count
    // picks MPICH's summation order (reference_order)
    size_t message = 0;
    for (size_t b : bytes) message += b;
    cap &= ~size_t(255);
    if (cap == 0 || total <= cap) {
        last_subplans_ = 1;
        void *fb = ensure(0, total, stream);
        copy(0, fb, const_cast<void *const *>(reinterpret_cast<const void *const *>(srcs.data())), bytes.data(),
             (int)srcs.size(), stream, nullptr, residuals ? residuals->data() : nullptr, nullptr, nullptr,
             prescale ? prescale->data() : nullptr, streams ? streams->data() : nullptr);
        ar(fb, total / es, message);
        double *sq = stat ? sumsq->pinned(bytes.size()) : nullptr;
        copy(1, fb, dsts.data(), bytes.data(), (int)dsts.size(), stream, ops ? ops->data() : nullptr, nullptr,
             stat ? sumsq->want : nullptr, sq, postscale ? postscale->data() : nullptr);
        for (size_t i = 0; stat && i < bytes.size(); ++i)
            if (sumsq->want[i]) sumsq->pieces.push_back(PlanSumsq::Piece{i, 0, sq + i});
        return;
    }
    struct Sub {
        std::vector<const void *> src;
        std::vector<void *> dst;
        std::vector<size_t> bytes;
        std::vector<int> ops;  // of each piece: its segment's (only with `ops`)
        std::vector<void *> res;  // of each piece: its slice of the segment's residual (only with `residuals`)
        std::vector<unsigned char> want;  // of each piece: its segment's (only with a wanted statistic)
        std::vector<size_t> seg, elem;    //   and the piece's segment and first element in it
        bool stat = false;
        std::vector<float> pre, post;  // of each piece: its segment's factors (only with `prescale` / `postscale`)
        std::vector<WireStream> sts;   // of each piece: its segment's stream from the piece's first element (only with `streams`)
        size_t flat = 0;
    };
    std::vector<Sub> subs(1);
    for (size_t i = 0; i < bytes.size(); ++i) {
        size_t off = 0;
        do {
            Sub *cur = &subs.back();
            if (cur->flat >= cap) {
                subs.emplace_back();
                cur = &subs.back();
            }
            // a piece fills the sub-plan up to cap; every cut is a multiple of 256 bytes (and so of
            // the element size) from the segment start
            const size_t room = cap - cur->flat, left = bytes[i] - off;
            const size_t len = left <= room ? left : room;
            cur->src.push_back(static_cast<const char *>(srcs[i]) + off / es * ses);
            cur->dst.push_back(static_cast<char *>(dsts[i]) + off / es * ses);
            cur->bytes.push_back(len);
            if (ops) cur->ops.push_back((*ops)[i]);
            // the residual is indexed like the tensor: the same fp32 element offset at a cut
            if (residuals)
                cur->res.push_back((*residuals)[i] ? static_cast<char *>((*residuals)[i]) + off / es * ses : nullptr);
            // the random bits are indexed like the tensor: the piece starts at its element offset in the request
            if (streams) cur->sts.push_back(WireStream{(*streams)[i].key, (*streams)[i].first + off / es, (*streams)[i].on});
            if (prescale) cur->pre.push_back((*prescale)[i]);
            if (postscale) cur->post.push_back((*postscale)[i]);
            if (stat) {
                cur->want.push_back(sumsq->want[i]);
                cur->seg.push_back(i);
                cur->elem.push_back(off / es);
                cur->stat = cur->stat || (sumsq->want[i] && len);
            }
            cur->flat += (len + 255) & ~size_t(255);
            off += len;
        } while (off < bytes[i]);
    }
    size_t maxflat = 0;
    for (const Sub &sb : subs) maxflat = sb.flat > maxflat ? sb.flat : maxflat;
    void *buf[2] = {ensure(0, maxflat, stream), ensure(1, maxflat, stream)};
    if (!side_) side_ = create_engine_stream(qc);
    const size_t J = subs.size();
    last_subplans_ = J;
    // events: [0] fork, [1 + 2j] pack j done, [2 + 2j] allreduce j done, [1 + 2J] join
    for (size_t k = 0; k <= 2 * J + 1; ++k) event_(k);
    DDL_HIP(hipEventRecord(events_[0], stream));  // inputs ready (the caller's waits ran on stream)
    dep::record(events_[0], stream);
    DDL_HIP(hipStreamWaitEvent(side_, events_[0], 0));
    dep::wait(side_, events_[0]);
    auto unpack = [&](size_t j) {
        DDL_HIP(hipStreamWaitEvent(side_, events_[2 + 2 * j], 0));
        dep::wait(side_, events_[2 + 2 * j]);
        const Sub &sb = subs[j];
        double *sq = sb.stat ? sumsq->pinned(sb.bytes.size()) : nullptr;
        copy(1, buf[j % 2], sb.dst.data(), sb.bytes.data(), (int)sb.dst.size(), side_, ops ? sb.ops.data() : nullptr,
             nullptr, sb.stat ? sb.want.data() : nullptr, sq, postscale ? sb.post.data() : nullptr);
        // the pieces of a segment in increasing offset: the sub-plans are unpacked in order
        for (size_t k = 0; sb.stat && k < sb.bytes.size(); ++k)
            if (sb.want[k] && sb.bytes[k]) sumsq->pieces.push_back(PlanSumsq::Piece{sb.seg[k], sb.elem[k], sq + k});
    };
    for (size_t j = 0; j < J; ++j) {
        Sub &sb = subs[j];
        copy(0, buf[j % 2], const_cast<void *const *>(reinterpret_cast<const void *const *>(sb.src.data())),
             sb.bytes.data(), (int)sb.src.size(), side_, nullptr, residuals ? sb.res.data() : nullptr, nullptr, nullptr,
             prescale ? sb.pre.data() : nullptr, streams ? sb.sts.data() : nullptr);
        DDL_HIP(hipEventRecord(events_[1 + 2 * j], side_));
        dep::record(events_[1 + 2 * j], side_);
        DDL_HIP(hipStreamWaitEvent(stream, events_[1 + 2 * j], 0));
        dep::wait(stream, events_[1 + 2 * j]);
        ar(buf[j % 2], sb.flat / es, message);
        DDL_HIP(hipEventRecord(events_[2 + 2 * j], stream));
        dep::record(events_[2 + 2 * j], stream);
        if (j >= 1) unpack(j - 1);
    }
    unpack(J - 1);
    DDL_HIP(hipEventRecord(events_[1 + 2 * J], side_));
    dep::record(events_[1 + 2 * J], side_);
    DDL_HIP(hipStreamWaitEvent(stream, events_[1 + 2 * J], 0));
    dep::wait(stream, events_[1 + 2 * J]);
}

}  // namespace ddl
