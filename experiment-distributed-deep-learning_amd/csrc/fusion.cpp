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

void FusionPipe::run(const std::vector<PlanSeg> &segs, int dt, int src_dt, size_t cap, int divisor, hipStream_t stream,
                     const Allreduce &ar, PlanSumsq *sumsq) {
    const size_t es = dtype_size(dt);
    DDL_REQUIRE(es != 0, DDL_STATUS_UNSUPPORTED_DTYPE, "unsupported dtype " << dt);
    const bool cvt = src_dt != 0 && src_dt != dt;
    const bool q8 = dt == kDtypeE4m3;
    DDL_REQUIRE(!q8 || src_dt == DDL_FLOAT, DDL_STATUS_UNSUPPORTED_DTYPE, "the e4m3 wire carries float32 tensors");
    // the tensors' element size (the e4m3 wire: of the 252 elements behind one wire element)
    const size_t ses = q8 ? kE4m3Elems * sizeof(float) : cvt ? dtype_size(src_dt) : es;
    DDL_REQUIRE(ses != 0, DDL_STATUS_UNSUPPORTED_DTYPE, "unsupported source dtype " << src_dt);
    // gather (dir 0) / scatter (dir 1) of one (sub-)plan on `s`: the converting kernels with a wire dtype.
    // The scatter of a (sub-)plan with a wanted non-empty piece (`all`: or an empty one) takes the sums of
    // squares into pinned memory and returns them, else null: that launch is as without the statistic.
    auto copy = [&](int dir, void *fb, const std::vector<PlanSeg> &p, hipStream_t s, bool all = false) {
        bool stat = false;
        for (size_t i = 0; dir == 1 && sumsq && !stat && i < p.size(); ++i) stat = p[i].want && (all || p[i].bytes);
        launch_.clear();
        for (const PlanSeg &g : p) {
            launch_.push_back(dir == 0 ? g.pack() : g.unpack());
            launch_.back().want = stat && g.want;
        }
        double *sq = stat ? sumsq->pinned(p.size()) : nullptr;
        copier.run(CopyLaunch{dir, fb, s, cvt ? src_dt : dt, cvt ? dt : 0, divisor, sq}, launch_.data(), (int)p.size());
        return sq;
    };
    if (sumsq) sumsq->pieces.clear();
    // the reference's MPI buffer holds the requests back to back (no padding): its byte count
    // picks MPICH's summation order (reference_order)
    size_t total = 0, message = 0;
    for (const PlanSeg &g : segs) {
        total += (g.bytes + 255) & ~size_t(255);
        message += g.bytes;
    }
    cap &= ~size_t(255);
    if (cap == 0 || total <= cap) {
        last_subplans_ = 1;
        void *fb = ensure(0, total, stream);
        copy(0, fb, segs, stream);
        ar(fb, total / es, message);
        const double *sq = copy(1, fb, segs, stream, true);
        for (size_t i = 0; sq && i < segs.size(); ++i)
            if (segs[i].want) sumsq->pieces.push_back(PlanSumsq::Piece{i, 0, sq + i});
        return;
    }
    const std::vector<SubPlan> subs = cut_plan(segs, cap, es, ses);
    size_t maxflat = 0;
    for (const SubPlan &sb : subs) maxflat = sb.flat > maxflat ? sb.flat : maxflat;
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
        const SubPlan &sb = subs[j];
        const double *sq = copy(1, buf[j % 2], sb.segs, side_);
        // the pieces of a segment in increasing offset: the sub-plans are unpacked in order
        for (size_t k = 0; sq && k < sb.segs.size(); ++k)
            if (sb.segs[k].want && sb.segs[k].bytes) sumsq->pieces.push_back(PlanSumsq::Piece{sb.seg[k], sb.elem[k], sq + k});
    };
    for (size_t j = 0; j < J; ++j) {
        const SubPlan &sb = subs[j];
        copy(0, buf[j % 2], sb.segs, side_);
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
