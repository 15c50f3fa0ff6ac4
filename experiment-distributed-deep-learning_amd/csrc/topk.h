// topk.h — the top-k sparsified wire with error feedback (DDL_ALLREDUCE_WIRE_TOPK): every rank sends the k
// entries of largest magnitude of (gradient + what it has not sent yet) and keeps the rest
// (include/ddl_amd.h "The top-k wire").
//
// Not a dense wire like the others: what travels is k (index, value) pairs per tensor. A plan of whole
// requests runs (topk.hip):
//   select    an exact radix select on the 31-bit magnitude key, digits of 11 / 10 / 10 bits: three histogram
//             passes (the first one also forms a = prescale x g + r and stores it over r) and a one-workgroup
//             scan per tensor behind each, which leave the threshold key T and the number of ties to take;
//   emit      ordered compaction: per-tile counts, a per-tensor scan to tile offsets and tie allowances, then
//             every tile writes its (index, value) pairs in ascending index and zeroes r where it selected;
//   gather    ONE allgatherv of this rank's slot (tile offsets, indices, values per tensor);
//   combine   one workgroup per output tile adds the P ranks' entries of that tile in LDS in rank order and
//             writes the tile once, AVG's quotient and the postscale applied.
// Integer atomics only (the histograms: order-independent), no float atomics, no dense zeroing pass: every rank
// stores the same bits.
#pragma once

#include <functional>
#include <vector>

#include "common.h"

namespace ddl {

// One tensor of a top-k plan: `n` fp32 elements, src -> dst, `residual` n fp32 elements of this rank's own.
struct TopkSeg {
    const void *src;
    void *dst;
    void *residual;
    size_t n;
    float prescale = 1.0f, postscale = 1.0f;
    int op = DDL_ALLREDUCE_OP_SUM;  // SUM or AVG
};

// k = min(n, max(1, ceil(n ppm / 10^6))): the entries a rank sends of a tensor of n elements
inline size_t topk_count(size_t n, long long ppm) {
    const unsigned long long k = ((unsigned long long)n * (unsigned long long)ppm + 999999ull) / 1000000ull;
    return (size_t)std::min<unsigned long long>(n, std::max<unsigned long long>(1, k));
}

// One per engine thread, as AdasumPipe: everything is posted on the caller's stream; the buffers grow and are
// retired like the other handler scratch. A plan holds whole requests (adasum_plans): selection is per tensor.
class TopkPipe {
public:
    TopkPipe() = default;
    ~TopkPipe();
    TopkPipe(const TopkPipe &) = delete;
    TopkPipe &operator=(const TopkPipe &) = delete;
    // the allgather of `elems` 4-byte words per rank: `send` is rank `rank`'s block inside `recv`
    using Gather = std::function<void(const void *send, void *recv, size_t elems)>;
    void run(const TopkSeg *segs, int count, int P, int rank, long long ppm, hipStream_t stream, const Gather &gather);

private:
    struct Table {  // the segment table's pinned staging and its device copy, rewritten once `ready` has passed
        void *host = nullptr, *dev = nullptr;
        size_t cap = 0;
        hipEvent_t ready = nullptr;
    };
    void *grow_(void *&buf, size_t &cap, size_t need);
    static constexpr int kTables = 4;
    Table tab_[kTables];
    int next_ = 0;
    void *gather_ = nullptr;   // P slots
    size_t gather_cap_ = 0;
    void *scratch_ = nullptr;  // uint32: the tensors' histograms and select state, the tiles' counts
    size_t scratch_cap_ = 0;
};

}  // namespace ddl
