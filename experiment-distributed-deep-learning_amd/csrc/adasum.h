// adasum.h — the Adasum allreduce op (DDL_ALLREDUCE_OP_ADASUM): the scale-invariant combination of the
// ranks' gradients that sums what is orthogonal and averages what is parallel (include/ddl_amd.h "Adasum").
//
// Not element-wise over the P inputs like every other op of the hot path: its coefficients are dot products
// and norms over whole tensors. All of them are functions of the per-tensor Gram matrix G[i][j] = x_i . x_j,
// so a plan is two passes over the data whatever P is (adasum.hip):
//   pack      the plan's requests into this rank's slot of a P-slot gather buffer (SegmentCopier; the
//             prescale rides on it), then ONE allgatherv of the slot;
//   gram      one read of the P slots: G per tensor on the matrix cores (v_mfma_f64_16x16x4_f64), a 16x16
//             partial per tile in a fixed place, added per tensor in a fixed order;
//   coef      one wave per tensor walks the tree on G alone and leaves P fp64 weights (x postscale);
//   apply     out = sum_i w_i x_i in fp64, rounded once to fp32, straight into each request's output.
// No float atomics and no order that depends on the launch shape: every rank stores the same bits.
// Each rank receives (P - 1) n bytes where the direct schedule of a SUM moves about 2 n, and the gather
// buffer holds P x the plan's bytes (DESIGN.md "Adasum").
#pragma once

#include <functional>
#include <utility>
#include <vector>

#include "common.h"

namespace ddl {

constexpr int kAdasumMaxRanks = 16;  // the rows of one MFMA tile

// One tensor of an Adasum plan: `n` fp32 elements, src -> dst.
struct AdasumSeg {
    const void *src;
    void *dst;
    size_t n;
    float prescale = 1.0f, postscale = 1.0f;
};

// Plans of WHOLE requests [begin, end) capped at `limit` bytes: the Gram matrix is of the whole tensor, so a
// plan never cuts one. A request above the cap is a plan of its own.
std::vector<std::pair<size_t, size_t>> adasum_plans(const std::vector<size_t> &elements, size_t limit);

// One per engine thread (the keyed handler's, one per virtual rank of the thread world). Everything is posted
// on the caller's stream; the buffers grow and are retired like the other handler scratch.
class AdasumPipe {
public:
    AdasumPipe() = default;
    ~AdasumPipe();
    AdasumPipe(const AdasumPipe &) = delete;
    AdasumPipe &operator=(const AdasumPipe &) = delete;
    // the allgather of `elems` floats per rank: `send` is rank `rank`'s block inside `recv`
    using Gather = std::function<void(const void *send, void *recv, size_t elems)>;
    void run(const AdasumSeg *segs, int count, int P, int rank, hipStream_t stream, SegmentCopier &copier,
             const Gather &gather);

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
    void *gather_ = nullptr;   // P slots of the plan's flat bytes
    size_t gather_cap_ = 0;
    void *scratch_ = nullptr;  // fp64: the tiles' partials, the tensors' Gram matrices, their weights
    size_t scratch_cap_ = 0;
};

}  // namespace ddl
