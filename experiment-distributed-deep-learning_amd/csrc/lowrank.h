// lowrank.h — the PowerSGD low-rank wire with error feedback (DDL_ALLREDUCE_WIRE_LOWRANK; Vogels et al. 2019,
// PyTorch's powerSGD_hook): every rank sends a rank-r factorisation of its gradient plus residual and keeps what
// that removed (include/ddl_amd.h "The low-rank wire").
//
// A tensor of n elements is the row-major R x C matrix M (C a multiple of 64, about sqrt(n); zero beyond n). The
// wire is REDUCED, not gathered: a plan of whole requests runs (lowrank.hip)
//   project      P_loc = A Q on the fp32 MFMA, K = C split over workgroups; the same kernel forms
//                a = prescale x g + e and stores it to the plan's scratch;
//   fold         the K-split partials added in split order into the plan's P buffer (small tensors: their a);
//   allreduce    ONE in-place fp32 SUM of the P buffer;
//   orthonorm.   one workgroup per tensor: modified Gram-Schmidt in fp64, the column flags, the poison flag;
//   back-project Q_loc = A^T P^ on the MFMA, K = R split over workgroups, then the fold;
//   allreduce    ONE in-place fp32 SUM of the Q buffer;
//   settle       one workgroup per tensor: finiteness first, then Q- = Q^ / P, the stored Q and its flags;
//   reconstruct  D- = P^ Q-^T by FMAs from registers, fused with e' = a - D- and out.
// No float atomics and no order a launch shape decides: every rank stores the same bits.
#pragma once

#include <functional>

#include "common.h"
#include "plan_scratch.h"

namespace ddl {

// One tensor of a low-rank plan: `n` fp32 elements, src -> dst; `residual` (n fp32) and `state` (lowrank_shape's
// state_floats 4-byte words: Q, C x r row-major, then r alive flags) are this rank's own under the request's
// name. A tensor that travels whole (lowrank_shape: small) uses neither: they may be null.
struct LowrankSeg {
    const void *src;
    void *dst;
    void *residual;
    void *state;
    size_t n;
    float prescale = 1.0f, postscale = 1.0f;
    int op = DDL_ALLREDUCE_OP_SUM;  // SUM or AVG
};

// The matrix view of n elements at rank r: C = 64 ceil(sqrt(n) / 64) in integers, R = ceil(n / C); `small`: the
// tensor is not worth compressing, 2 r (R + C) > n. state_floats: C r + r, 0 for a small tensor.
struct LowrankShape {
    size_t R, C, state_floats;
    bool small;
};
inline LowrankShape lowrank_shape(size_t n, int r) {
    size_t m = 1;  // the least m with (64 m)^2 >= n
    while (64 * m * 64 * m < n) ++m;
    LowrankShape s;
    s.C = 64 * m;
    s.R = (n + s.C - 1) / s.C;
    s.small = 2 * (size_t)r * (s.R + s.C) > n;
    s.state_floats = s.small ? 0 : s.C * (size_t)r + (size_t)r;
    return s;
}

// One per engine thread, as SignPipe: everything is posted on the caller's stream; the table staging and the
// scratch are plan_scratch.h's. A plan holds whole requests (adasum_plans).
class LowrankPipe {
public:
    LowrankPipe() = default;
    ~LowrankPipe();
    LowrankPipe(const LowrankPipe &) = delete;
    LowrankPipe &operator=(const LowrankPipe &) = delete;
    // the in-place fp32 SUM allreduce of `elems` floats at `buf`
    using Allreduce = std::function<void(void *buf, size_t elems)>;
    void run(const LowrankSeg *segs, int count, int P, int rank, int r, hipStream_t stream, const Allreduce &allreduce);

private:
    PlanTables tables_;
    void *scratch_ = nullptr;  // P and Q buffers, a, the K-split partials, the flags
    size_t scratch_cap_ = 0;
};

}  // namespace ddl
