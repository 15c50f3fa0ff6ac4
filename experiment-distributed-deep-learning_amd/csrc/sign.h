// sign.h — the 1-bit sign wire with error feedback (DDL_ALLREDUCE_WIRE_SIGN; 1-bit SGD, EF-signSGD): every rank
// sends one sign bit per element and one fp32 magnitude per block of 2048 elements, and keeps what that removed
// (include/ddl_amd.h "The sign wire").
//
// A dense wire, but gathered, not reduced: a sum of sign codes is no sign code. A plan of whole requests runs
// (sign.hip):
//   pack      one wave per block forms a = prescale x g + r in registers, the block's mean |a| by a xor
//             butterfly, the 64 sign words, and r' = a -+ s; the block is read once and written once;
//   gather    ONE allgatherv of this rank's slot (per tensor: its blocks' scales, then their sign words);
//   combine   one wave per output block adds +-s of the P ranks in rank order and writes the block once, AVG's
//             quotient and the postscale applied; a NaN scale of any rank makes the block NaN.
// No LDS, no atomics, no scratch: every rank stores the same bits.
#pragma once

#include <functional>

#include "common.h"
#include "plan_scratch.h"

namespace ddl {

constexpr size_t kSignBlock = 2048;                  // elements per scale: 64 lanes x 32 bits
constexpr size_t kSignBlockWords = 1 + kSignBlock / 32;  // what a block sends: its scale and 64 sign words

// One tensor of a sign plan: `n` fp32 elements, src -> dst, `residual` n fp32 elements of this rank's own.
struct SignSeg {
    const void *src;
    void *dst;
    void *residual;
    size_t n;
    float prescale = 1.0f, postscale = 1.0f;
    int op = DDL_ALLREDUCE_OP_SUM;  // SUM or AVG
};

inline size_t sign_blocks(size_t n) { return (n + kSignBlock - 1) / kSignBlock; }

// One per engine thread, as TopkPipe: everything is posted on the caller's stream; the buffers grow and are
// retired like the other handler scratch. A plan holds whole requests (adasum_plans).
class SignPipe {
public:
    SignPipe() = default;
    ~SignPipe();
    SignPipe(const SignPipe &) = delete;
    SignPipe &operator=(const SignPipe &) = delete;
    // the allgather of `elems` 4-byte words per rank: `send` is rank `rank`'s block inside `recv`
    using Gather = std::function<void(const void *send, void *recv, size_t elems)>;
    void run(const SignSeg *segs, int count, int P, int rank, hipStream_t stream, const Gather &gather);

private:
    PlanTables tables_;       // the segment tables (plan_scratch.h)
    void *gather_ = nullptr;  // P slots
    size_t gather_cap_ = 0;
};

}  // namespace ddl
