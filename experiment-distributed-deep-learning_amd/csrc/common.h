// common.h — shared definitions of the MI355X allreduce engine (host side).
//
// dtype numbers and status codes follow the C-ABI (include/ddl_amd.h), which mirrors the
// reference's tensorflow::DataType use (src/cpp/def.h:10) and StatusCode (def.h:70-74).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <sstream>
#include <vector>

#include "ddl_amd_testing.h"

namespace ddl {

// The wire element of DDL_ALLREDUCE_WIRE_E4M3 as a dtype of the engine's own (never a ddl_dtype: the C-ABI
// refuses it): one 256-byte granule — 252 e4m3fn codes and an fp32 scale (include/ddl_amd.h "The e4m3 wire").
// Plans, cuts, chunks and slices of such an allreduce count granules; its reduce is k_foldq, on the fold-once
// schedules only, its inputs always in rank order.
constexpr int kDtypeE4m3 = 0x1e43;
constexpr size_t kE4m3Granule = 256, kE4m3Elems = 252;
inline size_t e4m3_granules(size_t elements) { return (elements + kE4m3Elems - 1) / kE4m3Elems; }

inline size_t dtype_size(int dt) {
    switch (dt) {
        case kDtypeE4m3: return kE4m3Granule;
        case DDL_FLOAT: case DDL_INT32: return 4;
        case DDL_DOUBLE: case DDL_INT64: case DDL_UINT64: return 8;
        case DDL_HALF: case DDL_BFLOAT16: return 2;
        default: return 0;
    }
}

inline const char *dtype_name(int dt) {
    switch (dt) {
        case DDL_FLOAT: return "float32";
        case DDL_DOUBLE: return "float64";
        case DDL_INT32: return "int32";
        case DDL_INT64: return "int64";
        case DDL_UINT64: return "uint64";
        case DDL_HALF: return "float16";
        case DDL_BFLOAT16: return "bfloat16";
        case kDtypeE4m3: return "e4m3 granule";
        default: return "unsupported";
    }
}

inline bool dtype_is_float(int dt) {
    return dt == DDL_FLOAT || dt == DDL_DOUBLE || dt == DDL_HALF || dt == DDL_BFLOAT16;
}

// Thread-local description of the last failure (ddl_last_error).
void set_error(const std::string &msg);
const char *last_error();

// Error carried inside the library; converted to a status at the C-ABI (no exception
// crosses the boundary).
struct Error {
    int status;
    std::string msg;
};

[[noreturn]] inline void fail(int status, const std::string &msg) { throw Error{status, msg}; }

#define DDL_HIP(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            std::ostringstream _os;                                                         \
            _os << #expr << " failed: " << hipGetErrorString(_e) << " (" << __FILE__ << ":" \
                << __LINE__ << ")";                                                         \
            ::ddl::fail(DDL_STATUS_HIP_ERROR, _os.str());                                   \
        }                                                                                   \
    } while (0)

#define DDL_REQUIRE(cond, status, msg)                    \
    do {                                                  \
        if (!(cond)) {                                    \
            std::ostringstream _os;                       \
            _os << msg;                                   \
            ::ddl::fail((status), _os.str());             \
        }                                                 \
    } while (0)

inline bool op_is_minmax(int op) { return op == DDL_ALLREDUCE_OP_MIN || op == DDL_ALLREDUCE_OP_MAX; }
// What the reduce and fold kernels of an allreduce with `op` compute (launch_sum2 / launch_sumN's
// `op`): AVG is a SUM whose result is divided afterwards, MIN / MAX are themselves.
inline int reduce_kind(int op) { return op_is_minmax(op) ? op : DDL_ALLREDUCE_OP_SUM; }

// The op of every allreduce entry point: SUM, AVG (float types only), MIN or MAX. Refused before
// anything is posted; the dtype is the same on every rank, so all ranks refuse together.
inline void check_allreduce_op(int op, int dtype) {
    DDL_REQUIRE(op == DDL_ALLREDUCE_OP_SUM || op == DDL_ALLREDUCE_OP_AVG || op_is_minmax(op),
                DDL_STATUS_INVALID_ARGUMENT, "unknown allreduce op " << op << " (SUM = 0, AVG = 1, MIN = 3, MAX = 4)");
    DDL_REQUIRE(op != DDL_ALLREDUCE_OP_AVG || dtype_size(dtype) == 0 || dtype_is_float(dtype),
                DDL_STATUS_UNSUPPORTED_DTYPE, "AVG is not defined for " << dtype_name(dtype));
}

// The `op` of a keyed allreduce request: SUM / AVG / MIN / MAX in the low bits, with SUM / AVG
// optionally one ddl_allreduce_wire format flag, optionally DDL_ALLREDUCE_WIRE_FEEDBACK with it, or
// DDL_ALLREDUCE_WIRE_STOCHASTIC with WIRE_BF16; or DDL_ALLREDUCE_WIRE_E4M3 alone (kDtypeE4m3), optionally with
// DDL_ALLREDUCE_WIRE_E4M3_FEEDBACK (then *feedback is set: the wire dtype says which rule). Returns the wire dtype (DDL_HALF / DDL_BFLOAT16; 0 =
// uncompressed), leaves the op in *base, the feedback bit in *feedback and the stochastic bit in
// *stochastic. Refusals as ddl_amd.h lists them, before anything is registered.
inline int decode_keyed_op(int op, int dtype, bool host, int *base, bool *feedback, bool *stochastic) {
    constexpr int kWire = DDL_ALLREDUCE_WIRE_FP16 | DDL_ALLREDUCE_WIRE_BF16;
    const bool q8 = (op & DDL_ALLREDUCE_WIRE_E4M3) != 0;
    const bool q8fb = (op & DDL_ALLREDUCE_WIRE_E4M3_FEEDBACK) != 0;
    *base = op & ~(kWire | DDL_ALLREDUCE_WIRE_FEEDBACK | DDL_ALLREDUCE_WIRE_STOCHASTIC | DDL_ALLREDUCE_WIRE_E4M3 |
                   DDL_ALLREDUCE_WIRE_E4M3_FEEDBACK);
    *feedback = (op & DDL_ALLREDUCE_WIRE_FEEDBACK) != 0;
    *stochastic = (op & DDL_ALLREDUCE_WIRE_STOCHASTIC) != 0;
    const int w = op & kWire;
    DDL_REQUIRE(w != kWire, DDL_STATUS_INVALID_ARGUMENT, "both wire flags in allreduce op " << op);
    DDL_REQUIRE(*base == DDL_ALLREDUCE_OP_SUM || *base == DDL_ALLREDUCE_OP_AVG || op_is_minmax(*base),
                DDL_STATUS_INVALID_ARGUMENT,
                "unknown allreduce op " << op << " (SUM = 0, AVG = 1, | WIRE_FP16 = 0x100 or WIRE_BF16 = 0x200, "
                                                 "| WIRE_FEEDBACK = 0x1000 with one of them, | WIRE_STOCHASTIC = "
                                                 "0x8000 with WIRE_BF16; MIN = 3, MAX = 4)");
    DDL_REQUIRE(!op_is_minmax(*base) || (!w && !*feedback && !*stochastic), DDL_STATUS_INVALID_ARGUMENT,
                "MIN / MAX take no wire flag (allreduce op " << op << ")");
    DDL_REQUIRE(w || !*feedback, DDL_STATUS_INVALID_ARGUMENT,
                "WIRE_FEEDBACK without WIRE_FP16 or WIRE_BF16 in allreduce op " << op);
    DDL_REQUIRE(!*stochastic || w == DDL_ALLREDUCE_WIRE_BF16, DDL_STATUS_INVALID_ARGUMENT,
                "WIRE_STOCHASTIC takes WIRE_BF16 and no other wire flag (allreduce op " << op << ")");
    DDL_REQUIRE(!*stochastic || !*feedback, DDL_STATUS_INVALID_ARGUMENT,
                "WIRE_STOCHASTIC and WIRE_FEEDBACK are alternatives (allreduce op " << op << ")");
    DDL_REQUIRE(!q8 || (!w && !*feedback && !*stochastic), DDL_STATUS_INVALID_ARGUMENT,
                "WIRE_E4M3 takes no other wire flag, no WIRE_FEEDBACK and no WIRE_STOCHASTIC (allreduce op " << op << ")");
    DDL_REQUIRE(!(q8 || q8fb) || !op_is_minmax(*base), DDL_STATUS_INVALID_ARGUMENT,
                "MIN / MAX take no wire flag (allreduce op " << op << ")");
    DDL_REQUIRE(!q8fb || q8, DDL_STATUS_INVALID_ARGUMENT,
                "WIRE_E4M3_FEEDBACK takes WIRE_E4M3 and no other wire flag (allreduce op " << op << ")");
    if (q8fb) *feedback = true;
    if (!w && !q8) return 0;
    DDL_REQUIRE(!host, DDL_STATUS_INVALID_ARGUMENT, "wire compression is for device requests only");
    DDL_REQUIRE(dtype == DDL_FLOAT, DDL_STATUS_UNSUPPORTED_DTYPE,
                "wire compression is defined for float32 only, not " << dtype_name(dtype));
    if (q8) return kDtypeE4m3;
    return w == DDL_ALLREDUCE_WIRE_FP16 ? DDL_HALF : DDL_BFLOAT16;
}

// The e4m3 wire folds every chunk once: at most kMaxInputs + 1 ranks (more would go through partials, which
// requantize). The one refusal of every entry point that takes the wire, before anything is registered.
inline void check_wire_ranks(int wire, int size) {
    DDL_REQUIRE(wire != kDtypeE4m3 || size <= 16, DDL_STATUS_INVALID_ARGUMENT,
                "DDL_ALLREDUCE_WIRE_E4M3 takes a communicator of at most 16 ranks, not " << size);
}

// Stochastic rounding of the bf16 wire (DDL_ALLREDUCE_WIRE_STOCHASTIC; the rule, R and the host mix are
// fixed in ddl_amd.h and restated in tests/_stochastic_helpers.py). One per segment of a converting pack:
// the stream key S of the segment's request, the index in that request of the segment's first element
// (a piece of a cut request does not start at 0) and whether the segment is rounded stochastically at all.
struct WireStream {
    uint64_t key = 0;
    uint64_t first = 0;
    uint64_t on = 0;
};
// mix64: one splitmix64 step (add the golden-ratio increment, then its finaliser).
inline uint64_t sr_mix64(uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
// S = mix64(mix64(mix64(mix64(seed) ^ rank) ^ fnv1a64(key bytes)) ^ n)
inline uint64_t stochastic_stream(uint64_t seed, uint64_t rank, const void *key, size_t len, uint64_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < len; ++i) h = (h ^ static_cast<const unsigned char *>(key)[i]) * 0x100000001b3ull;
    return sr_mix64(sr_mix64(sr_mix64(sr_mix64(seed) ^ rank) ^ h) ^ n);
}

// Logging (the reference logs per rank to log-<rank>.txt, GlobalLog.cc:17-49; here
// stderr, gated by the "log_level" config: 0 errors, 1 info, 2 debug).
int log_level();
void log_line(int level, const std::string &msg);

#define DDL_LOG(level, msg)                                     \
    do {                                                        \
        if (::ddl::log_level() >= (level)) {                    \
            std::ostringstream _os;                             \
            _os << msg;                                         \
            ::ddl::log_line((level), _os.str());                \
        }                                                       \
    } while (0)

// Step-by-step trace of the program posting (log_level >= 4): every HIP call of run_, flushed
// before the call, so a crash inside the runtime names the call it was in.
#define DDL_TRACE(msg)                                                                          \
    do {                                                                                        \
        if (::ddl::log_level() >= 4) {                                                          \
            std::ostringstream _os;                                                             \
            _os << msg;                                                                         \
            std::fprintf(stderr, "[ddl trace] %s\n", _os.str().c_str());                         \
            std::fflush(stderr);                                                                \
        }                                                                                       \
    } while (0)

// ---- kernels (reduce_kernels.hip) ----------------------------------------------------
constexpr int kMaxSegments = 8;

// Up to kMaxSegments independent out = a + b problems in one launch (one per ring).
struct SegTable {
    const void *a[kMaxSegments];
    const void *b[kMaxSegments];
    void *out[kMaxSegments];
    uint64_t n[kMaxSegments];
    int count;
};

// One N-input problem over the inputs x_0 = a, x_1 = b[0], ..., x_nb = b[nb-1]: the direct and
// one-shot schedules' reduce of a chunk with its P-1 received copies.
constexpr int kMaxInputs = 15;
static_assert(kMaxInputs + 1 == 16, "check_wire_ranks: the e4m3 wire's rank cap is one fold's inputs");
// Addition order of an N-input fold (fp32 / fp64; integers wrap, so any order is the same):
enum FoldOrder : int {
    kFoldLeft = 0,      // ((x_0 + x_1) + x_2) + ...: the ring-0 order of the direct schedule
    kFoldMpichTree = 1, // MPICH 3.3.2 MPI_Allreduce above 2048 bytes (x in rank order): the first
                        // 2*rem inputs folded in pairs, then a pairwise tree over pof2 leaves
    kFoldBinomial = 2,  // MPICH 3.3.2 MPI_Allreduce up to 2048 bytes: binomial tree over ranks
};
// MPICH's order for an allreduce of `message_bytes` of `esize`-byte elements over P ranks
// (MPICH 3.3.2 MPIR_Allreduce_intra_auto): recursive doubling — the binomial order — when the
// message is at most MPIR_CVAR_ALLREDUCE_SHORT_MSG_SIZE = 2048 bytes or its element count is
// below pof2 (largest power of two <= P; above 2048 bytes that takes P >= 512), else
// reduce-scatter + allgather (pre-fold + pairwise tree). Pinned by live MPICH runs up to P = 520
// on one host (tests/golden, tests/test_live_mpich.py).
inline int mpich_fold_order(size_t message_bytes, size_t esize, int P) {
    size_t pof2 = 1;
    while (pof2 * 2 <= (size_t)P) pof2 *= 2;
    return message_bytes <= 2048 || message_bytes / esize < pof2 ? kFoldBinomial : kFoldMpichTree;
}
struct SegTableN {
    const void *a;
    const void *b[kMaxInputs];
    void *out;
    uint64_t n;
    int nb;
    int order = kFoldLeft;  // FoldOrder
};
// fp32/fp64/int: one rounding per add in `order`; fp16/bf16 (no reference order: the reference
// rejects them): accumulate in fp32 and round once at the end, whatever the order.
// `op`: DDL_ALLREDUCE_OP_SUM, or _MIN / _MAX (the element-wise IEEE 754-2019 minimum / maximum, the
// integer order; associative, so `order` is not used).
void launch_sumN(const SegTableN &t, int dtype, hipStream_t stream, int op = DDL_ALLREDUCE_OP_SUM);
// Up to kMaxFoldBatch independent folds with the same input count and order in ONE launch
// (blockIdx.y = problem): the grouped allreduce folds every bucket's slice of a tick together, so
// 64 back-to-back 2 MiB fp16 chunks (C4) become 8 launches of 8 chunks instead of 64 latency-bound
// ones. No problem may read what another writes. Misaligned problems are launched one by one.
constexpr int kMaxFoldBatch = 8;
struct FoldBatch {
    SegTableN t[kMaxFoldBatch];
    int count;
};
void launch_sumN_batch(const SegTableN *t, int count, int dtype, hipStream_t stream, int op = DDL_ALLREDUCE_OP_SUM);

// Reduce-kernel cache-policy / staging flags (bit set). kVariantDefault is what the engine uses;
// the others exist for measurement (ddl_reduce_sum2_variant, bench.py, tools/reduce_tune.hip).
enum ReduceVariant : int {
    kNtLoadA = 1,   // non-temporal loads of operand a (the rank's own gradient: read once)
    kNtLoadB = 2,   // non-temporal loads of operand b (the received chunk)
    kNtStore = 4,   // non-temporal stores of out
    kLdsStageB = 8, // operand b staged through LDS by global_load_lds_dwordx4
    kWtStore = 16,  // write-through stores of out (sc0 sc1: the line leaves the XCD's L2)
    kVariantMask = 31,
    // run form (r05): one workgroup per run of 8 tiles (kRun4: 4 tiles), a's run loaded, then
    // b's, then the stores — each workgroup on one stream at a time, as the fold's run form (cache
    // bits from the low bits; the LDS staging bit is not combined with it). default_variant takes
    // it with 4-tile runs from 32 to 128 MiB.
    kRunForm = 32,
    kRun4 = 64,
};
int default_variant(size_t bytes);  // standalone reduce (ddl_reduce_local / ddl_reduce_sum2), by bucket size
int ring_variant();     // reduce-scatter step of the ring
// Form of the N-input fold (config "fold_form"): 0 auto (the run form for chunks of at least 4 MiB
// and at least 7 inputs), 1 the tile form always, 2 the run form always (the binomial order is
// always tiled). Local: it changes no collective's program, only the kernel (the same sums either
// way).
void set_fold_form(int form);
void set_testing_fold_variant(int v);  // ddl_testing_fold_variant: 4 / 5 forced, -1 the size rule
int get_fold_form();

// out = a + b for each segment; dtype-generic. Returns via fail() on bad arguments.
// variant < 0 selects default_variant(). `op` as launch_sumN's; MIN / MAX take the variants
// default_variant and ring_variant choose, not the measurement-only ones.
void launch_sum2(const SegTable &t, int dtype, hipStream_t stream, int variant = -1, int op = DDL_ALLREDUCE_OP_SUM);
int device_cu_count();

// Chunk boundaries [cut[i], cut[i + 1]) of a host-staged transfer of `total` bytes through
// `chunk`-byte slots (chunk a multiple of 256): whole chunks, the last one short. They depend
// only on (total, chunk) — host_chunk_bytes is a shared tunable — so every rank cuts the same
// chunks (the per-chunk collectives must match). (r03 measured quarter chunks at the ends of a
// transfer — a shorter fill and drain — against whole chunks on two boxes: never faster, DESIGN §7;
// that option is gone.)
inline std::vector<size_t> host_chunk_cuts(size_t total, size_t chunk) {
    std::vector<size_t> cut{0};
    while (cut.back() < total) cut.push_back(cut.back() + std::min(chunk, total - cut.back()));
    return cut;
}

// One segment of one SegmentCopier launch. An option's kernel and table are a launch's only where some
// non-empty segment of it asks for the option: every other launch is the kernel it was, its tables
// unchanged, and a segment without the option inside such a launch is moved as it was. A launch ignores
// what it cannot use: a converting pack `op` and `want`; a scatter `residual` and `stream`; kSumsqInPlace
// `op` and `scale`; a non-converting launch `residual` and `stream`; an e4m3 pack `stream`.
struct CopySeg {
    void *ptr = nullptr;  // the tensor side: read by a pack, written by a scatter / in place
    size_t bytes = 0;     // flat-side bytes (wire bytes for a converting copy: elements x 2)
    // DDL_ALLREDUCE_OP_AVG with CopyLaunch::divisor > 1 (a float dtype): the scatter stores the quotient of
    // the segment's elements (k_seg<DivOp> in place of k_seg<CopyOp>), kDivInPlace divides them in place
    int op = DDL_ALLREDUCE_OP_SUM;
    // DDL_ALLREDUCE_SCALE (finite and > 0; DDL_FLOAT, or DDL_BFLOAT16 without a wire: widened, multiplied in fp32
    // and narrowed once per kernel — ScaleGather16Op, DivOp<kDivBF16, true>): dir 0 multiplies the elements on their way into the
    // flat buffer (the prescale, ahead of the narrowing and the residual's addition), dir 1 and kDivInPlace
    // on their way into the tensors, behind the widening and AVG's quotient (the postscale); the sum of
    // squares is of the scaled values
    float scale = 1.0f;
    // DDL_ALLREDUCE_WIRE_FEEDBACK (a converting pack): the segment packs narrow(tensor + residual) and leaves
    // what the rounding removed in `residual` (fp32, the segment's element count; CvtPackOp<WIRE, true>)
    // DDL_ALLREDUCE_WIRE_E4M3_FEEDBACK (an e4m3 pack): the granules of tensor + residual, and what their
    // quantization removed in `residual` (fp32, `elems` elements; Q8PackOp<SCALE, true>)
    void *residual = nullptr;
    // DDL_ALLREDUCE_WIRE_STOCHASTIC (a converting bf16 pack): a segment with stream.on (and no residual) is
    // narrowed by the rule of ddl_amd.h (k_seg<CvtPackSrOp>)
    WireStream stream{};
    // DDL_ALLREDUCE_SUMSQ (DDL_FLOAT, or DDL_BFLOAT16 without a wire: k_seg_sumsq16, the squares of the stored
    // bf16 values in the 2-byte order; dir 1 / kSumsqInPlace): k_seg_sumsq in place of k_seg stores what k_seg
    // would and leaves one fp64 partial per 1 KiB tile of the wanted segments (with a wire in the compressed
    // order: 512 elements per tile, 8 per lane), then the finishing kernel and an async copy of the launch's
    // values into CopyLaunch::sumsq on its stream. The order of the additions: include/ddl_amd.h.
    bool want = false;
    // the e4m3 wire (CopyLaunch::wire == kDtypeE4m3) only: the segment's true fp32 element count. `bytes` is
    // whole granules there (the one place where the tensor side is not bytes x a constant: the tail)
    size_t elems = 0;
};
struct CopyLaunch {  // what is per launch, not per segment
    int dir;         // 0 gather, 1 scatter, SegmentCopier::kDivInPlace, SegmentCopier::kSumsqInPlace
    void *flat;      // unused in place
    hipStream_t stream;
    int dtype = 0;  // the tensors' dtype
    // 0: the plain copies. DDL_HALF / DDL_BFLOAT16: the converting copies of the wire compression
    // (ddl_allreduce_wire; dir 0, 1, kSumsqInPlace) — the tensors hold DDL_FLOAT, the flat buffer `wire`
    // elements, so offsets, tiles and flat_bytes are the wire stream's. dir 0: round to nearest even
    // (k_seg<CvtPackOp>); dir 1: widen, AVG segments divided by (float)divisor (k_seg<CvtUnpackOp>).
    int wire = 0;
    int divisor = 1;  // the communicator's size
    // dir 1 / kSumsqInPlace: `count` doubles of PINNED host memory that stay valid until the work posted has
    // run; +0.0 at return, then every wanted non-empty segment's value
    double *sumsq = nullptr;
};

// Gather (dir 0: segments -> flat) / scatter (dir 1: flat -> segments) between tensors and a
// fusion buffer in one launch (pack.hip). Segment i sits at the running sum of the 256-byte-
// rounded lengths before it. Not thread-safe: one copier per engine thread.
class SegmentCopier {
public:
    SegmentCopier() = default;
    ~SegmentCopier();
    SegmentCopier(const SegmentCopier &) = delete;
    SegmentCopier &operator=(const SegmentCopier &) = delete;
    // the AVG segments divided and the scaled ones multiplied where they are (nothing else is touched)
    static constexpr int kDivInPlace = 2;
    // the sums of squares, read-only, over segments that hold their results (nothing wanted: nothing posted)
    static constexpr int kSumsqInPlace = 3;
    // Every refusal comes before anything is posted.
    void run(const CopyLaunch &how, const CopySeg *segs, int count);
    // The plain copy of ptrs[i] (bytes[i] each) into or out of `flat`.
    void copy(int dir, void *flat, void *const *ptrs, const size_t *bytes, int count, hipStream_t stream);
    static size_t flat_bytes(const size_t *bytes, int count);

private:
    struct Slot {
        void *host = nullptr, *dev = nullptr;
        size_t cap = 0;
        void *idx = nullptr;  // device tile -> segment map (k_tile_index): a byte or an int32 per tile
        size_t idx_cap = 0;
        void *stat = nullptr;  // device: the tiles' partial sums of squares, then one result per segment
        size_t stat_cap = 0;
        hipEvent_t ready = nullptr;
    };
    Slot &free_slot_();  // a slot whose last table copy has been consumed (grows the pool)
    static constexpr size_t kMaxSlots = 64;
    std::vector<Slot> slots_;
    std::vector<CopySeg> plain_;  // copy()'s segments, kept between calls
    size_t next_ = 0;
};

// Memory a data path outgrew (r06). hipFree / hipHostFree synchronise the whole device, and on a
// thread that posts RCCL work that can deadlock the ranks once two communicators are in flight:
// rank A's handler of communicator X blocks in hipFree until its in-flight kernel of communicator
// Y finishes, which waits for rank B's Y kernel, which B's handler of Y has not posted because it
// is blocked the same way behind its X kernel, which waits for A's X work (found with multi-rank
// RCCL communicators on one GPU, tests/test_multiproc_rccl_gpu.py). So buffers that grow during
// operation (staging, fusion buffers, pinned slots, tuning scratch) hand their old allocation here
// instead of freeing it; ddl_finalize frees the lot once every communicator is gone. Growth is
// geometric, so what waits here is less than twice the final sizes.
void retire_device(void *p);
void retire_host(void *p);
void free_retired();
// Device scratch of at least `bytes` for the calling thread on the current device (the control
// collectives: config agreement, the tuner's max, split records) — no allocation per call.
void *thread_scratch(size_t bytes);

// Hardware-queue class of an engine stream (executor.h create_engine_stream).
enum class QueueClass { kPooled, kHigh, kLow };

}  // namespace ddl
