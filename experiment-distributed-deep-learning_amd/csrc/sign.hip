// sign.hip — the kernels of the sign wire and their launcher (sign.h).
//
// Every tensor is cut into blocks of 2048 elements that restart at the tensor's start, so no block straddles two
// tensors. ONE WAVE owns one block (four waves, so four blocks, per workgroup; no wave talks to another, so there
// is no LDS and no barrier); it finds its tensor by a scalar binary search of the table's block0 column (as
// topk.hip). The block is eight rows of 256 elements, and lane w owns elements 4w .. 4w + 3 of every row: a row
// is one fully coalesced 16-byte access per lane (1 KiB per wave), eight rows are the lane's 32 elements, and those
// 32 are exactly the bits of sign word w — bit k is row k >> 2, element k & 3. So nothing is ever exchanged
// between lanes to build the words (no ballot, no transpose), and the word store is one coalesced 256 bytes.
//
// Pack. The lane's 32 a = fl32(pre x g) + r stay in VGPRs from the loads to the stores: the block is read once
// (g and r) and written once (r'), 12 bytes per element plus 33/256 for the slot. The lane sums its |a| in bit
// order, a six-step xor butterfly (the high half by a bpermute, the five steps inside 32 lanes by swizzles) leaves
// the same total in every lane — fp32 addition commutes, so every lane adds the same pairs — and s = total / c.
// A block whose s is not finite (a NaN or an overflowing sum) sends the NaN scale and keeps its r untouched.
//
// Slot of a rank, per tensor of nb blocks and the same on every rank: scale[nb] fp32 | word[64 nb] uint32.
//
// Combine. The wave of an output block reads the P scales by uniform loads and word w of each rank per lane,
// adds bits(s_q) ^ (bit << 31) in rank order into 32 accumulators, and writes eight rows: the quotient by
// (float)P for AVG, the postscale, 0x7fc00000 everywhere where any rank sent the NaN scale.
//
// A tensor pointer that is not 16-byte aligned, and the short last block's rows, go element by element.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sign.h"

namespace ddl {

namespace {

constexpr uint32_t kBlock = (uint32_t)kSignBlock;
constexpr uint32_t kNanScale = 0x7fc00000u;
constexpr uint32_t kSignBit = 0x80000000u;

struct SgSeg {
    uint64_t in, out, res;  // the request's tensors and this rank's residual
    uint64_t n;             // elements
    uint64_t slot;          // the tensor's section inside every slot, in 4-byte words
    uint32_t block0, nblocks;
    float pre, post;
    uint32_t avg, pad;
};

// the last tensor whose block0 <= block (every tensor has at least one block)
__device__ inline int block_tensor(const SgSeg *__restrict__ d, int count, unsigned block) {
    int lo = 0, hi = count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (d[mid].block0 <= block) lo = mid;
        else hi = mid;
    }
    return lo;
}

// a = fl32(pre x g) + r: two operations, each rounded to nearest even, never contracted (pre == 1: g itself)
__device__ inline float accumulate(float g, float pre, float r) {
#pragma clang fp contract(off)
    const float c = pre == 1.0f ? g : g * pre;
    return c + r;
}

// Elements [e, e + 4) of a block of c real ones; those past c read +0.0 and are never written.
__device__ inline void load4(const float *__restrict__ p, uint32_t e, uint32_t c, bool vec, float *v) {
    if (vec && e + 4 <= c) {
        const float4 x = *reinterpret_cast<const float4 *>(p + e);
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) v[j] = e + j < c ? p[e + j] : 0.0f;
}

__device__ inline void store4(float *__restrict__ p, uint32_t e, uint32_t c, bool vec, const float *v) {
    if (vec && e + 4 <= c) {
        *reinterpret_cast<float4 *>(p + e) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        if (e + j < c) p[e + j] = v[j];
}

// t of lane (w xor D): inside 32 lanes a swizzle in bit mode (and 0x1f, or 0, xor D), across them a bpermute
template <int D>
__device__ inline float lane_xor(float t) {
    if constexpr (D >= 32) return __shfl_xor(t, D, 64);
    else return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(t), 0x1f | (D << 10)));
}

// What a wave needs of its block: the tensor's row of the table, the block's index in the tensor, its first
// element and how many are real.
struct BlockAt {
    SgSeg sd;
    uint32_t lb, c;
    uint64_t e0;
};
__device__ inline BlockAt block_at(const SgSeg *__restrict__ d, int count, unsigned blk) {
    BlockAt b;
    b.sd = d[block_tensor(d, count, blk)];
    b.lb = blk - b.sd.block0;
    b.e0 = (uint64_t)b.lb * kBlock;
    const uint64_t left = b.sd.n - b.e0;
    b.c = left < kBlock ? (uint32_t)left : kBlock;
    return b;
}

__global__ void __launch_bounds__(256) k_sign_pack(const SgSeg *__restrict__ d, int count, unsigned blocks,
                                                   uint32_t *__restrict__ slot) {
    const unsigned blk = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (blk >= blocks) return;
    const uint32_t lane = threadIdx.x & 63;
    const BlockAt b = block_at(d, count, blk);
    const float *__restrict__ g = reinterpret_cast<const float *>(b.sd.in) + b.e0;
    float *__restrict__ r = reinterpret_cast<float *>(b.sd.res) + b.e0;
    const bool vg = (b.sd.in & 15u) == 0, vr = (b.sd.res & 15u) == 0;
    float a[32], rv[32];
#pragma unroll
    for (uint32_t row = 0; row < 8; ++row) load4(g, row * 256 + 4 * lane, b.c, vg, a + 4 * row);
#pragma unroll
    for (uint32_t row = 0; row < 8; ++row) load4(r, row * 256 + 4 * lane, b.c, vr, rv + 4 * row);
    float t = 0.0f;
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) {  // (an element past c: +0.0 x pre + +0.0 = +0.0, bit 0)
        a[k] = accumulate(a[k], b.sd.pre, rv[k]);
        t = t + fabsf(a[k]);
        word |= (__float_as_uint(a[k]) >> 31) << k;
    }
    t = t + lane_xor<32>(t);
    t = t + lane_xor<16>(t);
    t = t + lane_xor<8>(t);
    t = t + lane_xor<4>(t);
    t = t + lane_xor<2>(t);
    t = t + lane_xor<1>(t);
    const float s = t / (float)b.c;  // correctly rounded (the compiler's default for fp32 division)
    const uint32_t sb = __float_as_uint(s);
    const bool finite = (sb & 0x7f800000u) != 0x7f800000u;
    uint32_t *__restrict__ mine = slot + b.sd.slot;
    if (lane == 0) mine[b.lb] = finite ? sb : kNanScale;
    mine[b.sd.nblocks + (uint64_t)b.lb * 64 + lane] = word;
    if (!finite) return;  // the block's residual stays as it was
#pragma unroll
    for (uint32_t row = 0; row < 8; ++row) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x = a[4 * row + j];
            v[j] = x - __uint_as_float(sb ^ (__float_as_uint(x) & kSignBit));
        }
        store4(r, row * 256 + 4 * lane, b.c, vr, v);
    }
}

// out block = post(sum over q = 0 .. P - 1, from +0.0, of +-s_q), or the NaN scale's bits where any rank sent them
__global__ void __launch_bounds__(256) k_sign_combine(const uint32_t *__restrict__ gather, uint64_t slot_words, int P,
                                                      const SgSeg *__restrict__ d, int count, unsigned blocks) {
    const unsigned blk = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (blk >= blocks) return;
    const uint32_t lane = threadIdx.x & 63;
    const BlockAt b = block_at(d, count, blk);
    const uint64_t at_scale = b.sd.slot + b.lb, at_word = b.sd.slot + b.sd.nblocks + (uint64_t)b.lb * 64 + lane;
    float acc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.0f;
    bool nan = false;
    for (int q = 0; q < P; ++q) {
        const uint32_t *__restrict__ s = gather + (uint64_t)q * slot_words;
        const uint32_t sb = s[at_scale], word = s[at_word];
        nan = nan || sb == kNanScale;
#pragma unroll
        for (int k = 0; k < 32; ++k) acc[k] = acc[k] + __uint_as_float(sb ^ (((word >> k) & 1u) << 31));
    }
    const float dv = (float)P, post = b.sd.post;
    const bool avg = b.sd.avg != 0;
    float *__restrict__ out = reinterpret_cast<float *>(b.sd.out) + b.e0;
    const bool vo = (b.sd.out & 15u) == 0;
#pragma unroll
    for (uint32_t row = 0; row < 8; ++row) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // the correctly rounded quotient, then the factor: two roundings, as the unpack's
            float y = acc[4 * row + j];
            if (avg) y = y / dv;
            if (post != 1.0f) y = y * post;
            v[j] = nan ? __uint_as_float(kNanScale) : y;
        }
        store4(out, row * 256 + 4 * lane, b.c, vo, v);
    }
}

}  // namespace

SignPipe::~SignPipe() {
    if (gather_) (void)hipFree(gather_);
}

void SignPipe::run(const SignSeg *segs, int count, int P, int rank, hipStream_t stream, const Gather &gather) {
    DDL_REQUIRE(segs && count >= 1 && P >= 1 && rank >= 0 && rank < P, DDL_STATUS_INVALID_ARGUMENT, "bad sign plan");
    // the table, in pinned staging
    const size_t table = (size_t)count * sizeof(SgSeg);
    SgSeg *t = static_cast<SgSeg *>(tables_.stage(table));
    uint64_t blocks = 0;
    for (int i = 0; i < count; ++i) {
        const SignSeg &s = segs[i];
        DDL_REQUIRE(s.n >= 1 && s.src && s.dst && s.residual, DDL_STATUS_INVALID_ARGUMENT, "null or empty tensor " << i);
        DDL_REQUIRE((reinterpret_cast<uintptr_t>(s.src) | reinterpret_cast<uintptr_t>(s.dst) |
                     reinterpret_cast<uintptr_t>(s.residual)) % 4 == 0,
                    DDL_STATUS_INVALID_ARGUMENT, "tensor " << i << " is not aligned float32 elements");
        DDL_REQUIRE(s.op == DDL_ALLREDUCE_OP_SUM || s.op == DDL_ALLREDUCE_OP_AVG, DDL_STATUS_INVALID_ARGUMENT,
                    "the sign wire takes SUM or AVG");
        const uint64_t nb = sign_blocks(s.n);
        SgSeg &e = t[i];
        e.in = reinterpret_cast<uint64_t>(s.src);
        e.out = reinterpret_cast<uint64_t>(s.dst);
        e.res = reinterpret_cast<uint64_t>(s.residual);
        e.n = s.n;
        e.slot = blocks * kSignBlockWords;
        e.block0 = (uint32_t)blocks;
        e.nblocks = (uint32_t)nb;
        e.pre = s.prescale;
        e.post = s.postscale;
        e.avg = s.op == DDL_ALLREDUCE_OP_AVG;
        e.pad = 0;
        blocks += nb;
        DDL_REQUIRE(blocks < (1ull << 31), DDL_STATUS_INVALID_ARGUMENT, "sign plan too large");
    }
    const SgSeg *dd = static_cast<const SgSeg *>(tables_.upload(stream));

    const uint64_t words = blocks * kSignBlockWords;
    const size_t slot_bytes = (size_t)words * 4, need = (size_t)P * slot_bytes;
    char *g = static_cast<char *>(grow_retire(gather_, gather_cap_, need));
    uint32_t *own = reinterpret_cast<uint32_t *>(g + (size_t)rank * slot_bytes);

    const dim3 grid((unsigned)((blocks + 3) / 4)), wg(256);  // one wave per block
    hipLaunchKernelGGL(k_sign_pack, grid, wg, 0, stream, dd, count, (unsigned)blocks, own);
    DDL_HIP(hipGetLastError());
    if (P > 1) gather(own, g, (size_t)words);
    hipLaunchKernelGGL(k_sign_combine, grid, wg, 0, stream, reinterpret_cast<const uint32_t *>(g), words, P, dd, count,
                       (unsigned)blocks);
    DDL_HIP(hipGetLastError());
}

}  // namespace ddl
