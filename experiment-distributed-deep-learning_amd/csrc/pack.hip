// pack.hip — fusion gather/scatter between many gradient tensors and one HBM fusion buffer.
//
// Replaces the per-tensor memcpy loops of MPIRingTokenCommunication::executeCommunicatePlan_
// (MPIRingTokenCommunication.cc:548-733: memcpy in -> MPI_Allreduce -> memcpy out) with one
// launch per direction for any number of segments. HBM-bound copy: 2 bytes moved per byte.
//
// Fused layout: segment i occupies [off_i, off_i + len_i) of the flat buffer, off_i = running
// sum of the 256-byte-rounded lengths before it (every segment starts 256-byte aligned, so a
// fused bucket keeps the ring's 16-byte vector alignment). The segment table lives in device
// memory (uploaded with one async copy from a pinned staging table). Default mapping: every
// segment is cut into 1 KiB tiles that restart at the segment start, one 64-lane workgroup per
// tile, the tile's segment from a one-byte-per-tile index built on the device (k_tile_index).
// One kernel, k_seg, walks the tiles for every operation; what an operation does to a 16-byte
// unit and to a single element is its Op struct (CopyOp, DivOp, CvtPackOp, CvtUnpackOp, ScaleGatherOp,
// ScaleGather16Op, Q8PackOp, Q8UnpackOp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "common.h"
#include "deptrace.h"
#include "e4m3.h"

namespace ddl {

namespace {

using u32x4 = unsigned int __attribute__((ext_vector_type(4)));

struct SegDesc {
    uint64_t ptr;   // segment address (tensor side)
    uint64_t off;   // offset in the flat buffer (256-byte aligned)
    uint64_t len;   // bytes
    uint32_t vec;   // kSegVec: ptr is 16-byte aligned (16-byte units, else elements); kSegAvg; kSegStat; kSegScale
    uint32_t tile0; // segment-aligned tiling: index of the segment's first tile
};
// kSegStat: the segment's sum of squares is wanted (k_seg_sumsq only; the other kernels never see it)
// kSegScale: the segment's elements are multiplied by its factor of the launch's factor table (the scaled
// kernels only; the other kernels never see it)
constexpr uint32_t kSegVec = 1, kSegAvg = 2, kSegStat = 4, kSegScale = 8;

// Segment-aligned tiling: every segment is cut into tiles of kSegTile bytes that restart at the
// segment start, so a tile never crosses a segment and its workgroup needs no per-chunk search:
// the tile index (k_tile_index: one thread per tile, binary search of the tile0 column) names
// the segment, one scalar descriptor load gives ptr / off / len, and lane l moves bytes
// [16 l, 16 l + 16) of the tile. Small tiles keep the chunks in flight a compact window of each
// stream (tools/copy_tune.hip: 1R+1W copies reach 6.5 TB/s with 1-2 KiB per workgroup vs 5.3 TB/s
// with 64 KiB). One 1 KiB tile per 64-lane workgroup: the r01 tile-shape measurement (C5 bucket
// set, pack / unpack) had 6.10 / 6.37 TB/s for it against 6.09 / 6.29 for 2 KiB tiles of 128 lanes
// and 5.74 / 6.30 for 4 KiB tiles of 128 lanes x 2 chunks; the span kernel with an in-kernel
// segment search (2-64 KiB spans) 4.5-6.0. Other shapes are tried in tools/copy_tune.hip.
constexpr uint64_t kSegTile = 1024;
// Tile -> segment map, compact: the dispatcher deals workgroups round-robin over the 8 XCDs,
// each with its own L2, so every 128-byte line of a per-tile index is fetched by all 8 (r01: an
// int32 per tile cost +3.2 % HBM traffic on the C5 set). The map is therefore one byte per tile,
// the segment's distance from a per-128-tile base (kIdxBlock), so a line covers 128 tiles:
// seg = base[tile / 128] + delta[tile]. When some block spans more than 255 segments (runs of
// empty segments) the host falls back to an int32 per tile. Remapping tiles to XCDs instead cut
// the traffic too but slowed the copy 4-5 % (profiles/r02/pack/pack_xcd_ab.txt).
constexpr uint32_t kIdxBlock = 128;

template <bool NARROW>
__global__ void __launch_bounds__(256) k_tile_index(const SegDesc *__restrict__ d, int count, uint64_t tiles,
                                                    const uint32_t *__restrict__ base, void *__restrict__ map) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= tiles) return;
    int lo = 0, hi = count;  // last segment with tile0 <= t (segments without tiles share tile0)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (d[mid].tile0 <= t) lo = mid;
        else hi = mid;
    }
    if (NARROW) static_cast<uint8_t *>(map)[t] = (uint8_t)(lo - (int)base[t / kIdxBlock]);
    else static_cast<int *>(map)[t] = lo;
}

// the byte is read as its aligned dword (a scalar load; a byte load would go through the vector
// memory path and delay the whole tile)
template <bool NARROW>
__device__ inline int tile_segment(unsigned tile, const uint32_t *__restrict__ blk_base, const void *__restrict__ map) {
    return NARROW ? (int)(blk_base[tile / kIdxBlock] +
                          ((static_cast<const uint32_t *>(map)[tile / 4] >> (8 * (tile % 4))) & 0xffu))
                  : static_cast<const int *>(map)[tile];
}

// The tile walk of every operation. An Op says what happens to the data and nothing about where:
//   kUnit             bytes of SegDesc::len per element
//   Op(flat, sd, seg, a...)   the segment's addresses; `a` are the launch's extra arguments
//   vector()          may the lanes move whole 16-byte units (else the tile goes element by element)
//   vec(b)            the 16-byte unit at byte b of the segment (bytes as SegDesc::len counts them)
//   elem(e)           element e of the segment
// Element granular at the edges: a misaligned segment and a segment's last partial unit go element
// by element (the host guarantees whole, aligned elements), never byte by byte unless kUnit is 1.
template <class Op, bool NARROW, class... A>
__global__ void __launch_bounds__(64) k_seg(char *flat, const SegDesc *__restrict__ d,
                                            const uint32_t *__restrict__ blk_base, const void *__restrict__ map,
                                            A... a) {
    constexpr uint64_t kUnit = Op::kUnit;
    const unsigned tile = blockIdx.x;
    const int seg = tile_segment<NARROW>(tile, blk_base, map);
    const SegDesc sd = d[seg];
    const Op op(flat, sd, seg, a...);
    const uint64_t base = (uint64_t)(tile - sd.tile0) * kSegTile;  // tile start inside the segment
    if (!op.vector()) {
        const uint64_t end = (sd.len < base + kSegTile ? sd.len : base + kSegTile) / kUnit;
        for (uint64_t e = base / kUnit + threadIdx.x; e < end; e += 64) op.elem(e);
        return;
    }
    const uint64_t b = base + threadIdx.x * 16;
    if (b + 16 <= sd.len) {
        op.vec(b);
    } else if (b < sd.len) {  // the segment's last partial 16 bytes
        for (uint64_t e = b / kUnit; e < sd.len / kUnit; ++e) op.elem(e);
    }
}

template <class Op, class... A>
void launch(bool narrow, dim3 g, hipStream_t stream, char *fl, const SegDesc *dd, const uint32_t *db, const void *map,
            A... a) {
    if (narrow) hipLaunchKernelGGL((k_seg<Op, true, A...>), g, dim3(64), 0, stream, fl, dd, db, map, a...);
    else hipLaunchKernelGGL((k_seg<Op, false, A...>), g, dim3(64), 0, stream, fl, dd, db, map, a...);
}

// The launch's extra argument of type T, wherever it stands in `a...` (an Op takes its tables through
// one variadic constructor). A launch that does not carry it does not compile.
template <class T, class A0, class... A> __device__ inline T arg_of(A0 a0, A... a) {
    if constexpr (std::is_same_v<T, A0>) return a0;
    else return arg_of<T>(a...);
}

// ---- the scale factors (DDL_ALLREDUCE_SCALE: prescale in the packs, postscale in the unpacks) -------
// Every Op that can scale has a SCALE parameter; SCALE = false is the kernel it was, its argument list
// included. A scaled launch carries one fp32 factor per segment (a const float * behind the launch's
// other arguments: scl[seg], uploaded behind the block bases and the residual addresses); a segment
// flagged kSegScale has every element multiplied by it, a segment without the flag is moved exactly as
// the unscaled Op moves it (no multiply is issued: the bits are untouched). fp32 tensors, and native bf16
// tensors through the 16-bit Ops below (widened, multiplied, narrowed once per kernel). Every
// product is one fp32 operation rounded to nearest even with subnormals kept, and never part of an fma:
// hipcc contracts a * b + c by default, so the multiply is mul_rn, compiled with contraction off.
//   pack:    c = g (x) a, then what the unscaled pack does with c (store / narrow / feedback's c (+) r)
//   unpack:  y = s (widened), y = y (/) (float)P for kSegAvg, y = y (x) b for kSegScale, store y
//   bf16 tensors:  c = narrow(widen(g) (x) a);  store narrow(widen(s) (/) (float)P (x) b): one rounding, at the end
__device__ inline float mul_rn(float x, float a) {
#pragma clang fp contract(off)
    return x * a;
}

// A segment's factor inside a launch: nothing at all when SCALE is false.
template <bool SCALE> struct Factor {
    float a = 1.0f;
    bool on = false;
    template <class... A> __device__ Factor(const SegDesc &sd, int seg, A... x) {
        if constexpr (SCALE) {
            on = (sd.vec & kSegScale) != 0;
            if (on) a = arg_of<const float *>(x...)[seg];
        }
    }
    __device__ float operator()(float x) const { return SCALE && on ? mul_rn(x, a) : x; }
    template <int N> __device__ void operator()(float (&x)[N]) const {
        if (SCALE && on) {
#pragma unroll
            for (int k = 0; k < N; ++k) x[k] = mul_rn(x[k], a);
        }
    }
};

// ---- the plain copies ---------------------------------------------------------------------------
// DIR 0: gather segments -> flat; DIR 1: scatter flat -> segments. Bytes.
template <int DIR> struct CopyOp {
    static constexpr uint32_t kUnit = 1;
    char *fl, *tp;
    bool v;
    __device__ CopyOp(char *flat, const SegDesc &sd, int)
        : fl(flat + sd.off), tp(reinterpret_cast<char *>(sd.ptr)), v((sd.vec & kSegVec) != 0) {}
    __device__ bool vector() const { return v; }
    __device__ void vec(uint64_t b) const {
        const u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>((DIR == 0 ? tp : fl) + b));
        __builtin_nontemporal_store(x, reinterpret_cast<u32x4 *>((DIR == 0 ? fl : tp) + b));
    }
    __device__ void elem(uint64_t e) const {
        if (DIR == 0) fl[e] = tp[e];
        else tp[e] = fl[e];
    }
};

// ---- the dividing scatter (DDL_ALLREDUCE_OP_AVG) ------------------------------------------------
// DivOp: the scatter with the mean's quotient in the store: the elements of a segment flagged
// kSegAvg leave as q(x, P), the others unchanged. The source is the flat buffer (the dividing
// unpack) or, with flat == nullptr, the segment itself (in place: every lane reads and writes its
// own bytes only). A quotient needs whole elements, so kUnit is the dtype's size.
// q: fp32 / fp64 the correctly rounded IEEE quotient by (float)P / (double)P (hipcc's default
// correctly rounded division; subnormals kept, kernel mode float_denorm_mode_32 = 3); fp16 / bf16
// widened to fp32, divided, rounded to nearest even into the type — what numpy and torch CPU
// compute. No reciprocal multiply anywhere: at P = 3, 5, 6, 7 it differs in the last bit for
// about a third of the values.
enum DivType : int { kDivF32 = 0, kDivF64 = 1, kDivF16 = 2, kDivBF16 = 3 };

template <int DT> struct DivTraits;
template <> struct DivTraits<kDivF32> {
    using T = float;
    using D = float;
    static __device__ inline T q(T x, D d) { return x / d; }
};
template <> struct DivTraits<kDivF64> {
    using T = double;
    using D = double;
    static __device__ inline T q(T x, D d) { return x / d; }
};
template <> struct DivTraits<kDivF16> {
    using T = _Float16;
    using D = float;
    static __device__ inline T q(T x, D d) { return (T)((float)x / d); }
};
template <> struct DivTraits<kDivBF16> {
    using T = uint16_t;  // the bits
    using D = float;
    static __device__ inline T q(T x, D d) {
        const float r = __uint_as_float((uint32_t)x << 16) / d;
        const uint32_t u = __float_as_uint(r);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (T)((u >> 16) | 0x40u);  // NaN stays a NaN
        return (T)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);                 // nearest even
    }
};

// What every scatter does to the values on their way into a tensor, written once (DivOp, CvtUnpackOp
// and k_seg_sumsq after their loads and widenings): q(x, P) for a kSegAvg segment, then (SCALE) the
// factor for a kSegScale one. This order is contract.
// A native 16-bit tensor dtype seen as fp32 (the scaled and the counted paths of 16-bit tensors are written
// over this trait): widen is exact, narrow the one rounding to nearest even of the wire of the same format
// (overflow gives inf, a NaN stays a NaN). bfloat16 is the only instance; float16 would be one more.
template <int DT> struct Wide16;
template <> struct Wide16<kDivBF16> {
    using T = DivTraits<kDivBF16>::T;  // the bits
    static __device__ inline float widen(T x) { return __uint_as_float((uint32_t)x << 16); }
    static __device__ inline T narrow(float y) { return __builtin_bit_cast(T, (__bf16)y); }
};
template <int DT> constexpr bool kIs16 = DT == kDivF16 || DT == kDivBF16;

template <int DT, bool SCALE> struct Chain {
    static_assert(!SCALE || DT == kDivF32 || DT == kDivBF16, "scale factors are defined for float32 and bfloat16 tensors");
    using Tr = DivTraits<DT>;
    typename Tr::D dv;
    bool avg;
    Factor<SCALE> fac;
    template <class... A>
    __device__ Chain(const SegDesc &sd, int seg, typename Tr::D divisor, A... a)
        : dv(divisor), avg((sd.vec & kSegAvg) != 0), fac(sd, seg, a...) {}
    template <int N> __device__ void operator()(typename Tr::T (&x)[N]) const {
        if constexpr (SCALE && kIs16<DT>) {
            // 16-bit tensors: widen, quotient, factor, ONE narrowing — never one between the quotient and the
            // factor. A segment without a factor takes the unscaled q (the same bits), a SUM one nothing.
            if (fac.on) {
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    float y = Wide16<DT>::widen(x[k]);
                    if (avg) y = y / dv;
                    x[k] = Wide16<DT>::narrow(mul_rn(y, fac.a));
                }
                return;
            }
        }
        if (avg) {
#pragma unroll
            for (int k = 0; k < N; ++k) x[k] = Tr::q(x[k], dv);
        }
        if constexpr (SCALE && !kIs16<DT>) fac(x);
    }
};

// SCALE (kDivF32, kDivBF16): the scaled scatter, with the factor table behind the divisor.
template <int DT, bool SCALE = false> struct DivOp {
    using T = typename DivTraits<DT>::T;
    static constexpr uint32_t kUnit = sizeof(T);
    union Vec {
        u32x4 v;
        T e[16 / sizeof(T)];
    };
    char *tp;
    const char *sp;
    Chain<DT, SCALE> val;
    bool v;
    template <class... A>
    __device__ DivOp(const char *flat, const SegDesc &sd, int seg, double divisor, A... a)
        : tp(reinterpret_cast<char *>(sd.ptr)), sp(flat ? flat + sd.off : tp),
          val(sd, seg, (typename DivTraits<DT>::D)divisor, a...), v((sd.vec & kSegVec) != 0) {}
    __device__ bool vector() const { return v; }
    __device__ void vec(uint64_t b) const {
        Vec x;
        x.v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(sp + b));
        val(x.e);
        __builtin_nontemporal_store(x.v, reinterpret_cast<u32x4 *>(tp + b));
    }
    __device__ void elem(uint64_t e) const {
        T x[1] = {reinterpret_cast<const T *>(sp)[e]};
        val(x);
        reinterpret_cast<T *>(tp)[e] = x[0];
    }
};

// ---- the converting copies (ddl_allreduce_wire: fp32 tensors, 16-bit flat buffer) -----------------
// CvtPackOp / CvtUnpackOp: the tiles are defined on the WIRE side. SegDesc::len / off and the 1 KiB
// tile count wire bytes (512 elements), so the segment table, the tile index and flat_bytes are
// those of a plain copy of the wire stream; the tensor side of a tile is 2 KiB of fp32. A lane
// handles 8 elements: two 16-byte fp32 vectors on the tensor side, one 16-byte wire vector on the
// flat side (6 bytes moved per element against the plain copy's 8); vec(b) takes the wire byte b
// of the lane's vector, the tensor's byte 2b.
// Pack: round to nearest even — the plain fptrunc, which hipcc lowers for gfx950 to v_cvt_pk_f16_f32
// (the kernel's rounding mode, nearest even; NOT the round-toward-zero v_cvt_pkrtz_f16_f32; overflow
// gives inf, subnormals are kept: the kernel's fp16 denormal mode) and to v_cvt_pk_bf16_f32, the
// hardware's packed RNE conversion (profiles/wire_compress/kernel_resource_usage.txt); a NaN stays a
// NaN in both. Unpack: widen (exact) and, for a kSegAvg segment, the correctly rounded fp32 quotient
// by (float)P — true division, as DivOp. A tensor that is only 4-byte aligned and a segment's last
// partial vector go element by element.
enum WireType : int { kWireF16 = 0, kWireBF16 = 1 };
template <int WIRE> struct WireTraits;
template <> struct WireTraits<kWireF16> {
    using T = _Float16;
    static __device__ inline T narrow(float x) { return (T)x; }
    static __device__ inline float widen(T x) { return (float)x; }
};
template <> struct WireTraits<kWireBF16> {
    using T = __bf16;
    static __device__ inline T narrow(float x) { return (T)x; }
    static __device__ inline float widen(T x) { return (float)x; }
};
union F32x4 {
    u32x4 v;
    float e[4];
};
template <class T> union Wire8 {
    u32x4 v;
    T e[8];
};

// ---- the converting pack with error feedback (DDL_ALLREDUCE_WIRE_FEEDBACK) -----------------------
// CvtPackOp<WIRE, true>: the converting pack plus one table of residual addresses, res[seg] (0: the
// segment is converted as CvtPackOp<WIRE, false> converts it). Per element of a segment with a
// residual r (fp32, the segment's element count, indexed like the tensor):
//     v = g + r;  w = narrow(v);  r' = isfinite(widen(w)) ? v - widen(w) : 0
// w goes to the flat buffer, r' replaces r. One fp32 rounding (g + r, nearest even, subnormals kept)
// beyond the wire's own: v - widen(w) is exact whenever widen(w) is finite. A NaN or inf in v, or
// an overflow of the narrowing, clears the residual. The plain feedback pack has no multiply, so nothing
// can contract; the scaled one (SCALE) multiplies first, through mul_rn, whose product is
// rounded on its own and never fuses with this addition. No reciprocal. Moves 14 bytes per element against the plain converting pack's 6: the vector path
// (tensor AND residual 16-byte aligned) is two 16-byte loads from each, one 16-byte wire store and
// two 16-byte residual stores. The tensor loads and all stores are non-temporal (the residual is
// next read a whole step later); the residual LOADS are plain: with non-temporal loads of both read
// streams the C5 set took 1.73 ms against 1.49-1.53 ms (profiles/wire_feedback/feedback_probe_nt_loads.json
// against feedback_probe.json). Otherwise, and for a segment's last partial vector, element by
// element. FB = false takes no table and stays its own, smaller kernel.
template <int WIRE>
__device__ inline typename WireTraits<WIRE>::T feedback(float g, float &r) {
    using Tr = WireTraits<WIRE>;
    const float v = g + r;
    const typename Tr::T w = Tr::narrow(v);
    const float wf = Tr::widen(w);
    r = __builtin_isfinite(wf) ? v - wf : 0.0f;
    return w;
}

// SCALE: the product ahead of the narrowing (FB: ahead of the residual's addition, so the residual is in
// prescaled units); the factor table behind the residual table.
template <int WIRE, bool FB, bool SCALE = false> struct CvtPackOp {
    using Tr = WireTraits<WIRE>;
    using T = typename Tr::T;
    static constexpr uint32_t kUnit = sizeof(T);
    T *fl;
    const float *tp;
    float *rs;
    bool v;
    Factor<SCALE> fac;
    template <class... A>
    __device__ CvtPackOp(char *flat, const SegDesc &sd, int seg, A... a)
        : fl(reinterpret_cast<T *>(flat + sd.off)), tp(reinterpret_cast<const float *>(sd.ptr)), rs(nullptr),
          v((sd.vec & kSegVec) != 0), fac(sd, seg, a...) {
        if constexpr (FB) {  // tensor or residual only 4-byte aligned: elements
            const uint64_t r = arg_of<const uint64_t *>(a...)[seg];
            rs = reinterpret_cast<float *>(r);
            v = v && (r & 15u) == 0;
        }
    }
    __device__ bool vector() const { return v; }
    __device__ void vec(uint64_t b) const {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(tp + b / sizeof(T));
        F32x4 lo, hi;
        lo.v = __builtin_nontemporal_load(src);
        hi.v = __builtin_nontemporal_load(src + 1);
        fac(lo.e);
        fac(hi.e);
        Wire8<T> o;
        if (FB && rs) {
            u32x4 *rv = reinterpret_cast<u32x4 *>(rs + b / sizeof(T));
            F32x4 rlo, rhi;
            rlo.v = rv[0];  // plain loads: measured faster than non-temporal ones (above)
            rhi.v = rv[1];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o.e[k] = feedback<WIRE>(lo.e[k], rlo.e[k]);
                o.e[4 + k] = feedback<WIRE>(hi.e[k], rhi.e[k]);
            }
            __builtin_nontemporal_store(rlo.v, rv);
            __builtin_nontemporal_store(rhi.v, rv + 1);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o.e[k] = Tr::narrow(lo.e[k]);
                o.e[4 + k] = Tr::narrow(hi.e[k]);
            }
        }
        __builtin_nontemporal_store(o.v, reinterpret_cast<u32x4 *>(reinterpret_cast<char *>(fl) + b));
    }
    __device__ void elem(uint64_t e) const {
        if (FB && rs) {
            float r = rs[e];
            fl[e] = feedback<WIRE>(fac(tp[e]), r);
            rs[e] = r;
        } else {
            fl[e] = Tr::narrow(fac(tp[e]));
        }
    }
};

// ---- the converting pack with stochastic rounding (DDL_ALLREDUCE_WIRE_STOCHASTIC) -----------------
// CvtPackSrOp: the bf16 converting pack plus one table of WireStream, st[seg]. A segment whose entry is
// not `on` is converted as CvtPackOp<kWireBF16, false> converts it. Per element i of a stochastic
// segment's REQUEST (i = st[seg].first + the element's index in the segment), with u the bits of c:
//     c NaN or inf:  w = narrow(c)                       round to nearest even, as the plain pack
//     otherwise:     w = (u + R(S, i)) >> 16             R: 16 bits, below
// The sign never changes, +-0 stays +-0, subnormals need no case of their own, and a finite c above the
// largest bf16 value carries into inf with the probability its low half gives. Integer arithmetic only.
// R(S, i): one 32-bit word per element pair j = i >> 1,
//     x = fmix32(lo32(j) ^ lo32(S));  x = fmix32(x + hi32(S) + hi32(j) * 0x9e3779b9)
// (fmix32: MurmurHash3's finaliser), element i taking bits 16 (i & 1) .. + 15. Four 32-bit multiplies per
// word, two per element: the vector path computes the lane's 4 words (5 where the piece starts at an odd
// index of its request — uniform over the segment), 16-20 multiplies for 48 bytes moved, against the
// ~10 B/clk/CU the HBM-bound stream sustains. hi32(j) * 0x9e3779b9 is one multiply per lane: the words
// behind a carry of lo32(j) take that product plus the constant. Same loads and stores as the plain
// pack: two 16-byte non-temporal loads, one 16-byte non-temporal store; 6 bytes per element.
__device__ inline uint32_t fmix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}
constexpr uint32_t kSrGolden = 0x9e3779b9u;
// the word of pair j: lo = lo32(j), c = hi32(S) + hi32(j) * kSrGolden
__device__ inline uint32_t sr_word(uint32_t s_lo, uint32_t lo, uint32_t c) { return fmix32(fmix32(lo ^ s_lo) + c); }
__device__ inline uint16_t sr_narrow(float c, uint32_t r16) {
    const uint32_t u = __float_as_uint(c);
    if ((u & 0x7f800000u) == 0x7f800000u) return __builtin_bit_cast(uint16_t, (__bf16)c);
    return (uint16_t)((u + r16) >> 16);
}

// FB: the launch also holds error-feedback segments (a plan may mix requests of both kinds; a segment is
// never both): the residual table ahead of the streams, a segment with a residual packed as
// CvtPackOp<kWireBF16, true> packs it.
template <bool SCALE = false, bool FB = false> struct CvtPackSrOp {
    using Tr = WireTraits<kWireBF16>;
    using T = typename Tr::T;
    static constexpr uint32_t kUnit = sizeof(T);
    T *fl;
    const float *tp;
    float *rs = nullptr;
    bool v, on;
    uint64_t S, first;
    Factor<SCALE> fac;
    template <class... A>
    __device__ CvtPackSrOp(char *flat, const SegDesc &sd, int seg, A... a)
        : fl(reinterpret_cast<T *>(flat + sd.off)), tp(reinterpret_cast<const float *>(sd.ptr)),
          v((sd.vec & kSegVec) != 0), fac(sd, seg, a...) {
        const WireStream st = arg_of<const WireStream *>(a...)[seg];
        on = st.on != 0;
        S = st.key;
        first = st.first;
        if constexpr (FB) {  // tensor or residual only 4-byte aligned: elements
            const uint64_t r = arg_of<const uint64_t *>(a...)[seg];
            rs = reinterpret_cast<float *>(r);
            v = v && (r & 15u) == 0;
            on = on && !rs;
        }
    }
    __device__ bool vector() const { return v; }
    __device__ void vec(uint64_t b) const {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(tp + b / sizeof(T));
        F32x4 lo, hi;
        lo.v = __builtin_nontemporal_load(src);
        hi.v = __builtin_nontemporal_load(src + 1);
        fac(lo.e);
        fac(hi.e);
        union {
            u32x4 v;
            uint16_t e[8];
        } o;
        if (FB && rs) {
            u32x4 *rv = reinterpret_cast<u32x4 *>(rs + b / sizeof(T));
            F32x4 rlo, rhi;
            rlo.v = rv[0];
            rhi.v = rv[1];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o.e[k] = __builtin_bit_cast(uint16_t, feedback<kWireBF16>(lo.e[k], rlo.e[k]));
                o.e[4 + k] = __builtin_bit_cast(uint16_t, feedback<kWireBF16>(hi.e[k], rhi.e[k]));
            }
            __builtin_nontemporal_store(rlo.v, rv);
            __builtin_nontemporal_store(rhi.v, rv + 1);
        } else if (on) {
            const uint64_t i0 = first + b / sizeof(T), j0 = i0 >> 1;
            const bool odd = (i0 & 1u) != 0;  // uniform: b / 2 is a multiple of 8
            const uint32_t s_lo = (uint32_t)S, l0 = (uint32_t)j0;
            const uint32_t c0 = (uint32_t)(S >> 32) + (uint32_t)(j0 >> 32) * kSrGolden, c1 = c0 + kSrGolden;
            uint32_t w[5];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) w[k] = sr_word(s_lo, l0 + k, l0 + k < l0 ? c1 : c0);
            w[4] = odd ? sr_word(s_lo, l0 + 4, l0 + 4 < l0 ? c1 : c0) : 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                // element k is half (k & 1) of word k / 2, or with an odd start half ((k + 1) & 1) of word (k + 1) / 2
                const uint32_t even = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
                const uint32_t shifted = (w[(k + 1) >> 1] >> (16 * ((k + 1) & 1))) & 0xffffu;
                o.e[k] = sr_narrow(k < 4 ? lo.e[k] : hi.e[k - 4], odd ? shifted : even);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o.e[k] = __builtin_bit_cast(uint16_t, Tr::narrow(lo.e[k]));
                o.e[4 + k] = __builtin_bit_cast(uint16_t, Tr::narrow(hi.e[k]));
            }
        }
        __builtin_nontemporal_store(o.v, reinterpret_cast<u32x4 *>(reinterpret_cast<char *>(fl) + b));
    }
    __device__ void elem(uint64_t e) const {
        const float c = fac(tp[e]);
        if (FB && rs) {
            float r = rs[e];
            fl[e] = feedback<kWireBF16>(c, r);
            rs[e] = r;
        } else if (on) {
            const uint64_t i = first + e, j = i >> 1;
            const uint32_t x = sr_word((uint32_t)S, (uint32_t)j, (uint32_t)(S >> 32) + (uint32_t)(j >> 32) * kSrGolden);
            reinterpret_cast<uint16_t *>(fl)[e] = sr_narrow(c, (x >> (16 * (uint32_t)(i & 1u))) & 0xffffu);
        } else {
            fl[e] = Tr::narrow(c);
        }
    }
};

// SCALE: the factor behind the quotient; the factor table behind the divisor.
template <int WIRE, bool SCALE = false> struct CvtUnpackOp {
    using Tr = WireTraits<WIRE>;
    using T = typename Tr::T;
    static constexpr uint32_t kUnit = sizeof(T);
    union F32x8 {
        u32x4 v[2];
        float e[8];
    };
    const T *fl;
    float *tp;
    Chain<kDivF32, SCALE> val;
    bool v;
    template <class... A>
    __device__ CvtUnpackOp(const char *flat, const SegDesc &sd, int seg, float dv, A... a)
        : fl(reinterpret_cast<const T *>(flat + sd.off)), tp(reinterpret_cast<float *>(sd.ptr)), val(sd, seg, dv, a...),
          v((sd.vec & kSegVec) != 0) {}
    __device__ bool vector() const { return v; }
    __device__ void vec(uint64_t b) const {
        Wire8<T> x;
        x.v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(fl) + b));
        F32x8 y;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            y.e[k] = Tr::widen(x.e[k]);
            y.e[4 + k] = Tr::widen(x.e[4 + k]);
        }
        val(y.e);
        u32x4 *dst = reinterpret_cast<u32x4 *>(tp + b / sizeof(T));
        __builtin_nontemporal_store(y.v[0], dst);
        __builtin_nontemporal_store(y.v[1], dst + 1);
    }
    __device__ void elem(uint64_t e) const {
        float y[1] = {Tr::widen(fl[e])};
        val(y);
        tp[e] = y[0];
    }
};

// ---- the e4m3 wire (DDL_ALLREDUCE_WIRE_E4M3: fp32 tensors, 256-byte granules in the flat buffer) ----
// Q8PackOp / Q8UnpackOp: the tiles are defined on the WIRE side, as the converting copies': SegDesc::len / off
// count granule bytes (whole granules: len is a multiple of 256, so the walk takes every lane through vec()
// and a 16-lane row — one granule — is always whole), a 1 KiB tile is 4 granules and 1008 elements. The
// tensor side is not len x a constant at the tail, so the launch carries one SegElems per segment: the true
// element count. The lane whose unit is wire byte b works on granule b / 256 at row position r = b / 16 % 16.
// The mapping follows the TENSOR side, which moves four fifths of the bytes: a granule's 252 elements are 63
// 16-byte fp32 vectors, and lane r takes vectors r, 16 + r, 32 + r, 48 + r (vector 63 does not exist: lane
// 15 takes three), so each of the four load / store instructions of a row covers 256 contiguous tensor bytes
// (a first version gave lane r the 16 consecutive elements of its own wire unit, 64-byte strides between the
// lanes of one instruction: the unpack took 3.98 and the pack 1.26 of their bf16 counterparts' time,
// profiles/wire_e4m3/e4m3_probe_lane_contiguous.json). The codes of vector v are wire dword v of the granule:
// four dword accesses per lane, 64 contiguous bytes per row each; dword 63 — lane 15's fourth — is the scale.
// A tensor that is only 4-byte aligned and the vectors over the request's tail go element by element, elements
// past the end counting as +0.0. 4 + 256/252 bytes moved per element. The rule itself — amax over the row, the
// scale, the rounding, the NaN code — is e4m3.h's quantize_row; the prescale (SCALE) ahead of it through mul_rn.
// Unpack: code x scale (every lane loads its granule's scale dword), then Chain: AVG's quotient, the postscale.
struct SegElems {
    uint64_t n;
};

// FB (DDL_ALLREDUCE_WIRE_E4M3_FEEDBACK; the rule is ddl_amd.h's "Error feedback of the e4m3 wire"): the pack plus one
// table of residual addresses, res[seg], behind the element counts (0: the segment is packed exactly as
// Q8PackOp<SCALE, false> packs it). A lane reads and writes the residual with the tensor's mapping — vectors r,
// 16 + r, 32 + r, 48 + r of the granule, 256 contiguous bytes per row and instruction — so the lane that loaded
// v[k] holds its code when encode_row returns, and row_scale_exponent left the scale on every lane: it decodes its own four
// dwords (dequantize) and stores v (-) code * s, +0.0 where that is not finite (a NaN or an infinity in v, or a code
// that decodes to one: 256 * 2^120 and up). The residual moves as 16-byte
// vectors wherever it is 16-byte aligned and the vector lies inside the request (every piece of a cut request
// starts a multiple of 1008 bytes into a hipMalloc'd array), whatever the tensor's alignment, else element by
// element; nothing at or past n is read or written. Loads of the residual are plain, its stores non-temporal, as
// CvtPackOp<WIRE, true>'s. 4 + 4 + 4 + 256/252 bytes moved per element. c (+) r never contracts with the prescale
// (mul_rn), v (-) d never with the decode (mul1). FB = false takes no table and stays its own kernel.
template <bool SCALE = false, bool FB = false> struct Q8PackOp {
    static constexpr uint32_t kUnit = 1;
    char *fl;
    const float *tp;
    float *rs = nullptr;
    uint64_t n;
    bool v, rv = false;
    Factor<SCALE> fac;
    template <class... A>
    __device__ Q8PackOp(char *flat, const SegDesc &sd, int seg, A... a)
        : fl(flat + sd.off), tp(reinterpret_cast<const float *>(sd.ptr)), n(arg_of<const SegElems *>(a...)[seg].n),
          v((sd.vec & kSegVec) != 0), fac(sd, seg, a...) {
        if constexpr (FB) {
            const uint64_t r = arg_of<const uint64_t *>(a...)[seg];
            rs = reinterpret_cast<float *>(r);
            rv = (r & 15u) == 0;
        }
    }
    __device__ bool vector() const { return true; }  // whole granules: the edges are the tensor side's, below
    __device__ void vec(uint64_t b) const {
        if constexpr (FB) {
            if (rs) return vec_fb(b);
        }
        const int r = (int)(b >> 4) & 15;
        const uint64_t g0 = (b >> 8) * kE4m3Elems;  // the granule's first element
        float x[16];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int vi = 16 * h + r;  // the granule's vector
            const uint64_t e = g0 + (uint64_t)vi * 4;
            F32x4 q;
            q.v = u32x4{0, 0, 0, 0};
            if (vi < 63) {
                if (v && e + 4 <= n) {
                    q.v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(tp + e));
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (e + k < n) q.e[k] = __builtin_nontemporal_load(tp + e + k);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) x[4 * h + k] = q.e[k];
        }
        fac(x);
        const u32x4 w = e4m3::quantize_row(x, r);
        uint32_t *dst = reinterpret_cast<uint32_t *>(fl + (b & ~uint64_t(255))) + r;
#pragma unroll
        for (int h = 0; h < 4; ++h) __builtin_nontemporal_store(w[h], dst + 16 * h);
    }
    // the lane's share of a granule of `p` (the tensor, non-temporal; the residual, plain loads): vectors where
    // `whole` and inside the request, else elements; +0.0 past n
    template <bool NT> __device__ void gather(const float *p, bool whole, uint64_t g0, int r, float (&x)[16]) const {
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int vi = 16 * h + r;
            const uint64_t e = g0 + (uint64_t)vi * 4;
            F32x4 q;
            q.v = u32x4{0, 0, 0, 0};
            if (vi < 63) {
                if (whole && e + 4 <= n) {
                    const u32x4 *src = reinterpret_cast<const u32x4 *>(p + e);
                    q.v = NT ? __builtin_nontemporal_load(src) : *src;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (e + k < n) q.e[k] = NT ? __builtin_nontemporal_load(p + e + k) : p[e + k];
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) x[4 * h + k] = q.e[k];
        }
    }
    __device__ void vec_fb(uint64_t b) const {  // a segment with a residual
        const int r = (int)(b >> 4) & 15;
        const uint64_t g0 = (b >> 8) * kE4m3Elems;
        float x[16], q[16];
        gather<true>(tp, v, g0, r, x);
        gather<false>(rs, rv, g0, r, q);
        fac(x);
#pragma unroll
        for (int k = 0; k < 16; ++k) x[k] = x[k] + q[k];  // v = c (+) r
        const uint32_t se = e4m3::row_scale_exponent(x, r);
        const u32x4 w = e4m3::encode_row(x, r, se);
        uint32_t *dst = reinterpret_cast<uint32_t *>(fl + (b & ~uint64_t(255))) + r;
#pragma unroll
        for (int h = 0; h < 4; ++h) __builtin_nontemporal_store(w[h], dst + 16 * h);
        float d[16];  // what the fold / the unpack will read (lane 15's d[12..15] decode the scale dword: unused)
        e4m3::dequantize(w, __uint_as_float(se << 23), d);
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int vi = 16 * h + r;
            const uint64_t e = g0 + (uint64_t)vi * 4;
            if (vi >= 63) continue;
            F32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // not finite: v is a NaN or an infinity, or d is (256 * 2^120 and up: a finite v past 248 * 2^120)
                const float y = x[4 * h + k] - d[4 * h + k];
                o.e[k] = (__float_as_uint(y) & 0x7fffffffu) < 0x7f800000u ? y : 0.0f;
            }
            if (rv && e + 4 <= n) {
                __builtin_nontemporal_store(o.v, reinterpret_cast<u32x4 *>(rs + e));
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (e + k < n) __builtin_nontemporal_store(o.e[k], rs + e + k);
            }
        }
    }
    __device__ void elem(uint64_t) const {}
};

template <bool SCALE = false> struct Q8UnpackOp {
    static constexpr uint32_t kUnit = 1;
    const char *fl;
    float *tp;
    uint64_t n;
    Chain<kDivF32, SCALE> val;
    bool v;
    template <class... A>
    __device__ Q8UnpackOp(const char *flat, const SegDesc &sd, int seg, float dv, A... a)
        : fl(flat + sd.off), tp(reinterpret_cast<float *>(sd.ptr)), n(arg_of<const SegElems *>(a...)[seg].n),
          val(sd, seg, dv, a...), v((sd.vec & kSegVec) != 0) {}
    __device__ bool vector() const { return true; }
    __device__ void vec(uint64_t b) const {
        const int r = (int)(b >> 4) & 15;
        const uint64_t g0 = (b >> 8) * kE4m3Elems;
        const uint32_t *src = reinterpret_cast<const uint32_t *>(fl + (b & ~uint64_t(255)));
        u32x4 raw;
#pragma unroll
        for (int h = 0; h < 4; ++h) raw[h] = __builtin_nontemporal_load(src + 16 * h + r);
        const float s = __uint_as_float(__builtin_nontemporal_load(src + 63));
        float y[16];
        e4m3::dequantize(raw, s, y);
        val(y);
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int vi = 16 * h + r;
            const uint64_t e = g0 + (uint64_t)vi * 4;
            if (vi >= 63) continue;
            if (v && e + 4 <= n) {
                F32x4 q;
#pragma unroll
                for (int k = 0; k < 4; ++k) q.e[k] = y[4 * h + k];
                __builtin_nontemporal_store(q.v, reinterpret_cast<u32x4 *>(tp + e));
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (e + k < n) __builtin_nontemporal_store(y[4 * h + k], tp + e + k);
            }
        }
    }
    __device__ void elem(uint64_t) const {}
};

// ScaleGatherOp: the uncompressed prescale, tensor -> flat. Whole fp32 elements (kUnit 4): CopyOp moves
// bytes, so it has no twin to fold into.
struct ScaleGatherOp {
    static constexpr uint32_t kUnit = 4;
    float *fl;
    const float *tp;
    float a;
    bool sc, v;
    __device__ ScaleGatherOp(char *flat, const SegDesc &sd, int seg, const float *__restrict__ scl)
        : fl(reinterpret_cast<float *>(flat + sd.off)), tp(reinterpret_cast<const float *>(sd.ptr)),
          sc((sd.vec & kSegScale) != 0), v((sd.vec & kSegVec) != 0) {
        a = sc ? scl[seg] : 1.0f;
    }
    __device__ bool vector() const { return v; }
    __device__ void vec(uint64_t b) const {
        F32x4 x;
        x.v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(tp) + b));
        if (sc) {
#pragma unroll
            for (int k = 0; k < 4; ++k) x.e[k] = mul_rn(x.e[k], a);
        }
        __builtin_nontemporal_store(x.v, reinterpret_cast<u32x4 *>(reinterpret_cast<char *>(fl) + b));
    }
    __device__ void elem(uint64_t e) const { fl[e] = sc ? mul_rn(tp[e], a) : tp[e]; }
};

// ScaleGather16Op: the prescale of native 16-bit tensors, tensor -> flat: c = narrow(widen(g) (x) a) for a
// kSegScale segment, the bits moved untouched for any other. Whole 16-bit elements (kUnit 2). The vector path
// is one 16-byte load, 8 x widen / mul_rn / narrow and one 16-byte store; a tensor that is only 2-byte aligned
// and a segment's last partial unit go element by element. 4 bytes moved per element, as the plain copy.
template <int DT> struct ScaleGather16Op {
    using W = Wide16<DT>;
    using T = typename W::T;
    static constexpr uint32_t kUnit = sizeof(T);
    T *fl;
    const T *tp;
    float a;
    bool sc, v;
    __device__ ScaleGather16Op(char *flat, const SegDesc &sd, int seg, const float *__restrict__ scl)
        : fl(reinterpret_cast<T *>(flat + sd.off)), tp(reinterpret_cast<const T *>(sd.ptr)),
          sc((sd.vec & kSegScale) != 0), v((sd.vec & kSegVec) != 0) {
        a = sc ? scl[seg] : 1.0f;
    }
    __device__ bool vector() const { return v; }
    __device__ void vec(uint64_t b) const {
        Wire8<T> x;
        x.v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(tp) + b));
        if (sc) {
#pragma unroll
            for (int k = 0; k < 8; ++k) x.e[k] = W::narrow(mul_rn(W::widen(x.e[k]), a));
        }
        __builtin_nontemporal_store(x.v, reinterpret_cast<u32x4 *>(reinterpret_cast<char *>(fl) + b));
    }
    __device__ void elem(uint64_t e) const { fl[e] = sc ? W::narrow(mul_rn(W::widen(tp[e]), a)) : tp[e]; }
};

// ---- the unpacks with the sum of squares (DDL_ALLREDUCE_SUMSQ) -----------------------------
// k_seg_sumsq: the plain, the dividing (WIRE < 0: fp32 flat buffer, DivOp<kDivF32>'s quotient) and the
// converting scatter (WIRE = kWireF16 / kWireBF16: CvtUnpackOp's widening and quotient) of fp32
// tensors that also leave, for every tile of a segment flagged kSegStat, the fp64 sum of the squares
// of the fp32 values the tile stored in partials[tile]. Launched only when some segment of the launch
// carries the flag; a segment without it is stored as k_seg stores it and writes no partial. SCALE: the
// factor of a kSegScale segment behind the quotient, ahead of the store and the squares (the statistic is
// of what is stored); the factor table is the launch's one extra argument. Scatters only (flat != nullptr).
// The order of the additions (include/ddl_amd.h, tests/_sumsq_helpers.py): T = 256 elements per tile
// and E = 4 per lane (WIRE < 0), or T = 512 and E = 8. Lane l of tile t owns elements
// t*T + l*E .. + E-1 of the segment WHATEVER the tensor's alignment: acc = +0.0, acc += x*x left to
// right in fp64 (x*x is exact in fp64 for every fp32 x, so an fma contraction of acc + x*x changes no
// bit), elements past the segment's end count as +0.0; then the butterfly s[l] += s[l ^ d] for
// d = 32, 16, 8, 4, 2, 1 (every lane ends with the same bits: each step adds the same two numbers on
// both sides); lane 0 writes the tile's partial. The finishing kernels below combine the partials in
// groups of 4096. No atomic anywhere.
// The flat side of a lane's E elements is one aligned 16-byte unit inside the segment's 256-byte
// padded slot, so it is always one vector load; the tensor side is vector stores where the tensor is
// 16-byte aligned and the lane holds E whole elements, else element by element.
// flat == nullptr: in place and read-only — the same reduction over tensors that already hold their
// results (nothing is divided or stored), the same lanes owning the same elements.
__device__ inline double wave_sum(double s) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    return s;
}

template <int WIRE, bool NARROW, bool SCALE, class... A>
__device__ __forceinline__ void seg_sumsq(const char *flat, const SegDesc *__restrict__ d,
                                          const uint32_t *__restrict__ blk_base, const void *__restrict__ map,
                                          float divisor, double *__restrict__ partials, A... a) {
    constexpr int E = WIRE < 0 ? 4 : 8;
    constexpr uint64_t kUnit = WIRE < 0 ? 4 : 2;  // bytes of SegDesc::len per element
    const unsigned tile = blockIdx.x;
    const int seg = tile_segment<NARROW>(tile, blk_base, map);
    const SegDesc sd = d[seg];
    const uint64_t n = sd.len / kUnit;
    const uint64_t e0 = (uint64_t)(tile - sd.tile0) * (kSegTile / kUnit) + threadIdx.x * E;
    const int nv = e0 >= n ? 0 : n - e0 < (uint64_t)E ? (int)(n - e0) : E;  // the lane's elements inside the segment
    float *tp = reinterpret_cast<float *>(sd.ptr) + e0;
    const bool whole = (sd.vec & kSegVec) != 0 && nv == E;
    float x[E];
#pragma unroll
    for (int k = 0; k < E; ++k) x[k] = 0.0f;
    if (flat) {
        if (nv > 0) {
            const u32x4 raw = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(flat + sd.off + e0 * kUnit));
            if constexpr (WIRE < 0) {
                F32x4 v;
                v.v = raw;
#pragma unroll
                for (int k = 0; k < E; ++k) x[k] = v.e[k];
            } else {
                Wire8<typename WireTraits<WIRE>::T> w;
                w.v = raw;
#pragma unroll
                for (int k = 0; k < E; ++k) x[k] = WireTraits<WIRE>::widen(w.e[k]);
            }
            Chain<kDivF32, SCALE>(sd, seg, divisor, a...)(x);
            if (whole) {
#pragma unroll
                for (int h = 0; h < E / 4; ++h) {
                    F32x4 o;
#pragma unroll
                    for (int k = 0; k < 4; ++k) o.e[k] = x[4 * h + k];
                    __builtin_nontemporal_store(o.v, reinterpret_cast<u32x4 *>(tp) + h);
                }
            } else {
#pragma unroll
                for (int k = 0; k < E; ++k)
                    if (k < nv) tp[k] = x[k];
            }
        }
    } else if (whole) {
#pragma unroll
        for (int h = 0; h < E / 4; ++h) {
            F32x4 v;
            v.v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(tp) + h);
#pragma unroll
            for (int k = 0; k < 4; ++k) x[4 * h + k] = v.e[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < E; ++k)
            if (k < nv) x[k] = tp[k];
    }
    if (!(sd.vec & kSegStat)) return;  // (the whole workgroup: one segment per tile)
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const double v = (double)x[k];
        acc += k < nv ? v * v : 0.0;
    }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) partials[tile] = acc;
}

// (the walk stays a function inlined into its kernel: written as the kernel itself, hipcc emits the
// same additions with their operands swapped, and the unscaled code objects are to stay as they are)
template <int WIRE, bool NARROW, bool SCALE, class... A>
__global__ void __launch_bounds__(64) k_seg_sumsq(const char *flat, const SegDesc *__restrict__ d,
                                                  const uint32_t *__restrict__ blk_base, const void *__restrict__ map,
                                                  float divisor, double *__restrict__ partials, A... a) {
    seg_sumsq<WIRE, NARROW, SCALE>(flat, d, blk_base, map, divisor, partials, a...);
}

// k_seg_sumsq16: the same for native 16-bit tensors (DT: kDivBF16) — 16-bit flat buffer, 16-bit tensors, the
// 2-byte layout of the order above: T = 512 elements per tile, E = 8 per lane. The scatter stores what
// DivOp<DT, SCALE> stores (Chain: the unscaled quotient, or widen / quotient / factor / one narrowing; a SUM
// segment without a factor its bytes) and squares widen(stored element): the statistic is of what is in the
// tensor, so it is finite exactly when every stored element is. Both sides of a lane's 8 elements are one
// 16-byte unit: the flat side always, the tensor side where the tensor is 16-byte aligned and the lane holds 8
// whole elements, else element by element. flat == nullptr: in place and read-only, as above.
template <int DT, bool NARROW, bool SCALE, class... A>
__global__ void __launch_bounds__(64) k_seg_sumsq16(const char *flat, const SegDesc *__restrict__ d,
                                                    const uint32_t *__restrict__ blk_base, const void *__restrict__ map,
                                                    float divisor, double *__restrict__ partials, A... a) {
    using W = Wide16<DT>;
    using T = typename W::T;
    constexpr int E = 8;
    const unsigned tile = blockIdx.x;
    const int seg = tile_segment<NARROW>(tile, blk_base, map);
    const SegDesc sd = d[seg];
    const uint64_t n = sd.len / sizeof(T);
    const uint64_t e0 = (uint64_t)(tile - sd.tile0) * (kSegTile / sizeof(T)) + threadIdx.x * E;
    const int nv = e0 >= n ? 0 : n - e0 < (uint64_t)E ? (int)(n - e0) : E;  // the lane's elements inside the segment
    T *tp = reinterpret_cast<T *>(sd.ptr) + e0;
    const bool whole = (sd.vec & kSegVec) != 0 && nv == E;
    Wire8<T> x;
#pragma unroll
    for (int k = 0; k < E; ++k) x.e[k] = 0;
    if (flat) {
        if (nv > 0) {
            x.v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(flat + sd.off + e0 * sizeof(T)));
            Chain<DT, SCALE>(sd, seg, divisor, a...)(x.e);
            if (whole) {
                __builtin_nontemporal_store(x.v, reinterpret_cast<u32x4 *>(tp));
            } else {
#pragma unroll
                for (int k = 0; k < E; ++k)
                    if (k < nv) tp[k] = x.e[k];
            }
        }
    } else if (whole) {
        x.v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(tp));
    } else {
#pragma unroll
        for (int k = 0; k < E; ++k)
            if (k < nv) x.e[k] = tp[k];
    }
    if (!(sd.vec & kSegStat)) return;  // (the whole workgroup: one segment per tile)
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const double v = (double)W::widen(x.e[k]);
        acc += k < nv ? v * v : 0.0;
    }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) partials[tile] = acc;
}

// The finishing kernels: a segment's tile partials (nt of them, contiguous from tile0) into out[seg], in a
// fixed order that only nt decides. A GROUP is up to kFinGroup = 4096 consecutive values: lane l adds
// values l, l + 64, l + 128, ... of the group to +0.0 in that order (at most 64 additions), then the
// butterfly of k_seg_sumsq gives the group's value. k_sumsq_finish reduces every group of the
// partials (one workgroup per (segment, group): a 256 MiB segment is 64 independent groups, not one
// lane chain of 4096 dependent loads); a segment of one group is finished by it. k_sumsq_finish2
// reduces the group values of a longer segment, themselves one group (nt <= 4096^2: pieces up to
// 16 GiB, checked on the host). A segment without kSegStat gets +0.0.
// Group values of segment seg sit at lvl[tile0 / 4096 + seg + g]: distinct for distinct (seg, g).
constexpr uint64_t kFinGroup = 4096;

__device__ inline double group_sum(const double *__restrict__ v, uint64_t m) {
    double acc = 0.0;
#pragma unroll 8
    for (uint64_t t = threadIdx.x; t < m; t += 64) acc += v[t];
    return wave_sum(acc);
}

__global__ void __launch_bounds__(64) k_sumsq_finish(const SegDesc *__restrict__ d, const double *__restrict__ partials,
                                                     double *__restrict__ lvl, double *__restrict__ out) {
    const unsigned seg = blockIdx.x;
    const uint64_t g = blockIdx.y;
    const SegDesc sd = d[seg];
    if (!(sd.vec & kSegStat)) {
        if (g == 0 && threadIdx.x == 0) out[seg] = 0.0;
        return;
    }
    const uint64_t nt = (sd.len + kSegTile - 1) / kSegTile, groups = (nt + kFinGroup - 1) / kFinGroup;
    if (g >= groups) return;
    const uint64_t left = nt - g * kFinGroup;
    const double acc = group_sum(partials + sd.tile0 + g * kFinGroup, left < kFinGroup ? left : kFinGroup);
    if (threadIdx.x == 0) (groups == 1 ? out[seg] : lvl[sd.tile0 / kFinGroup + seg + g]) = acc;
}

__global__ void __launch_bounds__(64) k_sumsq_finish2(const SegDesc *__restrict__ d, const double *__restrict__ lvl,
                                                      double *__restrict__ out) {
    const unsigned seg = blockIdx.x;
    const SegDesc sd = d[seg];
    const uint64_t nt = (sd.len + kSegTile - 1) / kSegTile, groups = (nt + kFinGroup - 1) / kFinGroup;
    if (!(sd.vec & kSegStat) || groups <= 1) return;  // finished by k_sumsq_finish
    const double acc = group_sum(lvl + sd.tile0 / kFinGroup + seg, groups);
    if (threadIdx.x == 0) out[seg] = acc;
}

template <int WIRE, bool SCALE, class... A>
void launch_sumsq(bool narrow, dim3 g, hipStream_t stream, const char *fl, const SegDesc *dd, const uint32_t *db,
                  const void *map, float divisor, double *partials, A... a) {
    const auto k = narrow ? k_seg_sumsq<WIRE, true, SCALE, A...> : k_seg_sumsq<WIRE, false, SCALE, A...>;
    hipLaunchKernelGGL(k, g, dim3(64), 0, stream, fl, dd, db, map, divisor, partials, a...);
}

template <int DT, bool SCALE, class... A>
void launch_sumsq16(bool narrow, dim3 g, hipStream_t stream, const char *fl, const SegDesc *dd, const uint32_t *db,
                    const void *map, float divisor, double *partials, A... a) {
    const auto k = narrow ? k_seg_sumsq16<DT, true, SCALE, A...> : k_seg_sumsq16<DT, false, SCALE, A...>;
    hipLaunchKernelGGL(k, g, dim3(64), 0, stream, fl, dd, db, map, divisor, partials, a...);
}

// A run-time fact of a launch as a compile-time constant: f(std::integral_constant), so that each
// choice between two instances is written once.
template <class F> void with_bool(bool b, F f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
template <class F> void with_wire(int wire, F f) {  // of the converting copies: float16, else bfloat16 (CopyLaunch::wire)
    if (wire == DDL_HALF) f(std::integral_constant<int, kWireF16>{});
    else f(std::integral_constant<int, kWireBF16>{});
}

// fp32 tensors: every segment whole elements (`unit` bytes each in `bytes`: 4, or 2 for wire-side
// lengths) at a 4-byte aligned address.
void require_f32_segments(const CopySeg *segs, int count, size_t unit) {
    for (int i = 0; i < count; ++i)
        DDL_REQUIRE(segs[i].bytes % unit == 0 && reinterpret_cast<uintptr_t>(segs[i].ptr) % 4 == 0,
                    DDL_STATUS_INVALID_ARGUMENT, "segment " << i << " is not whole, aligned float32 elements");
}
// native 16-bit tensors: every segment whole elements at a 2-byte aligned address
void require_16bit_segments(const CopySeg *segs, int count, int dtype) {
    for (int i = 0; i < count; ++i)
        DDL_REQUIRE(segs[i].bytes % 2 == 0 && reinterpret_cast<uintptr_t>(segs[i].ptr) % 2 == 0, DDL_STATUS_INVALID_ARGUMENT,
                    "segment " << i << " is not whole, aligned " << dtype_name(dtype) << " elements");
}
// the tensors of a scaled or counted launch: float32 (also under a wire), or bfloat16 without one
void require_scalable_segments(const CopySeg *segs, int count, int dtype, int wire, const char *what) {
    const bool h16 = dtype == DDL_BFLOAT16 && !wire;
    DDL_REQUIRE(dtype == DDL_FLOAT || h16, DDL_STATUS_UNSUPPORTED_DTYPE,
                what << " defined for float32 tensors, not " << dtype_name(dtype));
    if (h16) require_16bit_segments(segs, count, dtype);
    else require_f32_segments(segs, count, wire ? 2 : 4);
}

}  // namespace

SegmentCopier::~SegmentCopier() {
    for (Slot &sl : slots_) {
        if (sl.ready) (void)hipEventSynchronize(sl.ready);
        if (sl.ready) (void)hipEventDestroy(sl.ready);
        if (sl.host) (void)hipHostFree(sl.host);
        if (sl.dev) (void)hipFree(sl.dev);
        if (sl.idx) (void)hipFree(sl.idx);
        if (sl.stat) (void)hipFree(sl.stat);
    }
}

// Table slots rotate; a slot is rewritten only after the copy that read it has run (its event).
// A slot still in use is skipped and the pool grows, so a pipeline of pack / unpack launches
// queued behind allreduces never blocks the host; at kMaxSlots the oldest slot is waited for.
SegmentCopier::Slot &SegmentCopier::free_slot_() {
    for (size_t k = 0; k < slots_.size(); ++k) {
        Slot &sl = slots_[(next_ + k) % slots_.size()];
        if (!sl.ready) continue;
        const hipError_t q = hipEventQuery(sl.ready);
        if (q == hipErrorNotReady) continue;
        DDL_HIP(q);
        next_ = (next_ + k + 1) % slots_.size();
        return sl;
    }
    if (slots_.size() < kMaxSlots) {
        slots_.emplace_back();
        Slot &sl = slots_.back();
        DDL_HIP(hipEventCreateWithFlags(&sl.ready, hipEventDisableTiming));
        next_ = 0;
        return sl;
    }
    Slot &sl = slots_[next_];
    next_ = (next_ + 1) % slots_.size();
    DDL_HIP(hipEventSynchronize(sl.ready));
    return sl;
}

size_t SegmentCopier::flat_bytes(const size_t *bytes, int count) {
    size_t off = 0;
    for (int i = 0; i < count; ++i) off += (bytes[i] + 255) & ~size_t(255);
    return off;
}

void SegmentCopier::copy(int dir, void *flat, void *const *ptrs, const size_t *bytes, int count, hipStream_t stream) {
    const bool tables = count > 0 && ptrs && bytes;  // null tables are run's to report
    plain_.resize(tables ? (size_t)count : 0);       // the other fields keep their defaults
    for (size_t i = 0; i < plain_.size(); ++i) plain_[i].ptr = ptrs[i], plain_[i].bytes = bytes[i];
    run(CopyLaunch{dir, flat, stream}, tables ? plain_.data() : nullptr, count);
}

void SegmentCopier::run(const CopyLaunch &how, const CopySeg *segs, int count) {
    const int dir = how.dir, dtype = how.dtype, wire = how.wire, divisor = how.divisor;
    void *flat = how.flat;
    const hipStream_t stream = how.stream;
    const int n = segs ? count : 0;  // a null table is reported below, behind the launch's own refusals
    // What the non-empty segments ask for, in one pass. An option's kernel, table and checks come only
    // with a segment that asks for it: every other launch is the kernel it was, its tables exactly as before.
    bool fbk = false, srk = false, sc = false, stat = false, div = false, wanted = false;
    int bad_scale = -1;  // the first factor that is not finite and positive: refused below, in its turn
    const uint64_t seg_tile = kSegTile;  // segment-aligned tiles of kSegTile bytes per workgroup
    uint64_t tiles = 0;
    const bool plain = segs == plain_.data();  // copy()'s own segments: every option at its default
    const bool h16 = !wire && dtype == DDL_BFLOAT16;  // native 16-bit tensors whose factors and statistic have kernels
    const bool q8 = wire == kDtypeE4m3;  // the e4m3 wire: granules in the flat buffer, the element counts in a table
    for (int i = 0; i < n; ++i) {
        const CopySeg &sg = segs[i];
        wanted |= sg.want;
        if (!sg.bytes) continue;
        tiles += (sg.bytes + seg_tile - 1) / seg_tile;
        if (plain) continue;
        fbk |= sg.residual != nullptr;
        srk |= sg.stream.on != 0;
        stat |= sg.want;
        div |= sg.op == DDL_ALLREDUCE_OP_AVG;
        if (sg.scale == 1.0f) continue;
        sc = true;
        if (bad_scale < 0 && !(std::isfinite(sg.scale) && sg.scale > 0.0f)) bad_scale = i;
    }
    fbk = fbk && wire && dir == 0;  // a converting pack's
    srk = srk && wire && dir == 0;
    sc = sc && (dir == 0 || dir == 1 || dir == kDivInPlace);
    // the e4m3 unpack takes no statistic itself: one read-only pass over the outputs behind it (below)
    const bool q8stat = q8 && stat && dir == 1 && how.sumsq;
    stat = stat && (dir == 1 || dir == kSumsqInPlace) && !q8;
    // the quotient where it is not the identity (kSumsqInPlace: the segments hold their results, nothing is
    // divided; a converting pack has no ops)
    div = div && divisor > 1 && (wire ? dir == 1 : dir != kSumsqInPlace);
    if (wire) {
        DDL_REQUIRE(dtype == DDL_FLOAT, DDL_STATUS_UNSUPPORTED_DTYPE,
                    "wire compression is defined for float32 sources, not " << dtype_name(dtype));
        DDL_REQUIRE(wire == DDL_HALF || wire == DDL_BFLOAT16 || q8, DDL_STATUS_UNSUPPORTED_DTYPE,
                    "wire dtype " << wire << " is neither float16 nor bfloat16");
        DDL_REQUIRE(dir == 0 || dir == 1 || (dir == kSumsqInPlace && !q8), DDL_STATUS_INVALID_ARGUMENT,
                    "copier direction " << dir);
        for (int i = 0; i < n && q8; ++i)
            DDL_REQUIRE(segs[i].bytes == e4m3_granules(segs[i].elems) * kE4m3Granule && !segs[i].stream.on,
                        DDL_STATUS_INVALID_ARGUMENT, "segment " << i << " is not the granules of its elements");
        DDL_REQUIRE(divisor >= 1, DDL_STATUS_INVALID_ARGUMENT, "divisor " << divisor);
        require_f32_segments(segs, n, 2);
        for (int i = 0; i < n && fbk; ++i)
            DDL_REQUIRE(!segs[i].bytes || reinterpret_cast<uintptr_t>(segs[i].residual) % 4 == 0, DDL_STATUS_INVALID_ARGUMENT,
                        "residual " << i << " is not aligned float32 elements");
        DDL_REQUIRE(!srk || wire == DDL_BFLOAT16, DDL_STATUS_INVALID_ARGUMENT,
                    "stochastic rounding is defined for the bfloat16 wire");
        for (int i = 0; i < n && srk && fbk; ++i)
            DDL_REQUIRE(!(segs[i].stream.on && segs[i].residual), DDL_STATUS_INVALID_ARGUMENT,
                        "segment " << i << " asks for error feedback and stochastic rounding");
    }
    if (count <= 0) return;
    if (sc) {
        DDL_REQUIRE(bad_scale < 0, DDL_STATUS_INVALID_ARGUMENT,
                    "scale factor " << segs[bad_scale].scale << " of segment " << bad_scale << " is not finite and positive");
        require_scalable_segments(segs, n, dtype, wire, "scale factors are");
    }
    if (dir == 1 || dir == kSumsqInPlace) {
        DDL_REQUIRE(!wanted || how.sumsq, DDL_STATUS_INVALID_ARGUMENT, "sum of squares without an output");
        // a launch that leaves the statistic out, an empty segment (host memory: ours until posted)
        for (int i = 0; i < n && how.sumsq; ++i) how.sumsq[i] = 0.0;
    }
    if (dir == kSumsqInPlace && !stat) return;  // nothing wanted: the zeros above are the answer
    if (stat) {
        require_scalable_segments(segs, n, dtype, wire, "the sum of squares is");
    }
    if (dir == kDivInPlace) {
        if (!div && !sc) return;  // nothing to divide or scale: the segments already hold their results
        flat = nullptr;
    } else if (dir == kSumsqInPlace) {
        flat = nullptr;
    } else {
        DDL_REQUIRE(dir == 0 || dir == 1, DDL_STATUS_INVALID_ARGUMENT, "copier direction " << dir);
        DDL_REQUIRE(!div || dir == 1, DDL_STATUS_INVALID_ARGUMENT, "the quotient belongs to the unpack");
    }
    const bool in_place = dir == kDivInPlace || dir == kSumsqInPlace;
    DDL_REQUIRE((flat || in_place) && segs, DDL_STATUS_INVALID_ARGUMENT, "null pack arguments");
    const size_t es = div ? dtype_size(dtype) : 1;
    if (div && !sc && !stat && !wire) {  // DivOp over `dtype`
        DDL_REQUIRE(dtype == DDL_FLOAT || dtype == DDL_DOUBLE || dtype == DDL_HALF || dtype == DDL_BFLOAT16,
                    DDL_STATUS_UNSUPPORTED_DTYPE, "AVG is not defined for dtype " << dtype);
        for (int i = 0; i < count; ++i)
            DDL_REQUIRE(segs[i].bytes % es == 0 && reinterpret_cast<uintptr_t>(segs[i].ptr) % es == 0,
                        DDL_STATUS_INVALID_ARGUMENT,
                        "segment " << i << " is not whole, aligned " << dtype_name(dtype) << " elements");
    }
    // in place only the segments the launch works on have tiles: the wanted ones of the sum of squares
    // (nothing else is read), else the AVG and the scaled ones (a SUM segment already is its result)
    std::vector<CopySeg> own;
    if (in_place) {
        own.assign(segs, segs + count);
        for (CopySeg &sg : own) {
            const bool work = dir == kSumsqInPlace ? sg.want
                                                   : (div && sg.op == DDL_ALLREDUCE_OP_AVG) || (sc && sg.scale != 1.0f);
            if (!work) sg.bytes = 0;
        }
        segs = own.data();
        tiles = 0;
        for (const CopySeg &sg : own) tiles += (sg.bytes + seg_tile - 1) / seg_tile;
    }
    Slot &sl = free_slot_();
    // tile0 = running tile count
    DDL_REQUIRE(tiles < (1ull << 31), DDL_STATUS_INVALID_ARGUMENT, "fusion buffer too large");
    const uint64_t nblk = (tiles + kIdxBlock - 1) / kIdxBlock;
    const size_t table = (size_t)count * sizeof(SegDesc);
    // descriptors, then the block bases, then (feedback pack) one residual address per segment or
    // (stochastic pack) one WireStream per segment, then (scaled launch) one factor per segment
    const size_t rtab = (table + nblk * sizeof(uint32_t) + 7) & ~size_t(7);
    // (the e4m3 wire: one SegElems per segment where a 16-bit feedback pack has its residual addresses, the
    // residual addresses of an e4m3 feedback pack behind them)
    const size_t ftab = q8 ? rtab + (size_t)count * sizeof(SegElems) : rtab;
    const size_t wtab = fbk ? ftab + (size_t)count * sizeof(uint64_t) : ftab;
    const size_t stab = srk ? wtab + (size_t)count * sizeof(WireStream) : fbk || q8 ? wtab : table + nblk * sizeof(uint32_t);
    const size_t need = sc ? stab + (size_t)count * sizeof(float) : stab;
    if (need > sl.cap) {  // outgrown tables kept until ddl_finalize: no hipFree on a data path (engine.h)
        retire_host(sl.host);
        retire_device(sl.dev);
        sl.host = sl.dev = nullptr;
        sl.cap = need + need / 2;
        DDL_HIP(hipHostMalloc(&sl.host, sl.cap, hipHostMallocDefault));
        DDL_HIP(hipMalloc(&sl.dev, sl.cap));
    }
    SegDesc *t = static_cast<SegDesc *>(sl.host);
    uint32_t *bases = reinterpret_cast<uint32_t *>(static_cast<char *>(sl.host) + table);
    uint64_t off = 0, tl = 0;
    for (int i = 0; i < count; ++i) {
        const CopySeg &sg = segs[i];
        DDL_REQUIRE(sg.bytes == 0 || sg.ptr, DDL_STATUS_INVALID_ARGUMENT, "null segment " << i);
        t[i].ptr = reinterpret_cast<uint64_t>(sg.ptr);
        t[i].off = off;
        t[i].len = sg.bytes;
        t[i].vec = (reinterpret_cast<uintptr_t>(sg.ptr) & 15u) == 0 ? kSegVec : 0;
        if (div && sg.op == DDL_ALLREDUCE_OP_AVG) t[i].vec |= kSegAvg;
        if (stat && sg.want && sg.bytes) t[i].vec |= kSegStat;
        if (sc && sg.bytes && sg.scale != 1.0f) t[i].vec |= kSegScale;
        t[i].tile0 = (uint32_t)tl;
        off += (sg.bytes + 255) & ~uint64_t(255);
        tl += (sg.bytes + seg_tile - 1) / seg_tile;
    }
    if (off == 0) return;
    if (fbk) {
        uint64_t *rt = reinterpret_cast<uint64_t *>(static_cast<char *>(sl.host) + ftab);
        for (int i = 0; i < count; ++i) rt[i] = segs[i].bytes ? reinterpret_cast<uint64_t>(segs[i].residual) : 0;
    }
    for (int i = 0; i < count && q8; ++i) reinterpret_cast<SegElems *>(static_cast<char *>(sl.host) + rtab)[i].n = segs[i].elems;
    for (int i = 0; i < count && srk; ++i) reinterpret_cast<WireStream *>(static_cast<char *>(sl.host) + wtab)[i] = segs[i].stream;
    for (int i = 0; i < count && sc; ++i) reinterpret_cast<float *>(static_cast<char *>(sl.host) + stab)[i] = segs[i].scale;
    // block b's base: the segment of tile b * 128 (the last one with tile0 <= it, as
    // k_tile_index resolves); narrow when no block spans more than 255 segments
    bool narrow = true;
    for (uint64_t b = 0, s0 = 0, s1 = 0; b < nblk; ++b) {
        const uint64_t first = b * kIdxBlock, last = std::min(tiles, first + kIdxBlock) - 1;
        while (s0 + 1 < (uint64_t)count && t[s0 + 1].tile0 <= first) ++s0;
        if (s1 < s0) s1 = s0;
        while (s1 + 1 < (uint64_t)count && t[s1 + 1].tile0 <= last) ++s1;
        bases[b] = (uint32_t)s0;
        if (s1 - s0 > 255) narrow = false;
    }
    DDL_HIP(hipMemcpyAsync(sl.dev, sl.host, need, hipMemcpyHostToDevice, stream));
    char *fl = static_cast<char *>(flat);
    const SegDesc *dd = static_cast<const SegDesc *>(sl.dev);
    const uint32_t *db = reinterpret_cast<const uint32_t *>(static_cast<char *>(sl.dev) + table);
    if (tiles > 0) {
        const size_t ib = narrow ? (tiles + 3) & ~uint64_t(3) : tiles * sizeof(int);
        if (ib > sl.idx_cap) {
            retire_device(sl.idx);
            sl.idx = nullptr;
            sl.idx_cap = ib + ib / 2;
            DDL_HIP(hipMalloc(&sl.idx, sl.idx_cap));
        }
        const dim3 ig((unsigned)((tiles + 255) / 256)), g((unsigned)tiles);
        if (narrow) hipLaunchKernelGGL(k_tile_index<true>, ig, dim3(256), 0, stream, dd, count, (uint64_t)tiles, db, sl.idx);
        else hipLaunchKernelGGL(k_tile_index<false>, ig, dim3(256), 0, stream, dd, count, (uint64_t)tiles, db, sl.idx);
        // the statistic's scratch: one partial per tile, the group values, then one result per segment
        double *partials = nullptr;
        uint64_t fin_groups = 0;  // of the longest wanted segment
        const uint64_t lvl_n = tiles / kFinGroup + (uint64_t)count + 1;
        if (stat) {
            for (int i = 0; i < count; ++i)
                if (t[i].vec & kSegStat)
                    fin_groups = std::max(fin_groups, ((segs[i].bytes + seg_tile - 1) / seg_tile + kFinGroup - 1) / kFinGroup);
            DDL_REQUIRE(fin_groups <= kFinGroup, DDL_STATUS_INVALID_ARGUMENT,
                        "the sum of squares takes pieces of at most " << kFinGroup * kFinGroup << " tiles");
            const size_t sb = (tiles + lvl_n + (size_t)count) * sizeof(double);
            if (sb > sl.stat_cap) {
                retire_device(sl.stat);
                sl.stat = nullptr;
                sl.stat_cap = sb + sb / 2;
                DDL_HIP(hipMalloc(&sl.stat, sl.stat_cap));
            }
            partials = static_cast<double *>(sl.stat);
        }
        const uint64_t *res = reinterpret_cast<const uint64_t *>(static_cast<char *>(sl.dev) + ftab);  // (fbk)
        const WireStream *sts = reinterpret_cast<const WireStream *>(static_cast<char *>(sl.dev) + wtab);  // (srk)
        const float *scl = reinterpret_cast<const float *>(static_cast<char *>(sl.dev) + stab);        // (sc)
        // The instance, from the launch's facts. SCALE: the scaled twin of the same Op, the factor table
        // behind its other arguments; an unscaled launch passes no table.
        with_bool(sc, [&](auto scaled) {
            constexpr bool SCALE = decltype(scaled)::value;
            const auto go = [&](auto launcher, auto... a) {
                if constexpr (SCALE) launcher(a..., scl);
                else launcher(a...);
            };
            const auto seg = [&](auto op, auto... a) {  // k_seg<Op>; op: a null pointer of the Op's type
                using Op = std::remove_pointer_t<decltype(op)>;
                go([&](auto... x) { launch<Op>(narrow, g, stream, fl, dd, db, sl.idx, x...); }, a...);
            };
            const auto sumsq = [&](auto w) {  // k_seg_sumsq: fp32 flat (-1), wire flat, in place
                constexpr int W = decltype(w)::value;
                go([&](auto... x) {
                    launch_sumsq<W, SCALE>(narrow, g, stream, fl, dd, db, sl.idx, (float)divisor, partials, x...);
                });
            };
            if (stat && h16) {  // bfloat16 tensors (checked above): the 2-byte layout, scatter or in place
                go([&](auto... x) {
                    launch_sumsq16<kDivBF16, SCALE>(narrow, g, stream, fl, dd, db, sl.idx, (float)divisor, partials, x...);
                });
            } else if (stat) {
                if (wire) with_wire(wire, sumsq);
                else sumsq(std::integral_constant<int, -1>{});
            } else if (q8) {
                const SegElems *cnt = reinterpret_cast<const SegElems *>(static_cast<char *>(sl.dev) + rtab);
                if (dir != 0) seg((Q8UnpackOp<SCALE> *)nullptr, (float)divisor, cnt);
                else if (fbk) seg((Q8PackOp<SCALE, true> *)nullptr, cnt, res);
                else seg((Q8PackOp<SCALE> *)nullptr, cnt);
            } else if (wire) {
                with_wire(wire, [&](auto w) {
                    constexpr int W = decltype(w)::value;
                    if (dir != 0) seg((CvtUnpackOp<W, SCALE> *)nullptr, (float)divisor);  // AVG or not: kSegAvg
                    else if (srk && fbk) seg((CvtPackSrOp<SCALE, true> *)nullptr, res, sts);
                    else if (srk) seg((CvtPackSrOp<SCALE> *)nullptr, sts);
                    else if (fbk) seg((CvtPackOp<W, true, SCALE> *)nullptr, res);
                    else seg((CvtPackOp<W, false, SCALE> *)nullptr);
                });
            } else if constexpr (SCALE) {  // fp32 or bf16 (checked above); the scatter also in place
                if (h16 && dir == 0) seg((ScaleGather16Op<kDivBF16> *)nullptr);
                else if (h16) seg((DivOp<kDivBF16, true> *)nullptr, (double)divisor);
                else if (dir == 0) seg((ScaleGatherOp *)nullptr);
                else seg((DivOp<kDivF32, true> *)nullptr, (double)divisor);
            } else if (dir == 0) {
                seg((CopyOp<0> *)nullptr);
            } else if (!div) {
                seg((CopyOp<1> *)nullptr);
            } else {
                const double dv = (double)divisor;
                switch (dtype) {
                    case DDL_FLOAT: seg((DivOp<kDivF32> *)nullptr, dv); break;
                    case DDL_DOUBLE: seg((DivOp<kDivF64> *)nullptr, dv); break;
                    case DDL_HALF: seg((DivOp<kDivF16> *)nullptr, dv); break;
                    case DDL_BFLOAT16: seg((DivOp<kDivBF16> *)nullptr, dv); break;
                    default: fail(DDL_STATUS_UNSUPPORTED_DTYPE, std::string("AVG is not defined for ") + dtype_name(dtype));
                }
            }
        });
        if (stat) {  // the segments' values, then to the caller's host memory ahead of whatever it records next
            double *lvl = partials + tiles, *res = lvl + lvl_n;
            hipLaunchKernelGGL(k_sumsq_finish, dim3((unsigned)count, (unsigned)fin_groups), dim3(64), 0, stream, dd, partials,
                               lvl, res);
            if (fin_groups > 1) hipLaunchKernelGGL(k_sumsq_finish2, dim3((unsigned)count), dim3(64), 0, stream, dd, lvl, res);
            DDL_HIP(hipMemcpyAsync(how.sumsq, res, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, stream));
        }
    }
    DDL_HIP(hipGetLastError());
    DDL_HIP(hipEventRecord(sl.ready, stream));
    if (dep::on()) {  // happens-before trace (deptrace.h): the segments and the flat buffer
        std::vector<dep::Access> acc;
        const bool gather = dir == 0 || dir == kSumsqInPlace;  // segments read (and the flat buffer written)
        if (!in_place) acc.push_back(gather ? dep::wr(flat, off) : dep::rd(flat, off));
        const size_t widen = wire && !q8 ? dtype_size(dtype) / dtype_size(wire) : 1;  // the tensor side in its own bytes
        for (int i = 0; i < count; ++i)
            if (segs[i].bytes) {
                const size_t tb = q8 ? segs[i].elems * sizeof(float) : segs[i].bytes * widen;
                acc.push_back(gather ? dep::rd(segs[i].ptr, tb) : dep::wr(segs[i].ptr, tb));
            }
        for (int i = 0; i < count && fbk; ++i)
            if (segs[i].bytes && segs[i].residual) {  // read and written: both, so the race check sees either side
                const size_t rb = q8 ? segs[i].elems * sizeof(float) : segs[i].bytes * widen;
                acc.push_back(dep::rd(segs[i].residual, rb));
                acc.push_back(dep::wr(segs[i].residual, rb));
            }
        const std::string label =
            in_place ? (dir == kSumsqInPlace ? "sumsq" : sc ? "scale" : "divide")
                     : std::string(dir == 0 ? "pack" : "unpack") + (wire ? " cvt" : "") + (fbk ? " fb" : "") + (srk ? " sr" : "") +
                           (div && !sc && !stat ? " avg" : "") + (sc ? " scale" : "") + (stat ? " sumsq" : "");
        dep::op(stream, label, std::move(acc));
    }
    if (q8stat) {  // the canonical uncompressed sums over what the unpack stored: one extra read of the outputs
        std::vector<CopySeg> f32(segs, segs + count);
        for (CopySeg &sg : f32) sg.bytes = sg.elems * sizeof(float), sg.scale = 1.0f, sg.op = DDL_ALLREDUCE_OP_SUM;
        run(CopyLaunch{kSumsqInPlace, nullptr, stream, DDL_FLOAT, 0, 1, how.sumsq}, f32.data(), count);
    }
}

}  // namespace ddl
