// e4m3.h — device code of the block-scaled e4m3 wire (DDL_ALLREDUCE_WIRE_E4M3; the format and the rules are
// fixed in include/ddl_amd.h "The e4m3 wire" and restated in tests/_e4m3_helpers.py), shared by the pack / unpack
// Ops (pack.hip) and the fold (reduce_kernels.hip k_foldq).
//
// A granule is 256 bytes = 64 dwords (63 of four codes, the last the fp32 scale) worked on by one row of 16 lanes,
// four dwords a lane: in the fold, lane r holds the 16-byte unit r (dwords 4 r .. 4 r + 3: elements 16 r .. + 15);
// in the pack and the unpack, dwords r, 16 + r, 32 + r, 48 + r (the tensor side's 16-byte vectors). Either way lane
// 15's fourth dword is the scale, so its x[12..15] are not elements. A granule's amax is a reduction over one DPP
// row (no LDS), and a row is always either whole inside a launch's data or whole outside it: every lane of a row
// executes the row operations together.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ddl {
namespace e4m3 {

using u32x4 = unsigned int __attribute__((ext_vector_type(4)));

// one fp32 product, rounded on its own: never part of an fma (hipcc contracts a * b + c by default)
__device__ inline float mul1(float x, float a) {
#pragma clang fp contract(off)
    return x * a;
}

// elements a lane of row position r holds
__device__ inline int lane_count(int r) { return r == 15 ? 12 : 16; }

// max over the 16 lanes of a DPP row: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
__device__ inline uint32_t row_max(uint32_t m) {
    uint32_t o;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xF, 0xF, false);
    m = m > o ? m : o;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xF, 0xF, false);
    m = m > o ? m : o;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x141, 0xF, 0xF, false);
    m = m > o ? m : o;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x140, 0xF, 0xF, false);
    return m > o ? m : o;
}

// the biased exponent of the scale for an amax with the bits `m` (sign clear, finite): the smallest power of
// two s with amax / s <= 448 = 1.75 * 2^8, at least 2^-126. A mantissa above 1.75 takes the next power.
__device__ inline uint32_t scale_exponent(uint32_t m) {
    const int e = (int)((m + 0x1fffffu) >> 23) - 8;
    return (uint32_t)(e < 1 ? 1 : e);
}

// The pack's rule over one lane's share of a granule: x[4 h .. 4 h + 3] are the contributions behind the lane's
// dword h (elements past the request's end are +0.0; lane 15's x[12..15] are not looked at). Returns the lane's
// four dwords. Every lane of the row calls it. SUM: x are sums (the fold) — IEEE 754 does not pin the sign of a NaN
// that arithmetic produced, so a NaN sum is written as 0x7f; an infinite sum (an overflow) keeps its sign.
template <bool SUM = false> __device__ inline u32x4 quantize_row(const float (&x)[16], int r) {
    const int cnt = lane_count(r);
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t a = __float_as_uint(x[k]) & 0x7fffffffu;
        if (k < cnt && a < 0x7f800000u) m = a > m ? a : m;  // finite elements only
    }
    m = row_max(m);
    const uint32_t se = scale_exponent(m);
    const float inv = __uint_as_float((254u - se) << 23);  // 1 / s: a normal power of two, the product exact
    uint32_t w[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        float y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = mul1(x[4 * h + k], inv);
        // v_cvt_pk_fp8_f32: RNE with subnormal codes over |y| <= 448 (tests/test_e4m3_kernel_gpu.py's rounding sweep)
        int p = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
        p = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], p, true);
        uint32_t c = (uint32_t)p;
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // a NaN or an infinity: 0x7f | sign, written explicitly
            const uint32_t u = __float_as_uint(x[4 * h + k]);
            const uint32_t a = u & 0x7fffffffu, sign = SUM && a > 0x7f800000u ? 0u : (u >> 24) & 0x80u;
            if (a >= 0x7f800000u) c = (c & ~(0xffu << (8 * k))) | ((0x7fu | sign) << (8 * k));
        }
        w[h] = c;
    }
    if (r == 15) w[3] = se << 23;
    return u32x4{w[0], w[1], w[2], w[3]};
}

// The same rule in two halves for the feedback pack (pack.hip Q8PackOp<SCALE, true>), which needs the scale on every
// lane to decode its own codes, without a second reduction or a shuffle: row_scale_exponent — the biased exponent of
// the granule's scale, the same on all sixteen lanes (the row reduction leaves the amax on every one) — and
// encode_row, the lane's four dwords under that scale. Written apart from quantize_row, not under it: the kernels
// that call quantize_row keep their instruction streams only while it stays the one function it was
// (profiles/wire_e4m3_feedback/parent_kernels_unchanged.txt).
__device__ inline uint32_t row_scale_exponent(const float (&x)[16], int r) {
    const int cnt = lane_count(r);
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t a = __float_as_uint(x[k]) & 0x7fffffffu;
        if (k < cnt && a < 0x7f800000u) m = a > m ? a : m;  // finite elements only
    }
    return scale_exponent(row_max(m));
}

__device__ inline u32x4 encode_row(const float (&x)[16], int r, const uint32_t se) {
    const float inv = __uint_as_float((254u - se) << 23);  // 1 / s
    uint32_t w[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        float y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = mul1(x[4 * h + k], inv);
        int p = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
        p = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], p, true);
        uint32_t c = (uint32_t)p;
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // a NaN or an infinity: 0x7f | sign
            const uint32_t u = __float_as_uint(x[4 * h + k]);
            if ((u & 0x7fffffffu) >= 0x7f800000u) c = (c & ~(0xffu << (8 * k))) | ((0x7fu | ((u >> 24) & 0x80u)) << (8 * k));
        }
        w[h] = c;
    }
    if (r == 15) w[3] = se << 23;
    return u32x4{w[0], w[1], w[2], w[3]};
}

// code * s of the lane's 16 codes, one fp32 product each (exact; subnormals kept; a NaN code or scale gives NaN)
__device__ inline void dequantize(const u32x4 raw, float s, float (&y)[16]) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int w = (int)raw[h];
        y[4 * h + 0] = mul1(__builtin_amdgcn_cvt_f32_fp8(w, 0), s);
        y[4 * h + 1] = mul1(__builtin_amdgcn_cvt_f32_fp8(w, 1), s);
        y[4 * h + 2] = mul1(__builtin_amdgcn_cvt_f32_fp8(w, 2), s);
        y[4 * h + 3] = mul1(__builtin_amdgcn_cvt_f32_fp8(w, 3), s);
    }
}

// the granule's scale, held by lane 15 of the row in the last dword of its unit
__device__ inline float row_scale(uint32_t last_dword) {
    return __uint_as_float((uint32_t)__shfl((int)last_dword, (int)(threadIdx.x | 15u), 64));
}

}  // namespace e4m3
}  // namespace ddl
