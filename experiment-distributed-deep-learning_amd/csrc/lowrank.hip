// lowrank.hip — the kernels of the low-rank (PowerSGD) wire and their launcher (lowrank.h).
//
// All tensors of a plan go in one launch per stage; a workgroup finds the tensor of its tile by a scalar binary
// search of that stage's tile0 column (as adasum.hip). Everything a stage hands to the next lies in one plan
// scratch `ws`, addressed in floats by the table.
//
// v_mfma_f32_16x16x4_f32 takes A (16 x 4) and B (4 x 16): lane l supplies A[l % 16][l / 16] and B[l / 16][l % 16],
// and register j of lane l holds D[4 (l / 16) + j][l % 16]. The sum over k has no order to keep, so in both GEMMs
// a lane takes a float4 of M and issues four MFMAs with its components.
//
// Project, P_loc = A Q_used (R x r, K = C). A tile is 16 rows of M against kProjCols columns. Lane-direct: lane
// (m, kk) = (l % 16, l / 16) loads the float4 of g and of e at row m, columns k + 4 kk .. + 3, forms a in registers,
// stores it, and its component i is A-operand [m][kk] of MFMA i; the B-operand is Q_used[k + 4 kk + i][m], one
// 16-byte LDS read of the chunk's Q_used, which the workgroup staged TRANSPOSED and padded to 16 columns (columns
// >= r zeros, dead columns qinit). Chosen over staging the row block through LDS: a lives in the lane that
// loads g and e and stores a, so the tile's 16 x 512 elements never cross LDS, and LDS carries only Q (33 KiB). The
// price is 64-byte runs per row and load; a wave walks its quarter of the chunk left to right, so two successive
// loads complete each 128-byte line while it is still in the vector cache. The four waves' accumulators meet in
// LDS and are added in wave order into the tile's 16 x 16 partial; k_lr_fold adds a row block's partials in split
// order. Nothing is atomic.
//
// Back-project, Q_loc = A^T P^ (C x r, K = R). A tile is 64 columns of M against kBackRows rows. Lane (m, kk) loads
// the float4 of a at row k + kk, columns 4 m .. 4 m + 3 — the 16 lanes of a row read one 256-byte run — and
// component i is the A-operand of MFMA i, whose output rows are the columns 4 m' + i: four accumulators, one
// B-operand P^[k + kk][m] for all four (columns >= r zeros), read from L2.
//
// Reconstruct, D- = P^ Q-^T with K = r <= 16: plain FMAs, not the MFMA. The MFMA's D layout gives a lane four
// ROWS of one column, so its stores would be 4-byte and column-strided; with FMAs a lane owns a float4 of a row,
// holds the 4 r entries of Q- of its columns in registers, reads the row's P^ by 16-byte LDS broadcasts, and
// reads a once and writes e' and out once as 16-byte row-contiguous accesses (256-byte runs per 16 lanes).
// Instantiated per r so the FMA chain has exactly r terms and Q- stays in registers.
//
// A tensor pointer that is not 16-byte aligned, and the ragged tail of the last row, go element by element;
// nothing at or past element n of a tensor is read or written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "lowrank.h"

namespace ddl {

namespace {

using f32x4 = float __attribute__((ext_vector_type(4)));

constexpr uint32_t kProjCols = 512;        // columns of M per project workgroup (a K-split of the project)
constexpr uint32_t kQStride = kProjCols + 4;  // floats per column of the transposed Q_used in LDS
constexpr uint32_t kBackRows = 512;        // rows of M per back-project workgroup (a K-split of the back-project)
constexpr uint32_t kReconRows = 64;        // a reconstruct tile: 64 rows x 64 columns
constexpr uint32_t kCtl = 32;              // words of flags per tensor: the r column flags, the poison at kPoison
constexpr uint32_t kPoison = 16;
constexpr uint32_t kNan = 0x7fc00000u;

struct LrSeg {
    uint64_t in, out, res, state;  // the request's tensors, this rank's residual and Q state (Q, then r flags)
    uint32_t n, R, C, small;
    uint64_t p_at, q_at, a_at, pp_at, qp_at;  // in ws, in floats: P (a small tensor: its a), Q, a, the partials
    uint32_t S, T;                             // K-splits of the project, of the back-project
    uint32_t t_proj, t_pfold, t_back, t_qfold, t_recon;  // the tensor's first tile of each stage
    float pre, post;
    uint32_t avg, pad;
};

// the last tensor whose first tile of the stage <= tile (tensors without tiles share the next one's)
template <uint32_t LrSeg::*T0>
__device__ inline int seg_of(const LrSeg *__restrict__ d, int count, unsigned tile) {
    int lo = 0, hi = count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (d[mid].*T0 <= tile) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ inline uint32_t fmix32(uint32_t x) {  // MurmurHash3's finaliser
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}

// the start of a dead column: a function of the indices only, so the same on every rank
__device__ inline float qinit(uint32_t c, uint32_t j) {
    return (float)(int32_t)fmix32(16u * c + j + 0x9e3779b9u) * 0x1p-31f;
}

// a = fl32(pre x g) + e: two operations, each rounded to nearest even, never contracted (pre == 1: g itself)
__device__ inline float accumulate(float g, float pre, float e) {
#pragma clang fp contract(off)
    const float c = pre == 1.0f ? g : g * pre;
    return c + e;
}

__device__ inline bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// Elements [i, i + 4) of a tensor of n; those at or past n read +0.0 and are never written.
__device__ inline void load4(const float *__restrict__ p, uint32_t i, uint32_t n, bool vec, float *v) {
    if (vec && i + 4 <= n) {
        const float4 x = *reinterpret_cast<const float4 *>(p + i);
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) v[j] = i + j < n ? p[i + j] : 0.0f;
}

__device__ inline void store4(float *__restrict__ p, uint32_t i, uint32_t n, bool vec, const float *v) {
    if (vec && i + 4 <= n) {
        *reinterpret_cast<float4 *>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        if (i + j < n) p[i + j] = v[j];
}

__global__ void __launch_bounds__(256) k_lr_project(const LrSeg *__restrict__ d, int count, uint32_t r,
                                                    float *__restrict__ ws) {
    __shared__ float qs[16 * kQStride];
    __shared__ float red[4][16][16];
    const unsigned tile = blockIdx.x;
    const LrSeg sd = d[seg_of<&LrSeg::t_proj>(d, count, tile)];
    const uint32_t lt = tile - sd.t_proj, rb = lt / sd.S, c0 = (lt % sd.S) * kProjCols;
    const uint32_t cols = sd.C - c0 < kProjCols ? sd.C - c0 : kProjCols;  // a multiple of 64
    // Q_used of the chunk, transposed: qs[j][c]
    const float *__restrict__ Q = reinterpret_cast<const float *>(sd.state);
    const uint32_t *__restrict__ flags = reinterpret_cast<const uint32_t *>(Q + (uint64_t)sd.C * r);
    uint32_t alive = 0;
    for (uint32_t j = 0; j < r; ++j) alive |= (flags[j] != 0 ? 1u : 0u) << j;
    for (uint32_t e = threadIdx.x; e < cols * 16; e += 256) {
        const uint32_t c = e >> 4, j = e & 15;
        float v = 0.0f;
        if (j < r) v = (alive >> j) & 1 ? Q[(uint64_t)(c0 + c) * r + j] : qinit(c0 + c, j);
        qs[j * kQStride + c] = v;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kk = lane >> 4;
    const uint32_t row = rb * 16 + m;
    const bool live = row < sd.R;
    const float *__restrict__ g = reinterpret_cast<const float *>(sd.in);
    const float *__restrict__ er = reinterpret_cast<const float *>(sd.res);
    float *__restrict__ a = ws + sd.a_at;
    const bool vg = (sd.in & 15u) == 0, ve = (sd.res & 15u) == 0;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    const uint32_t quarter = cols / 4;  // a multiple of 16
    for (uint32_t k = wave * quarter; k < (wave + 1) * quarter; k += 16) {  // (wave-uniform)
        const uint64_t at = (uint64_t)row * sd.C + c0 + k + 4 * kk;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (live && at < sd.n) {
            float gv[4], ev[4];
            load4(g, (uint32_t)at, sd.n, vg, gv);
            load4(er, (uint32_t)at, sd.n, ve, ev);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = accumulate(gv[i], sd.pre, ev[i]);
            store4(a, (uint32_t)at, sd.n, true, v);
        }
        const float4 q = *reinterpret_cast<const float4 *>(&qs[m * kQStride + k + 4 * kk]);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v[0], q.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v[1], q.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v[2], q.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v[3], q.w, acc, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) red[wave][4 * kk + j][m] = acc[j];
    __syncthreads();
    const float *__restrict__ f = &red[0][0][0];
    float t = f[threadIdx.x];
    for (int w = 1; w < 4; ++w) t = t + f[w * 256 + threadIdx.x];
    ws[sd.pp_at + (uint64_t)lt * 256 + threadIdx.x] = t;
}

__global__ void __launch_bounds__(256) k_lr_back(const LrSeg *__restrict__ d, int count, uint32_t r,
                                                 float *__restrict__ ws) {
    __shared__ float red[4][64][16];
    const unsigned tile = blockIdx.x;
    const LrSeg sd = d[seg_of<&LrSeg::t_back>(d, count, tile)];
    const uint32_t lt = tile - sd.t_back, cb = lt / sd.T, r0 = (lt % sd.T) * kBackRows;
    const uint32_t r1 = sd.R - r0 < kBackRows ? sd.R : r0 + kBackRows;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kk = lane >> 4;
    const uint32_t col = cb * 64 + 4 * m;
    const float *__restrict__ a = ws + sd.a_at;
    const float *__restrict__ ph = ws + sd.p_at;
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t k = r0 + 4 * wave; k < r1; k += 16) {  // (wave-uniform)
        const uint32_t row = k + kk;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float p = 0.0f;
        if (row < r1) {
            const uint64_t at = (uint64_t)row * sd.C + col;
            if (at < sd.n) load4(a, (uint32_t)at, sd.n, true, v);
            if (m < r) p = ph[(uint64_t)row * r + m];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[i], p, acc[i], 0, 0, 0);
    }
    // output row 4 kk + j of MFMA i is column 4 (4 kk + j) + i of the tile
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) red[wave][4 * (4 * kk + j) + i][m] = acc[i][j];
    __syncthreads();
    const float *__restrict__ f = &red[0][0][0];
    for (uint32_t e = threadIdx.x; e < 1024; e += 256) {
        float t = f[e];
        for (int w = 1; w < 4; ++w) t = t + f[w * 1024 + e];
        ws[sd.qp_at + (uint64_t)lt * 1024 + e] = t;
    }
}

// The K-split partials of a block of B rows (of P: B = 16; of Q: B = 64) added in split order, from the first:
// one thread per entry of the tensor's P or Q. A small tensor's fold (of P only) is its a = fl32(pre x g).
template <uint32_t B, bool kOfP>
__global__ void __launch_bounds__(256) k_lr_fold(const LrSeg *__restrict__ d, int count, uint32_t r,
                                                 float *__restrict__ ws) {
    const unsigned tile = blockIdx.x;
    const LrSeg sd = d[seg_of<kOfP ? &LrSeg::t_pfold : &LrSeg::t_qfold>(d, count, tile)];
    const uint32_t u = (tile - (kOfP ? sd.t_pfold : sd.t_qfold)) * 256 + threadIdx.x;
    if (kOfP && sd.small) {
        if (u < sd.n) {
            const float g = reinterpret_cast<const float *>(sd.in)[u];
            ws[sd.p_at + u] = sd.pre == 1.0f ? g : g * sd.pre;
        }
        return;
    }
    if (u >= (kOfP ? sd.R : sd.C) * r) return;
    const uint32_t x = u / r, j = u % r, splits = kOfP ? sd.S : sd.T;
    const float *__restrict__ v = ws + (kOfP ? sd.pp_at : sd.qp_at) + (uint64_t)(x / B) * splits * (B * 16) + (x % B) * 16 + j;
    float t = v[0];
    for (uint32_t s = 1; s < splits; ++s) t = t + v[(uint64_t)s * (B * 16)];
    ws[(kOfP ? sd.p_at : sd.q_at) + u] = t;
}

// v summed over the workgroup in fp64, in an order only the thread index decides: the same bits in every thread
__device__ inline double block_sum(double v, double *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const double t = sh[0];
    __syncthreads();
    return t;
}

// Modified Gram-Schmidt of the summed P, in place, column by column; thread t owns rows t, t + 256, ...
__global__ void __launch_bounds__(256) k_lr_ortho(const LrSeg *__restrict__ d, uint32_t r, float *__restrict__ ws,
                                                  uint32_t *__restrict__ ctl) {
    __shared__ double sh[256];
    const LrSeg sd = d[blockIdx.x];
    if (sd.small) return;
    float *__restrict__ p = ws + sd.p_at;
    uint32_t *__restrict__ c = ctl + (uint64_t)blockIdx.x * kCtl;
    bool poison = false;
    for (uint32_t j = 0; j < r; ++j) {
        for (uint32_t i = 0; i < j; ++i) {
            double dot = 0.0;
            for (uint32_t row = threadIdx.x; row < sd.R; row += 256)
                dot += (double)p[(uint64_t)row * r + i] * (double)p[(uint64_t)row * r + j];
            dot = block_sum(dot, sh);
            for (uint32_t row = threadIdx.x; row < sd.R; row += 256)
                p[(uint64_t)row * r + j] = (float)fma(-dot, (double)p[(uint64_t)row * r + i], (double)p[(uint64_t)row * r + j]);
        }
        double nn = 0.0;
        for (uint32_t row = threadIdx.x; row < sd.R; row += 256) {
            const double x = (double)p[(uint64_t)row * r + j];
            nn += x * x;
        }
        nn = block_sum(nn, sh);
        const bool fin = nn - nn == 0.0, dead = nn == 0.0;
        poison = poison || !fin;
        const double norm = sqrt(nn);
        if (fin)
            for (uint32_t row = threadIdx.x; row < sd.R; row += 256)
                p[(uint64_t)row * r + j] = dead ? 0.0f : (float)((double)p[(uint64_t)row * r + j] / norm);
        if (threadIdx.x == 0) c[j] = fin && !dead ? 1u : 0u;
    }
    if (threadIdx.x == 0) c[kPoison] = poison ? 1u : 0u;
}

// Finiteness first, then Q- = Q^ / P (in place for the reconstruct), the stored Q and its flags: a poisoned
// tensor's state is never touched.
__global__ void __launch_bounds__(256) k_lr_settle(const LrSeg *__restrict__ d, uint32_t r, int P,
                                                   float *__restrict__ ws, uint32_t *__restrict__ ctl) {
    const LrSeg sd = d[blockIdx.x];
    if (sd.small) return;
    float *__restrict__ q = ws + sd.q_at;
    uint32_t *__restrict__ c = ctl + (uint64_t)blockIdx.x * kCtl;
    const uint32_t units = sd.C * r;
    int bad = c[kPoison] != 0;
    for (uint32_t u = threadIdx.x; u < units; u += 256) bad |= !finite_bits(q[u]);
    if (__syncthreads_or(bad)) {
        if (threadIdx.x == 0) c[kPoison] = 1u;
        return;
    }
    float *__restrict__ st = reinterpret_cast<float *>(sd.state);
    const float dv = (float)P;
    for (uint32_t u = threadIdx.x; u < units; u += 256) {
        const float v = q[u] / dv;  // correctly rounded (the compiler's default for fp32 division)
        q[u] = v;
        st[u] = v;
    }
    if (threadIdx.x < r) reinterpret_cast<uint32_t *>(st + units)[threadIdx.x] = c[threadIdx.x];
}

// out and e' of a 64 x 64 tile. Thread (rr, m) = (t / 16, t % 16) owns columns 4 m .. 4 m + 3 of rows rr + 16 it.
template <int RK>
__global__ void __launch_bounds__(256) k_lr_recon(const LrSeg *__restrict__ d, int count, int P,
                                                  const float *__restrict__ ws, const uint32_t *__restrict__ ctl) {
    __shared__ float ps[kReconRows][16];
    const unsigned tile = blockIdx.x;
    const int seg = seg_of<&LrSeg::t_recon>(d, count, tile);
    const LrSeg sd = d[seg];
    const uint32_t lt = tile - sd.t_recon, cbs = sd.C / 64, row0 = (lt / cbs) * kReconRows;
    const uint32_t m = threadIdx.x & 15, rr = threadIdx.x >> 4, col = (lt % cbs) * 64 + 4 * m;
    float *__restrict__ out = reinterpret_cast<float *>(sd.out);
    const bool vo = (sd.out & 15u) == 0, avg = sd.avg != 0;
    const float dv = (float)P, post = sd.post;
    const bool poisoned = !sd.small && ctl[(uint64_t)seg * kCtl + kPoison] != 0;
    if (sd.small || poisoned) {  // the allreduced a with the quotient and the postscale; or NaN everywhere
        for (uint32_t it = 0; it < 4; ++it) {
            const uint64_t at = (uint64_t)(row0 + rr + 16 * it) * sd.C + col;
            if (row0 + rr + 16 * it >= sd.R || at >= sd.n) continue;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (!poisoned) load4(ws + sd.p_at, (uint32_t)at, sd.n, true, v);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float y = v[i];
                if (avg) y = y / dv;
                if (post != 1.0f) y = y * post;
                v[i] = poisoned ? __uint_as_float(kNan) : y;
            }
            store4(out, (uint32_t)at, sd.n, vo, v);
        }
        return;
    }
    const float *__restrict__ ph = ws + sd.p_at;
    for (uint32_t e = threadIdx.x; e < kReconRows * 16; e += 256) {
        const uint32_t rw = e >> 4, j = e & 15;
        ps[rw][j] = row0 + rw < sd.R && j < RK ? ph[(uint64_t)(row0 + rw) * RK + j] : 0.0f;
    }
    float q[4 * RK];  // Q-[col + i][j] at i RK + j: 4 RK contiguous floats, 16-byte aligned
    const float4 *__restrict__ q4 = reinterpret_cast<const float4 *>(ws + sd.q_at + (uint64_t)col * RK);
#pragma unroll
    for (int k = 0; k < RK; ++k) {
        const float4 x = q4[k];
        q[4 * k] = x.x, q[4 * k + 1] = x.y, q[4 * k + 2] = x.z, q[4 * k + 3] = x.w;
    }
    __syncthreads();
    const float *__restrict__ a = ws + sd.a_at;
    float *__restrict__ er = reinterpret_cast<float *>(sd.res);
    const bool ve = (sd.res & 15u) == 0;
#pragma unroll
    for (uint32_t it = 0; it < 4; ++it) {
        const uint32_t rw = rr + 16 * it;
        const uint64_t at = (uint64_t)(row0 + rw) * sd.C + col;
        if (row0 + rw >= sd.R || at >= sd.n) continue;
        float p[16];
#pragma unroll
        for (int k = 0; k < (RK + 3) / 4; ++k) {
            const float4 x = *reinterpret_cast<const float4 *>(&ps[rw][4 * k]);
            p[4 * k] = x.x, p[4 * k + 1] = x.y, p[4 * k + 2] = x.z, p[4 * k + 3] = x.w;
        }
        float av[4], ev[4], ov[4];
        load4(a, (uint32_t)at, sd.n, true, av);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float dd = 0.0f;
#pragma unroll
            for (int j = 0; j < RK; ++j) dd = fmaf(p[j], q[i * RK + j], dd);
            const float left = av[i] - dd;
            ev[i] = finite_bits(left) ? left : 0.0f;
            float y = avg ? dd : dd * dv;
            if (post != 1.0f) y = y * post;
            ov[i] = y;
        }
        store4(er, (uint32_t)at, sd.n, ve, ev);
        store4(out, (uint32_t)at, sd.n, vo, ov);
    }
}

template <class F> void with_rank(int r, F f) {
    switch (r) {
#define DDL_LR_CASE(K) \
    case K: f(std::integral_constant<int, K>{}); break;
        DDL_LR_CASE(1) DDL_LR_CASE(2) DDL_LR_CASE(3) DDL_LR_CASE(4) DDL_LR_CASE(5) DDL_LR_CASE(6) DDL_LR_CASE(7) DDL_LR_CASE(8)
        DDL_LR_CASE(9) DDL_LR_CASE(10) DDL_LR_CASE(11) DDL_LR_CASE(12) DDL_LR_CASE(13) DDL_LR_CASE(14) DDL_LR_CASE(15) DDL_LR_CASE(16)
#undef DDL_LR_CASE
    }
}

inline uint64_t round4(uint64_t x) { return (x + 3) & ~uint64_t(3); }

}  // namespace

LowrankPipe::~LowrankPipe() {
    if (scratch_) (void)hipFree(scratch_);
}

void LowrankPipe::run(const LowrankSeg *segs, int count, int P, int rank, int r, hipStream_t stream,
                      const Allreduce &allreduce) {
    DDL_REQUIRE(segs && count >= 1 && P >= 1 && rank >= 0 && rank < P, DDL_STATUS_INVALID_ARGUMENT, "bad low-rank plan");
    check_lowrank_rank(r);
    const size_t table = (size_t)count * sizeof(LrSeg);
    LrSeg *t = static_cast<LrSeg *>(tables_.stage(table));
    // ws, in floats: [P of every tensor (a small one: its a)] [Q] [a] [project partials] [back-project partials]
    uint64_t np = 0, nq = 0, na = 0, npp = 0, nqp = 0;
    uint64_t tp = 0, tpf = 0, tb = 0, tqf = 0, tr = 0;
    bool any = false;  // a tensor that is compressed
    for (int i = 0; i < count; ++i) {
        const LowrankSeg &s = segs[i];
        DDL_REQUIRE(s.n >= 1 && s.src && s.dst, DDL_STATUS_INVALID_ARGUMENT, "null or empty tensor " << i);
        check_lowrank_elements(s.n);
        DDL_REQUIRE(s.op == DDL_ALLREDUCE_OP_SUM || s.op == DDL_ALLREDUCE_OP_AVG, DDL_STATUS_INVALID_ARGUMENT,
                    "the low-rank wire takes SUM or AVG");
        const LowrankShape sh = lowrank_shape(s.n, r);
        DDL_REQUIRE(sh.small || (s.residual && s.state), DDL_STATUS_INVALID_ARGUMENT, "tensor " << i << " has no residual or state");
        DDL_REQUIRE((reinterpret_cast<uintptr_t>(s.src) | reinterpret_cast<uintptr_t>(s.dst) |
                     reinterpret_cast<uintptr_t>(s.residual) | reinterpret_cast<uintptr_t>(s.state)) % 4 == 0,
                    DDL_STATUS_INVALID_ARGUMENT, "tensor " << i << " is not aligned float32 elements");
        LrSeg &e = t[i];
        e.in = reinterpret_cast<uint64_t>(s.src);
        e.out = reinterpret_cast<uint64_t>(s.dst);
        e.res = sh.small ? 0 : reinterpret_cast<uint64_t>(s.residual);
        e.state = sh.small ? 0 : reinterpret_cast<uint64_t>(s.state);
        e.n = (uint32_t)s.n, e.R = (uint32_t)sh.R, e.C = (uint32_t)sh.C, e.small = sh.small;
        e.S = (uint32_t)((sh.C + kProjCols - 1) / kProjCols), e.T = (uint32_t)((sh.R + kBackRows - 1) / kBackRows);
        const uint64_t rbs = (sh.R + 15) / 16, cbs = sh.C / 64;
        e.p_at = np, e.q_at = nq, e.a_at = na, e.pp_at = npp, e.qp_at = nqp;  // (rebased below)
        e.t_proj = (uint32_t)tp, e.t_pfold = (uint32_t)tpf, e.t_back = (uint32_t)tb, e.t_qfold = (uint32_t)tqf, e.t_recon = (uint32_t)tr;
        e.pre = s.prescale, e.post = s.postscale;
        e.avg = s.op == DDL_ALLREDUCE_OP_AVG, e.pad = 0;
        np += round4(sh.small ? s.n : sh.R * (uint64_t)r);
        tpf += ((sh.small ? s.n : sh.R * (uint64_t)r) + 255) / 256;
        tr += (sh.R + kReconRows - 1) / kReconRows * cbs;
        if (!sh.small) {
            any = true;
            nq += round4(sh.C * (uint64_t)r);
            na += round4(s.n);
            npp += rbs * e.S * 256;
            nqp += cbs * e.T * 1024;
            tp += rbs * e.S;
            tb += cbs * e.T;
            tqf += (sh.C * (uint64_t)r + 255) / 256;
        }
        DDL_REQUIRE((tp | tpf | tb | tqf | tr) < (1ull << 31), DDL_STATUS_INVALID_ARGUMENT, "low-rank plan too large");
    }
    np = (np + 63) & ~uint64_t(63), nq = (nq + 63) & ~uint64_t(63);  // the allreduced buffers start 256-byte aligned
    for (int i = 0; i < count; ++i) {
        t[i].q_at += np;
        t[i].a_at += np + nq;
        t[i].pp_at += np + nq + na;
        t[i].qp_at += np + nq + na + npp;
    }
    const uint64_t floats = np + nq + na + npp + nqp;
    const LrSeg *dd = static_cast<const LrSeg *>(tables_.upload(stream));
    float *ws = static_cast<float *>(grow_retire(scratch_, scratch_cap_, (size_t)(floats + (uint64_t)count * kCtl) * 4));
    uint32_t *ctl = reinterpret_cast<uint32_t *>(ws + floats);

    const dim3 wg(256);
    if (any) hipLaunchKernelGGL(k_lr_project, dim3((unsigned)tp), wg, 0, stream, dd, count, (uint32_t)r, ws);
    hipLaunchKernelGGL((k_lr_fold<16, true>), dim3((unsigned)tpf), wg, 0, stream, dd, count, (uint32_t)r, ws);
    DDL_HIP(hipGetLastError());
    if (P > 1) allreduce(ws, (size_t)np);
    if (any) {
        hipLaunchKernelGGL(k_lr_ortho, dim3((unsigned)count), wg, 0, stream, dd, (uint32_t)r, ws, ctl);
        hipLaunchKernelGGL(k_lr_back, dim3((unsigned)tb), wg, 0, stream, dd, count, (uint32_t)r, ws);
        hipLaunchKernelGGL((k_lr_fold<64, false>), dim3((unsigned)tqf), wg, 0, stream, dd, count, (uint32_t)r, ws);
        DDL_HIP(hipGetLastError());
        if (P > 1) allreduce(ws + np, (size_t)nq);
        hipLaunchKernelGGL(k_lr_settle, dim3((unsigned)count), wg, 0, stream, dd, (uint32_t)r, P, ws, ctl);
    }
    with_rank(r, [&](auto rk) {
        hipLaunchKernelGGL(k_lr_recon<decltype(rk)::value>, dim3((unsigned)tr), wg, 0, stream, dd, count, P, ws, ctl);
    });
    DDL_HIP(hipGetLastError());
}

}  // namespace ddl
