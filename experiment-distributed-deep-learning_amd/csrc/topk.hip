// topk.hip — the kernels of the top-k wire and their launcher (topk.h).
//
// Every tensor is cut into tiles of kTile elements that restart at the tensor's start, so no tile straddles two
// tensors; a workgroup finds its tensor by a scalar binary search of the table's tile0 column (as adasum.hip).
// A lane owns 8 consecutive elements of its tile (two 16-byte vectors where the pointer is 16-byte aligned,
// element by element otherwise and at the tensor's tail), so lane order is index order.
//
// Select. key(a) = bits(a) & 0x7fffffff (a NaN above inf). The k-th largest key T is found digit by digit,
// 11 / 10 / 10 bits from the top: a histogram pass counts, per tensor, the digit of every element whose higher
// digits equal the prefix fixed so far (tile histograms in LDS, flushed by integer atomics into the tensor's
// global one: order-independent, so deterministic); k_scan, one workgroup per tensor, walks the histogram from
// the top, fixes the digit whose bin holds the k-th element and leaves the count still to take inside that bin.
// After the third scan the prefix is T and the count is the number of ties (key == T) to take. The first pass
// also forms a = fl32(prescale x g) + r — two roundings, never an fma — and stores it over r: the later passes
// and the emit read r alone. A 16 / 15 split (two refinement passes) would save one read of r, but 64 Ki bins
// are 256 KiB, above the 160 KiB of LDS, and a global histogram that wide loses the tile-local atomics; an
// 8-bit split takes four passes. Neither was built.
//
// Emit. k_count leaves per tile (#key > T, #key == T). k_offsets, one workgroup per tensor, turns them into
// the tile's first output position and its allowance of ties — the ties are taken in ascending index, so tile t
// may take min(eq_t, ties - eq before t) — and writes the positions as the slot's tile_start section.
// k_emit scans (gt, eq) over the tile's lanes in one packed prefix sum, so a lane knows its output position in
// closed form: start + gt before + min(eq before, allowance). It writes (index, value) in ascending index and
// zeroes r where it selected.
//
// Slot of a rank, per tensor and the same on every rank, each section 256-byte aligned:
//   tile_start[ntiles + 1] uint32 | idx[k] uint32 | val[k] fp32
//
// Combine. One workgroup owns one output tile: 8 KiB of LDS zeroed, then for q = 0 .. P - 1 the entries
// [tile_start_q[t], tile_start_q[t + 1]) of rank q added at idx - t0 (indices are unique within a rank: a
// barrier between ranks is all the order needs), then one write of the tile: the quotient by (float)P for AVG,
// the postscale, 16-byte stores where the output is aligned.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "topk.h"

namespace ddl {

namespace {

constexpr uint32_t kTile = 2048;            // elements of one tensor per workgroup: 8 per lane
constexpr uint32_t kBins = 2048;            // the widest digit (11 bits)
constexpr uint32_t kState = kBins + 4;      // per tensor: the histogram, then
constexpr uint32_t kPrefix = kBins, kRemain = kBins + 1;  // the key digits fixed so far, the count still to take
constexpr uint32_t kKeyMask = 0x7fffffffu;

struct TkSeg {
    uint64_t in, out, res;  // the request's tensors and this rank's residual
    uint64_t ts, idx, val;  // the tensor's sections inside every slot, in 4-byte words
    uint32_t n, k;          // elements, entries sent
    uint32_t tile0, ntiles;
    float pre, post;
    uint32_t avg;
};

// the last tensor whose tile0 <= tile (every tensor has at least one tile)
__device__ inline int tile_tensor(const TkSeg *__restrict__ d, int count, unsigned tile) {
    int lo = 0, hi = count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (d[mid].tile0 <= tile) lo = mid;
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

// The lane's 8 elements [base, base + 8) of a tensor of n: how many exist (0 .. 8); the others read +0.0.
__device__ inline int load8(const float *__restrict__ p, uint32_t base, uint32_t n, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.0f;
    if (base >= n) return 0;
    if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0 && n - base >= 8) {
        const float4 a = *reinterpret_cast<const float4 *>(p + base), b = *reinterpret_cast<const float4 *>(p + base + 4);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
        return 8;
    }
    const int m = n - base < 8 ? (int)(n - base) : 8;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < m) v[j] = p[base + j];
    return m;
}

__device__ inline void store8(float *__restrict__ p, uint32_t base, int m, const float (&v)[8]) {
    if (m == 8 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        *reinterpret_cast<float4 *>(p + base) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4 *>(p + base + 4) = make_float4(v[4], v[5], v[6], v[7]);
        return;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < m) p[base + j] = v[j];
}

__global__ void __launch_bounds__(256) k_topk_init(const TkSeg *__restrict__ d, uint32_t *__restrict__ state) {
    uint32_t *st = state + (uint64_t)blockIdx.x * kState;
    for (uint32_t b = threadIdx.x; b < kState; b += 256) st[b] = b == kRemain ? d[blockIdx.x].k : 0u;
}

// One histogram pass. FIRST: a = fl32(pre x g) + r stored over r, the digit key >> 20 of every element.
// Otherwise the digit (key >> SHIFT) & 1023 of the elements with key >> (SHIFT + 10) == prefix.
template <bool FIRST, int SHIFT>
__global__ void __launch_bounds__(256) k_topk_hist(const TkSeg *__restrict__ d, int count, uint32_t *__restrict__ state) {
    constexpr uint32_t kDigits = FIRST ? kBins : 1024u;
    __shared__ uint32_t h[kDigits];
    const unsigned tile = blockIdx.x;
    const int seg = tile_tensor(d, count, tile);
    const TkSeg sd = d[seg];
    uint32_t *st = state + (uint64_t)seg * kState;
    for (uint32_t b = threadIdx.x; b < kDigits; b += 256) h[b] = 0;
    __syncthreads();
    const uint32_t base = (tile - sd.tile0) * kTile + threadIdx.x * 8;
    float *__restrict__ r = reinterpret_cast<float *>(sd.res);
    float v[8];
    int m;
    if constexpr (FIRST) {
        float g[8];
        m = load8(reinterpret_cast<const float *>(sd.in), base, sd.n, g);
        load8(r, base, sd.n, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = accumulate(g[j], sd.pre, v[j]);
        if (m) store8(r, base, m, v);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < m) atomicAdd(&h[(__float_as_uint(v[j]) & kKeyMask) >> 20], 1u);
    } else {
        const uint32_t prefix = st[kPrefix];
        m = load8(r, base, sd.n, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t key = __float_as_uint(v[j]) & kKeyMask;
            if (j < m && (key >> (SHIFT + 10)) == prefix) atomicAdd(&h[(key >> SHIFT) & 1023u], 1u);
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kDigits; b += 256)
        if (h[b]) atomicAdd(&st[b], h[b]);
}

// One workgroup per tensor: the digit whose bin holds the `remain`-th largest of the elements counted, from the
// top; prefix = prefix << log2(DIGITS) | digit, remain -= the elements in the bins above. Zeroes the histogram
// for the next pass.
template <uint32_t DIGITS>
__global__ void __launch_bounds__(256) k_topk_scan(uint32_t *__restrict__ state) {
    constexpr uint32_t kPer = DIGITS / 256;
    __shared__ uint32_t s[256];
    uint32_t *st = state + (uint64_t)blockIdx.x * kState;
    uint32_t c[kPer], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) {
        c[j] = st[threadIdx.x * kPer + j];
        st[threadIdx.x * kPer + j] = 0;
        sum += c[j];
    }
    s[threadIdx.x] = sum;
    const uint32_t prefix = st[kPrefix], remain = st[kRemain];
    __syncthreads();  // every lane has read prefix and remain
    uint32_t above = 0;
    for (uint32_t u = threadIdx.x + 1; u < 256; ++u) above += s[u];
#pragma unroll
    for (int j = (int)kPer - 1; j >= 0; --j) {
        if (above < remain && remain <= above + c[j]) {  // exactly one bin of one lane
            st[kPrefix] = prefix * DIGITS + threadIdx.x * kPer + (uint32_t)j;
            st[kRemain] = remain - above;
        }
        above += c[j];
    }
}

// (#key > T) << 16 | (#key == T) of a lane's elements (at most 8 each)
__device__ inline uint32_t count8(const float (&v)[8], int m, uint32_t T) {
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t key = __float_as_uint(v[j]) & kKeyMask;
        if (j < m) c += key > T ? 0x10000u : key == T ? 1u : 0u;
    }
    return c;
}

// The packed counts summed over the lanes before this one in the workgroup (a tile holds at most 2048 of
// each, so the halves never carry into each other); *total: over the whole workgroup.
__device__ inline uint32_t block_exclusive(uint32_t c, uint32_t *total) {
    __shared__ uint32_t waves[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = c;
#pragma unroll
    for (int s = 1; s < 64; s *= 2) {
        const uint32_t up = __shfl_up(inc, s, 64);
        if (lane >= s) inc += up;
    }
    if (lane == 63) waves[wave] = inc;
    __syncthreads();
    uint32_t before = inc - c, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += waves[w];
        all += waves[w];
    }
    *total = all;
    return before;
}

__global__ void __launch_bounds__(256) k_topk_count(const TkSeg *__restrict__ d, int count, const uint32_t *__restrict__ state,
                                                    uint2 *__restrict__ cnt) {
    const unsigned tile = blockIdx.x;
    const int seg = tile_tensor(d, count, tile);
    const TkSeg sd = d[seg];
    const uint32_t T = state[(uint64_t)seg * kState + kPrefix];
    float v[8];
    const int m = load8(reinterpret_cast<const float *>(sd.res), (tile - sd.tile0) * kTile + threadIdx.x * 8, sd.n, v);
    uint32_t total;
    block_exclusive(count8(v, m, T), &total);
    if (threadIdx.x == 0) cnt[tile] = make_uint2(total >> 16, total & 0xffffu);
}

// One workgroup per tensor: lane l takes the tensor's tiles [l c, (l + 1) c), c = ceil(ntiles / 256); their
// sums meet in LDS, a lane adds those of the lanes before it and walks its tiles. With G / E the gt / eq
// counts of the tiles before tile t: tile_start[t] = G + min(E, ties), allowance[t] = min(eq_t, ties - min(E, ties)),
// kept in cnt[t].y; tile_start[ntiles] = k.
__global__ void __launch_bounds__(256) k_topk_offsets(const TkSeg *__restrict__ d, const uint32_t *__restrict__ state,
                                                      uint2 *__restrict__ cnt, uint32_t *__restrict__ slot) {
    __shared__ uint32_t sg[256], se[256];
    const TkSeg sd = d[blockIdx.x];
    const uint32_t ties = state[(uint64_t)blockIdx.x * kState + kRemain];
    const uint32_t per = (sd.ntiles + 255) / 256;
    const uint32_t lo = min(threadIdx.x * per, sd.ntiles), hi = min(lo + per, sd.ntiles);
    uint2 *__restrict__ c = cnt + sd.tile0;
    uint32_t g = 0, e = 0;
    for (uint32_t t = lo; t < hi; ++t) {
        g += c[t].x;
        e += c[t].y;
    }
    sg[threadIdx.x] = g;
    se[threadIdx.x] = e;
    __syncthreads();
    uint32_t G = 0, E = 0;
    for (uint32_t u = 0; u < threadIdx.x; ++u) {
        G += sg[u];
        E += se[u];
    }
    uint32_t *__restrict__ ts = slot + sd.ts;
    for (uint32_t t = lo; t < hi; ++t) {
        const uint2 ct = c[t];
        const uint32_t taken = min(E, ties);
        ts[t] = G + taken;
        c[t].y = min(ct.y, ties - taken);
        G += ct.x;
        E += ct.y;
    }
    if (threadIdx.x == 0) ts[sd.ntiles] = sd.k;
}

__global__ void __launch_bounds__(256) k_topk_emit(const TkSeg *__restrict__ d, int count, const uint32_t *__restrict__ state,
                                                   const uint2 *__restrict__ cnt, uint32_t *__restrict__ slot) {
    const unsigned tile = blockIdx.x;
    const int seg = tile_tensor(d, count, tile);
    const TkSeg sd = d[seg];
    const uint32_t T = state[(uint64_t)seg * kState + kPrefix];
    const uint32_t base = (tile - sd.tile0) * kTile + threadIdx.x * 8;
    float *__restrict__ r = reinterpret_cast<float *>(sd.res);
    float v[8];
    const int m = load8(r, base, sd.n, v);
    uint32_t total;
    const uint32_t before = block_exclusive(count8(v, m, T), &total);
    const uint32_t allow = cnt[tile].y;
    uint32_t eq = before & 0xffffu;  // ties before this element, in index order
    uint32_t pos = slot[sd.ts + (tile - sd.tile0)] + (before >> 16) + min(eq, allow);
    uint32_t *__restrict__ idx = slot + sd.idx;
    float *__restrict__ val = reinterpret_cast<float *>(slot + sd.val);
    bool any = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t key = __float_as_uint(v[j]) & kKeyMask;
        const bool tie = j < m && key == T;
        const bool sel = j < m && (key > T || (tie && eq < allow));
        if (tie) ++eq;
        if (sel) {
            if (pos < sd.k) {  // (always: the counts add up to k)
                idx[pos] = base + j;
                val[pos] = v[j];
            }
            ++pos;
            v[j] = 0.0f;
            any = true;
        }
    }
    if (any) store8(r, base, m, v);
}

// out tile = post(sum over the ranks that selected the element, in rank order, from +0.0)
__global__ void __launch_bounds__(256) k_topk_combine(const uint32_t *__restrict__ gather, uint64_t slot_words, int P,
                                                      const TkSeg *__restrict__ d, int count) {
    __shared__ float acc[kTile];
    const unsigned tile = blockIdx.x;
    const TkSeg sd = d[tile_tensor(d, count, tile)];
    const uint32_t lt = tile - sd.tile0, t0 = lt * kTile;
    for (uint32_t e = threadIdx.x; e < kTile; e += 256) acc[e] = 0.0f;
    __syncthreads();
    for (int q = 0; q < P; ++q) {
        const uint32_t *__restrict__ s = gather + (uint64_t)q * slot_words;
        const uint32_t *__restrict__ idx = s + sd.idx;
        const float *__restrict__ val = reinterpret_cast<const float *>(s + sd.val);
        const uint32_t b = s[sd.ts + lt], e = min(s[sd.ts + lt + 1], sd.k);
        for (uint32_t j = b + threadIdx.x; j < e; j += 256) {
            const uint32_t at = idx[j] - t0;
            if (at < kTile) acc[at] += val[j];  // (always: rank q's tile range holds this tile's indices)
        }
        __syncthreads();
    }
    const uint32_t tend = min(sd.n - t0, kTile);
    const float dv = (float)P;
    auto post = [&](float y) {  // the correctly rounded quotient, then the factor: two roundings, as the unpack's
        if (sd.avg) y = y / dv;
        return sd.post == 1.0f ? y : y * sd.post;
    };
    float *__restrict__ out = reinterpret_cast<float *>(sd.out) + t0;
    const bool vec = (sd.out & 15u) == 0;
    for (uint32_t e = threadIdx.x * 4; e < tend; e += 1024) {
        if (vec && e + 4 <= tend) {
            *reinterpret_cast<float4 *>(out + e) = make_float4(post(acc[e]), post(acc[e + 1]), post(acc[e + 2]), post(acc[e + 3]));
        } else {
            for (uint32_t t = e; t < tend && t < e + 4; ++t) out[t] = post(acc[t]);
        }
    }
}

inline uint64_t words256(uint64_t words) { return (words + 63) & ~uint64_t(63); }  // a section: whole 256 bytes

}  // namespace

TopkPipe::~TopkPipe() {
    for (Table &t : tab_) {
        if (t.ready) (void)hipEventSynchronize(t.ready);
        if (t.ready) (void)hipEventDestroy(t.ready);
        if (t.host) (void)hipHostFree(t.host);
        if (t.dev) (void)hipFree(t.dev);
    }
    if (gather_) (void)hipFree(gather_);
    if (scratch_) (void)hipFree(scratch_);
}

void *TopkPipe::grow_(void *&buf, size_t &cap, size_t need) {
    if (need > cap) {  // may still be read on the device: retired, not freed (common.h retire_device)
        if (buf) retire_device(buf);
        buf = nullptr;
        cap = 0;
        const size_t sz = need + need / 2;
        DDL_HIP(hipMalloc(&buf, sz));
        cap = sz;
    }
    return buf;
}

void TopkPipe::run(const TopkSeg *segs, int count, int P, int rank, long long ppm, hipStream_t stream, const Gather &gather) {
    DDL_REQUIRE(segs && count >= 1 && P >= 1 && rank >= 0 && rank < P, DDL_STATUS_INVALID_ARGUMENT, "bad top-k plan");
    check_topk_ppm(ppm);
    // the table, in pinned staging
    Table &tb = tab_[next_];
    next_ = (next_ + 1) % kTables;
    if (!tb.ready) DDL_HIP(hipEventCreateWithFlags(&tb.ready, hipEventDisableTiming));
    else DDL_HIP(hipEventSynchronize(tb.ready));  // its last upload has been consumed
    const size_t table = (size_t)count * sizeof(TkSeg);
    if (table > tb.cap) {
        retire_host(tb.host);
        retire_device(tb.dev);
        tb.host = tb.dev = nullptr;
        tb.cap = table + table / 2;
        DDL_HIP(hipHostMalloc(&tb.host, tb.cap, hipHostMallocDefault));
        DDL_HIP(hipMalloc(&tb.dev, tb.cap));
    }
    TkSeg *t = static_cast<TkSeg *>(tb.host);
    uint64_t words = 0, tiles = 0;
    for (int i = 0; i < count; ++i) {
        const TopkSeg &s = segs[i];
        check_topk_elements(s.n);
        DDL_REQUIRE(s.n >= 1 && s.src && s.dst && s.residual, DDL_STATUS_INVALID_ARGUMENT, "null or empty tensor " << i);
        DDL_REQUIRE((reinterpret_cast<uintptr_t>(s.src) | reinterpret_cast<uintptr_t>(s.dst) |
                     reinterpret_cast<uintptr_t>(s.residual)) % 4 == 0,
                    DDL_STATUS_INVALID_ARGUMENT, "tensor " << i << " is not aligned float32 elements");
        DDL_REQUIRE(s.op == DDL_ALLREDUCE_OP_SUM || s.op == DDL_ALLREDUCE_OP_AVG, DDL_STATUS_INVALID_ARGUMENT,
                    "the top-k wire takes SUM or AVG");
        const uint64_t nt = (s.n + kTile - 1) / kTile, k = topk_count(s.n, ppm);
        TkSeg &e = t[i];
        e.in = reinterpret_cast<uint64_t>(s.src);
        e.out = reinterpret_cast<uint64_t>(s.dst);
        e.res = reinterpret_cast<uint64_t>(s.residual);
        e.ts = words;
        e.idx = e.ts + words256(nt + 1);
        e.val = e.idx + words256(k);
        words = e.val + words256(k);
        e.n = (uint32_t)s.n;
        e.k = (uint32_t)k;
        e.tile0 = (uint32_t)tiles;
        e.ntiles = (uint32_t)nt;
        e.pre = s.prescale;
        e.post = s.postscale;
        e.avg = s.op == DDL_ALLREDUCE_OP_AVG;
        tiles += nt;
    }
    DDL_REQUIRE(tiles < (1ull << 31), DDL_STATUS_INVALID_ARGUMENT, "top-k plan too large");
    DDL_HIP(hipMemcpyAsync(tb.dev, tb.host, table, hipMemcpyHostToDevice, stream));
    DDL_HIP(hipEventRecord(tb.ready, stream));
    const TkSeg *dd = static_cast<const TkSeg *>(tb.dev);

    const size_t slot_bytes = (size_t)words * 4;
    char *g = static_cast<char *>(grow_(gather_, gather_cap_, (size_t)P * slot_bytes));
    uint32_t *own = reinterpret_cast<uint32_t *>(g + (size_t)rank * slot_bytes);
    uint32_t *state = static_cast<uint32_t *>(grow_(scratch_, scratch_cap_, ((size_t)count * kState + (size_t)tiles * 2) * 4));
    uint2 *cnt = reinterpret_cast<uint2 *>(state + (size_t)count * kState);

    const dim3 per_tile((unsigned)tiles), per_tensor((unsigned)count), wg(256);
    // 1) select: the threshold key and the ties to take, per tensor
    hipLaunchKernelGGL(k_topk_init, per_tensor, wg, 0, stream, dd, state);
    hipLaunchKernelGGL((k_topk_hist<true, 20>), per_tile, wg, 0, stream, dd, count, state);
    hipLaunchKernelGGL(k_topk_scan<kBins>, per_tensor, wg, 0, stream, state);
    hipLaunchKernelGGL((k_topk_hist<false, 10>), per_tile, wg, 0, stream, dd, count, state);
    hipLaunchKernelGGL(k_topk_scan<1024>, per_tensor, wg, 0, stream, state);
    hipLaunchKernelGGL((k_topk_hist<false, 0>), per_tile, wg, 0, stream, dd, count, state);
    hipLaunchKernelGGL(k_topk_scan<1024>, per_tensor, wg, 0, stream, state);
    // 2) emit into this rank's slot
    hipLaunchKernelGGL(k_topk_count, per_tile, wg, 0, stream, dd, count, state, cnt);
    hipLaunchKernelGGL(k_topk_offsets, per_tensor, wg, 0, stream, dd, state, cnt, own);
    hipLaunchKernelGGL(k_topk_emit, per_tile, wg, 0, stream, dd, count, state, cnt, own);
    DDL_HIP(hipGetLastError());
    // 3) every rank's slot, then the dense result
    if (P > 1) gather(own, g, (size_t)words);
    hipLaunchKernelGGL(k_topk_combine, per_tile, wg, 0, stream, reinterpret_cast<const uint32_t *>(g), words, P, dd, count);
    DDL_HIP(hipGetLastError());
}

}  // namespace ddl
