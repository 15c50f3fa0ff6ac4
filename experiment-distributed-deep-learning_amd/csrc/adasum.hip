// adasum.hip — the kernels of the Adasum allreduce op and their launcher (adasum.h).
//
// The gather buffer holds P slots of `slot` floats, slot i rank i's pack of the plan: tensor s at the same
// 256-byte aligned offset of every slot (the copier's flat layout). Every tensor is cut into tiles of
// kAdaTile elements that restart at the tensor's start, as pack.hip cuts its segments, so no tile straddles
// two tensors; a workgroup finds its tensor by a scalar binary search of the table's tile0 column.
//
// Gram pass. G = X^T X with X (elements x P) is a skinny GEMM whose K is the element count. One
// v_mfma_f64_16x16x4_f64 takes A (16 x 4) and B (4 x 16) with lane l supplying A[l % 16][l / 16] and
// B[l / 16][l % 16]: for X^T X both are x_{l % 16}[e + l / 16], so ONE register feeds both operands. The sum
// over k has no order to keep, so a lane loads a float4 of one input (lane-direct: 64-byte runs per input and
// element block, no LDS on the way in), widens each component in registers — the products of widened floats
// are exact in fp64, only the accumulation rounds — and issues 4 MFMAs. With P <= 8 the 16 rows hold 16 / PP
// element blocks of PP = 2, 4, 8 inputs each (PP: P rounded up to a power of two), and G is the sum of the
// diagonal PP x PP blocks of the 16 x 16 product: the MFMA count per element falls by 16 / PP, which keeps
// the pass memory-bound at small P. Rows of inputs >= P are fed zeros.
// The 4 waves of a workgroup walk the tile's steps round-robin; their accumulators meet in LDS and are added
// in wave order, then block order, into the tile's PP x PP partial at a fixed place. k_gram_groups and
// k_gram_finish add a tensor's partials in an order only the tile count decides (groups of 256 tiles in tile order, then
// the groups in group order), the two levels of k_sumsq_finish. Bit-equal across ranks and runs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "adasum.h"

namespace ddl {

namespace {

using f64x4 = double __attribute__((ext_vector_type(4)));

constexpr uint32_t kAdaTile = 2048;  // elements of one tensor per workgroup (8 KiB of every slot)

struct AdaSeg {
    uint64_t out;    // the request's output tensor
    uint64_t off;    // the tensor's first float inside every slot (a multiple of 64)
    uint64_t n;      // elements
    uint32_t tile0;  // index of the tensor's first tile
    float post;      // the postscale, multiplied into the weights
};

// the last tensor whose tile0 <= tile (tensors without tiles share the next one's tile0)
__device__ inline int tile_tensor(const AdaSeg *__restrict__ d, int count, unsigned tile) {
    int lo = 0, hi = count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (d[mid].tile0 <= tile) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <int PP>
__global__ void __launch_bounds__(256) k_gram(const float *__restrict__ gather, uint64_t slot, int P,
                                              const AdaSeg *__restrict__ d, int count, double *__restrict__ partials) {
    constexpr int kBlocks = 16 / PP;        // element blocks stacked down the 16 rows
    constexpr uint64_t kStep = 16 * kBlocks;  // elements one wave feeds to its 4 MFMAs
    static_assert(kAdaTile % (4 * kStep) == 0, "a tile is whole steps of every wave");
    __shared__ double acc_lds[4][16][16];
    const unsigned tile = blockIdx.x;
    const AdaSeg sd = d[tile_tensor(d, count, tile)];
    const uint64_t t0 = (uint64_t)(tile - sd.tile0) * kAdaTile;
    const uint64_t tend = sd.n < t0 + kAdaTile ? sd.n : t0 + kAdaTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = lane & 15, k = lane >> 4;
    const int input = row % PP, block = row / PP;
    const bool live = input < P;
    const float *__restrict__ x = gather + (live ? (uint64_t)input * slot + sd.off : 0);
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (uint64_t e = t0 + wave * kStep; e < tend; e += 4 * kStep) {  // (wave-uniform)
        const uint64_t me = e + (uint64_t)(block * 4 + k) * 4;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (live) {
            if (me + 4 <= sd.n) {
                v = *reinterpret_cast<const float4 *>(x + me);
            } else {  // the tensor's tail: what lies behind it in the slot is not the tensor's
                if (me < sd.n) v.x = x[me];
                if (me + 1 < sd.n) v.y = x[me + 1];
                if (me + 2 < sd.n) v.z = x[me + 2];
            }
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)v.x, (double)v.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)v.y, (double)v.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)v.z, (double)v.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)v.w, (double)v.w, acc, 0, 0, 0);
    }
    // register j of lane l holds D[4 j + l / 16][l % 16]
    for (int j = 0; j < 4; ++j) acc_lds[wave][4 * j + k][row] = acc[j];
    __syncthreads();
    const int r = threadIdx.x / 16, c = threadIdx.x % 16;
    if (r < PP && c < PP) {
        double g = 0.0;
        for (int w = 0; w < 4; ++w)
            for (int b = 0; b < kBlocks; ++b) g += acc_lds[w][b * PP + r][b * PP + c];
        partials[(uint64_t)tile * (PP * PP) + r * PP + c] = g;
    }
}

// The finish, two levels, each in an order only the tile count decides (as k_sumsq_finish / k_sumsq_finish2):
// a GROUP is up to kFinGroup consecutive tiles of one tensor. k_gram_groups: one workgroup per (tensor, group),
// thread t adds entry t of the group's partials in tile order (the threads' loads of one tile are contiguous)
// into lvl[tile0 / kFinGroup + tensor + group] — distinct for distinct (tensor, group). k_gram_finish: one
// workgroup per tensor adds its group values in group order. A 64 Mi-element tensor is 128 groups of 256
// loads, not one chain of 512 strided loads per lane.
constexpr uint32_t kFinGroup = 256;

template <int PP>
__global__ void __launch_bounds__(256) k_gram_groups(const AdaSeg *__restrict__ d, unsigned max_groups,
                                                     const double *__restrict__ partials, double *__restrict__ lvl) {
    const unsigned seg = blockIdx.x / max_groups, g = blockIdx.x % max_groups;
    const AdaSeg sd = d[seg];
    const uint64_t nt = (sd.n + kAdaTile - 1) / kAdaTile, first = (uint64_t)g * kFinGroup;
    if (first >= nt || threadIdx.x >= PP * PP) return;
    const uint64_t m = nt - first < kFinGroup ? nt - first : kFinGroup;
    const double *__restrict__ v = partials + ((uint64_t)sd.tile0 + first) * (PP * PP) + threadIdx.x;
    double acc = 0.0;
#pragma unroll 8
    for (uint64_t t = 0; t < m; ++t) acc += v[t * (PP * PP)];
    lvl[((uint64_t)sd.tile0 / kFinGroup + seg + g) * (PP * PP) + threadIdx.x] = acc;
}

template <int PP>
__global__ void __launch_bounds__(256) k_gram_finish(const AdaSeg *__restrict__ d, const double *__restrict__ lvl,
                                                     double *__restrict__ gram) {
    const unsigned seg = blockIdx.x;
    if (threadIdx.x >= PP * PP) return;
    const AdaSeg sd = d[seg];
    const uint64_t nt = (sd.n + kAdaTile - 1) / kAdaTile, groups = (nt + kFinGroup - 1) / kFinGroup;
    const double *__restrict__ v = lvl + ((uint64_t)sd.tile0 / kFinGroup + seg) * (PP * PP) + threadIdx.x;
    double acc = 0.0;
#pragma unroll 8
    for (uint64_t g = 0; g < groups; ++g) acc += v[g * (PP * PP)];
    gram[(uint64_t)seg * (PP * PP) + threadIdx.x] = acc;
}

// a[0] + ... + a[N - 1] (N a power of two) as a pairwise tree: exact where the terms are equal on aligned
// power-of-two blocks (the weights 2^-k of identical inputs), which a left-to-right sum is not
template <int N> __device__ inline double tree_sum(double *a) {
    for (int s = 1; s < N; s *= 2)
        for (int i = 0; i < N; i += 2 * s) a[i] += a[i + s];
    return a[0];
}

// x summed over the PP lanes l ^ 1, l ^ 2, ... of a lane's aligned group: the same pairwise tree as tree_sum
// ((x_0 + x_1) + (x_2 + x_3)) + ..., the same bits on every lane of the group
template <int PP> __device__ inline double lane_tree_sum(double x) {
    for (int s = 1; s < PP; s *= 2) x += __shfl_xor(x, s, 64);
    return x;
}

// The coefficient step: one WAVE per tensor walks the tree on G alone (four tensors per workgroup; G and the
// nodes in LDS). A node is a weight vector over the P original inputs (PP padded); each level replaces
// adjacent pairs (a, b) by
//   (1 - a.b / (2 a.a)) a + (1 - a.b / (2 b.b)) b,   a coefficient whose own norm^2 is exactly 0 being 1,
// and carries an odd last node up unchanged. u.v = u^T G v = sum_i u_i (sum_j G_ij v_j): lane i (mod PP) takes
// row i of G a and G b as pairwise trees in registers, the three sums over i are pairwise trees across the
// lanes — exact for the weights 2^-k of identical inputs. A NaN or inf in any input reaches every weight.
template <int PP>
__global__ void __launch_bounds__(256) k_coef(const AdaSeg *__restrict__ d, int count, int P,
                                              const double *__restrict__ gram, double *__restrict__ weights) {
    __shared__ double G_lds[4][PP * PP], w_lds[4][PP][PP];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane % PP;
    const int seg = blockIdx.x * 4 + wave;
    const bool live = seg < count;  // (a wave without a tensor runs along for the barriers and stores nothing)
    const double *G = G_lds[wave];
    double(*w)[PP] = w_lds[wave];
    for (int e = lane; e < PP * PP; e += 64) {
        G_lds[wave][e] = live ? gram[(uint64_t)seg * (PP * PP) + e] : 0.0;
        w[e / PP][e % PP] = e / PP == e % PP ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int m = P; m > 1; m = (m + 1) / 2) {
        const int half = m / 2;
        for (int q = 0; q < half; ++q) {
            const double *a = w[2 * q], *b = w[2 * q + 1];
            double ga[PP], gb[PP];
            for (int j = 0; j < PP; ++j) {
                const double g = i < P && j < P ? G[i * PP + j] : 0.0;
                ga[j] = g * a[j];
                gb[j] = g * b[j];
            }
            const double ai = i < P ? a[i] : 0.0, bi = i < P ? b[i] : 0.0;
            const double Ga = tree_sum<PP>(ga), Gb = tree_sum<PP>(gb);
            const double aa = lane_tree_sum<PP>(ai * Ga), bb = lane_tree_sum<PP>(bi * Gb), ab = lane_tree_sum<PP>(ai * Gb);
            const double ca = aa == 0.0 ? 1.0 : 1.0 - ab / (2.0 * aa), cb = bb == 0.0 ? 1.0 : 1.0 - ab / (2.0 * bb);
            __syncthreads();  // every lane has read a and b
            if (lane < PP) w[q][i] = ca * ai + cb * bi;
            __syncthreads();
        }
        const double carry = w[m - 1][i];
        __syncthreads();
        if ((m & 1) && lane < PP) w[half][i] = carry;
        __syncthreads();
    }
    if (live && lane < 16) weights[(uint64_t)seg * 16 + lane] = lane < PP ? w[0][lane] * (double)d[seg].post : 0.0;
}

// The apply pass: out[e] = sum_i w_i x_i[e], the fp64 FMA chain in input order, one rounding to fp32, into
// the request's output tensor (which may not be 16-byte aligned: then element by element).
__global__ void __launch_bounds__(256) k_apply(const float *__restrict__ gather, uint64_t slot, int P,
                                               const AdaSeg *__restrict__ d, int count,
                                               const double *__restrict__ weights) {
    __shared__ double w[16];
    const unsigned tile = blockIdx.x;
    const int seg = tile_tensor(d, count, tile);
    const AdaSeg sd = d[seg];
    if (threadIdx.x < 16) w[threadIdx.x] = weights[(uint64_t)seg * 16 + threadIdx.x];
    __syncthreads();
    const uint64_t t0 = (uint64_t)(tile - sd.tile0) * kAdaTile;
    const uint64_t tend = sd.n < t0 + kAdaTile ? sd.n : t0 + kAdaTile;
    float *__restrict__ out = reinterpret_cast<float *>(sd.out);
    const float *__restrict__ x = gather + sd.off;
    const bool vec = (sd.out & 15u) == 0;
    for (uint64_t e = t0 + threadIdx.x * 4; e < tend; e += 1024) {
        if (e + 4 <= tend) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            for (int i = 0; i < P; ++i) {
                const float4 v = *reinterpret_cast<const float4 *>(x + (uint64_t)i * slot + e);
                a0 = fma(w[i], (double)v.x, a0);
                a1 = fma(w[i], (double)v.y, a1);
                a2 = fma(w[i], (double)v.z, a2);
                a3 = fma(w[i], (double)v.w, a3);
            }
            if (vec) {
                *reinterpret_cast<float4 *>(out + e) = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
            } else {
                out[e] = (float)a0;
                out[e + 1] = (float)a1;
                out[e + 2] = (float)a2;
                out[e + 3] = (float)a3;
            }
        } else {
            for (uint64_t t = e; t < tend; ++t) {
                double a = 0.0;
                for (int i = 0; i < P; ++i) a = fma(w[i], (double)x[(uint64_t)i * slot + t], a);
                out[t] = (float)a;
            }
        }
    }
}

template <class F> void with_padded_ranks(int P, F f) {  // P rounded up to a power of two, at least 2
    if (P <= 2) f(std::integral_constant<int, 2>{});
    else if (P <= 4) f(std::integral_constant<int, 4>{});
    else if (P <= 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 16>{});
}

}  // namespace

std::vector<std::pair<size_t, size_t>> adasum_plans(const std::vector<size_t> &elements, size_t limit) {
    DDL_REQUIRE(limit > 0, DDL_STATUS_INVALID_ARGUMENT, "fusion threshold must be > 0");
    std::vector<std::pair<size_t, size_t>> plans;
    size_t begin = 0, bytes = 0;
    for (size_t i = 0; i < elements.size(); ++i) {
        const size_t b = elements[i] * sizeof(float);
        if (i > begin && bytes + b > limit) {
            plans.emplace_back(begin, i);
            begin = i;
            bytes = 0;
        }
        bytes += b;
    }
    if (begin < elements.size()) plans.emplace_back(begin, elements.size());
    return plans;
}

AdasumPipe::~AdasumPipe() {
    for (Table &t : tab_) {
        if (t.ready) (void)hipEventSynchronize(t.ready);
        if (t.ready) (void)hipEventDestroy(t.ready);
        if (t.host) (void)hipHostFree(t.host);
        if (t.dev) (void)hipFree(t.dev);
    }
    if (gather_) (void)hipFree(gather_);
    if (scratch_) (void)hipFree(scratch_);
}

void *AdasumPipe::grow_(void *&buf, size_t &cap, size_t need) {
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

void AdasumPipe::run(const AdasumSeg *segs, int count, int P, int rank, hipStream_t stream, SegmentCopier &copier,
                     const Gather &gather) {
    DDL_REQUIRE(P >= 1 && P <= kAdasumMaxRanks, DDL_STATUS_INVALID_ARGUMENT,
                "DDL_ALLREDUCE_OP_ADASUM takes a communicator of at most " << kAdasumMaxRanks << " ranks, not " << P);
    DDL_REQUIRE(segs && count >= 1 && rank >= 0 && rank < P, DDL_STATUS_INVALID_ARGUMENT, "bad Adasum plan");
    std::vector<CopySeg> pack((size_t)count);
    std::vector<size_t> bytes((size_t)count);
    uint64_t tiles = 0, max_groups = 1;  // max_groups: of the longest tensor (k_gram_groups)
    for (int i = 0; i < count; ++i) {
        DDL_REQUIRE(segs[i].n == 0 || (segs[i].src && segs[i].dst), DDL_STATUS_INVALID_ARGUMENT, "null tensor " << i);
        DDL_REQUIRE(reinterpret_cast<uintptr_t>(segs[i].dst) % 4 == 0, DDL_STATUS_INVALID_ARGUMENT,
                    "tensor " << i << " is not aligned float32 elements");
        bytes[(size_t)i] = segs[i].n * sizeof(float);
        pack[(size_t)i] = CopySeg{const_cast<void *>(segs[i].src), bytes[(size_t)i], DDL_ALLREDUCE_OP_SUM, segs[i].prescale};
        const uint64_t nt = (segs[i].n + kAdaTile - 1) / kAdaTile;
        tiles += nt;
        max_groups = std::max<uint64_t>(max_groups, (nt + kFinGroup - 1) / kFinGroup);
    }
    DDL_REQUIRE(tiles < (1ull << 31) && (uint64_t)count * max_groups < (1ull << 31), DDL_STATUS_INVALID_ARGUMENT, "Adasum plan too large");
    const size_t slot_bytes = SegmentCopier::flat_bytes(bytes.data(), count);
    if (slot_bytes == 0 || tiles == 0) return;
    const uint64_t slot = slot_bytes / sizeof(float);

    // 1) this rank's slot, then every rank's
    char *g = static_cast<char *>(grow_(gather_, gather_cap_, (size_t)P * slot_bytes));
    char *own = g + (size_t)rank * slot_bytes;
    copier.run(CopyLaunch{0, own, stream, DDL_FLOAT}, pack.data(), count);
    if (P > 1) gather(own, g, slot);

    // 2) the table
    Table &tb = tab_[next_];
    next_ = (next_ + 1) % kTables;
    if (!tb.ready) DDL_HIP(hipEventCreateWithFlags(&tb.ready, hipEventDisableTiming));
    else DDL_HIP(hipEventSynchronize(tb.ready));  // its last upload has been consumed
    const size_t table = (size_t)count * sizeof(AdaSeg);
    if (table > tb.cap) {
        retire_host(tb.host);
        retire_device(tb.dev);
        tb.host = tb.dev = nullptr;
        tb.cap = table + table / 2;
        DDL_HIP(hipHostMalloc(&tb.host, tb.cap, hipHostMallocDefault));
        DDL_HIP(hipMalloc(&tb.dev, tb.cap));
    }
    AdaSeg *t = static_cast<AdaSeg *>(tb.host);
    uint64_t off = 0, tl = 0;
    for (int i = 0; i < count; ++i) {
        t[i] = AdaSeg{reinterpret_cast<uint64_t>(segs[i].dst), off / sizeof(float), segs[i].n, (uint32_t)tl, segs[i].postscale};
        off += (bytes[(size_t)i] + 255) & ~uint64_t(255);
        tl += (segs[i].n + kAdaTile - 1) / kAdaTile;
    }
    DDL_HIP(hipMemcpyAsync(tb.dev, tb.host, table, hipMemcpyHostToDevice, stream));
    DDL_HIP(hipEventRecord(tb.ready, stream));
    const AdaSeg *dd = static_cast<const AdaSeg *>(tb.dev);
    const float *gf = reinterpret_cast<const float *>(g);

    // 3) Gram, coefficients, apply
    with_padded_ranks(P, [&](auto pp) {
        constexpr int PP = decltype(pp)::value;
        const size_t lvl_n = (size_t)(tiles / kFinGroup) + (size_t)count + 1;  // group values (k_gram_groups)
        const size_t need = ((size_t)tiles + lvl_n + (size_t)count) * PP * PP * sizeof(double) + (size_t)count * 16 * sizeof(double);
        double *partials = static_cast<double *>(grow_(scratch_, scratch_cap_, need));
        double *lvl = partials + (size_t)tiles * PP * PP, *gram = lvl + lvl_n * PP * PP, *weights = gram + (size_t)count * PP * PP;
        hipLaunchKernelGGL(k_gram<PP>, dim3((unsigned)tiles), dim3(256), 0, stream, gf, slot, P, dd, count, partials);
        hipLaunchKernelGGL(k_gram_groups<PP>, dim3((unsigned)(count * max_groups)), dim3(256), 0, stream, dd,
                           (unsigned)max_groups, partials, lvl);
        hipLaunchKernelGGL(k_gram_finish<PP>, dim3((unsigned)count), dim3(256), 0, stream, dd, lvl, gram);
        hipLaunchKernelGGL(k_coef<PP>, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, stream, dd, count, P, gram, weights);
        hipLaunchKernelGGL(k_apply, dim3((unsigned)tiles), dim3(256), 0, stream, gf, slot, P, dd, count, weights);
    });
    DDL_HIP(hipGetLastError());
}

}  // namespace ddl
