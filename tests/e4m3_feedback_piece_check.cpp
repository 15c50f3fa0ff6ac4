// Checks what PlanSeg::piece / cut_plan (csrc/fusion_cuts.cpp) hand to the feedback pack of the e4m3 wire: a piece of
// a request cut at granule g must carry the tensor AND the residual at element 252 g — 1008 bytes per granule, the
// tensor side, never the 256 wire bytes — and the request's true element count for its tail. The pieces' residual
// ranges must tile [0, 4 n) of the request's residual: no gap, no overlap, nothing past n; every piece offset is a
// multiple of 16 bytes. Built by tests/test_e4m3_feedback_piece_cpu.py under ASan + UBSan (the residual is a real
// allocation of exactly 4 n bytes that every piece's range is read from); exits 0 with nothing on stderr.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "fusion.h"

using ddl::PlanSeg;
using ddl::SubPlan;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                                   \
        }                                                                                 \
    } while (0)

constexpr size_t kEs = ddl::kE4m3Granule, kSes = ddl::kE4m3Elems * sizeof(float);

void check_plan(const std::vector<size_t> &elems, const std::vector<bool> &with_residual, size_t cap) {
    std::vector<std::vector<float>> src(elems.size()), res(elems.size());
    std::vector<PlanSeg> segs;
    for (size_t i = 0; i < elems.size(); ++i) {
        src[i].assign(elems[i], 1.0f);
        res[i].assign(elems[i], 2.0f);  // exactly n elements: a read past them is a sanitizer report
        PlanSeg s{src[i].data(), src[i].data(), ddl::e4m3_granules(elems[i]) * kEs};
        s.elems = elems[i];
        if (with_residual[i]) s.residual = res[i].data();
        segs.push_back(s);
    }
    std::vector<size_t> next(elems.size(), 0);  // the element every request's next piece must start at
    for (const SubPlan &sb : ddl::cut_plan(segs, cap, kEs, kSes)) {
        CHECK(sb.flat <= cap || sb.segs.size() == 1);
        for (size_t k = 0; k < sb.segs.size(); ++k) {
            const PlanSeg &p = sb.segs[k];
            const size_t i = sb.seg[k], e0 = sb.elem[k];
            CHECK(e0 == next[i] && e0 % ddl::kE4m3Elems == 0);
            CHECK(p.bytes % kEs == 0 && p.bytes == ddl::e4m3_granules(p.elems) * kEs);
            CHECK(p.src == static_cast<const void *>(src[i].data() + e0));
            CHECK((e0 * sizeof(float)) % 16 == 0);
            if (with_residual[i]) {
                CHECK(p.residual == static_cast<void *>(res[i].data() + e0));
                float sum = 0;
                for (size_t e = 0; e < p.elems; ++e) sum += static_cast<const float *>(p.residual)[e];
                CHECK(sum == 2.0f * (float)p.elems);
            } else {
                CHECK(p.residual == nullptr);
            }
            CHECK(e0 + p.elems <= elems[i]);
            CHECK(p.elems == p.bytes / kEs * ddl::kE4m3Elems || e0 + p.elems == elems[i]);  // short only at the tail
            next[i] = e0 + p.elems;
        }
    }
    for (size_t i = 0; i < elems.size(); ++i) CHECK(next[i] == elems[i]);
}

}  // namespace

int main() {
    // the engine tests' requests under their pipeline of 4096 bytes, and the handler test's 70 001 elements under
    // 64 KiB plans (PlanSeg::piece is what cuts both)
    check_plan({1, 253, 1009, 20011}, {true, true, true, true}, 4096);
    check_plan({1, 253, 1009, 20011}, {true, false, true, false}, 4096);
    check_plan({70001}, {true}, 64 << 10);
    {  // one piece by hand: granules 16 .. 31 of 20 011 elements
        std::vector<float> t(20011), r(20011);
        PlanSeg s{t.data(), t.data(), ddl::e4m3_granules(20011) * kEs};
        s.elems = 20011;
        s.residual = r.data();
        const PlanSeg p = s.piece(16 * kEs, 16 * kEs, kEs, kSes);
        CHECK(p.residual == static_cast<void *>(r.data() + 16 * 252) && p.elems == 16 * 252 && p.bytes == 4096);
        const PlanSeg last = s.piece(64 * kEs, 16 * kEs, kEs, kSes);  // granules 64 .. 79: the request ends in granule 79
        CHECK(last.residual == static_cast<void *>(r.data() + 64 * 252) && last.elems == 20011 - 64 * 252);
    }
    std::mt19937 rng(12345);
    for (int it = 0; it < 300; ++it) {
        const size_t k = 1 + rng() % 6;
        std::vector<size_t> elems(k);
        std::vector<bool> with(k);
        for (size_t i = 0; i < k; ++i) {
            elems[i] = 1 + rng() % (it % 3 ? 3000 : 40000);
            with[i] = rng() % 3 != 0;
        }
        check_plan(elems, with, (1 + rng() % 40) * 256);
    }
    if (g_failed) std::fprintf(stderr, "%d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
