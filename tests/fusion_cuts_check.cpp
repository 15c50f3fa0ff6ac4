// Checks cut_plan (csrc/fusion_cuts.cpp) against a closed form of the cuts, not against a copy of its
// loop. Lay the segments on the padded stream: segment i starts at the sum of round256(bytes[j]) for
// j < i. The stream is cut at every multiple of cap; the piece at stream position pos belongs to
// sub-plan pos / cap; an empty segment is one empty piece in sub-plan start_i / cap; a sub-plan's flat is
// the sum of round256(len) over its pieces. Built by tests/test_fusion_cuts_cpu.py under ASan + UBSan;
// exits 0 with nothing on stderr when every check holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "fusion.h"

using ddl::PlanSeg;
using ddl::SubPlan;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                          \
        }                                                                        \
    } while (0)

size_t round256(size_t n) { return (n + 255) & ~size_t(255); }

struct Piece {
    size_t seg, off, len;
    bool operator==(const Piece &o) const { return seg == o.seg && off == o.off && len == o.len; }
};

// the closed form: sub-plan -> its pieces (segment, wire offset in it, wire bytes)
std::vector<std::vector<Piece>> expected(const std::vector<size_t> &bytes, size_t cap) {
    std::vector<std::vector<Piece>> subs;
    auto put = [&](size_t sub, Piece p) {
        if (subs.size() <= sub) subs.resize(sub + 1);
        subs[sub].push_back(p);
    };
    size_t start = 0;
    for (size_t i = 0; i < bytes.size(); ++i) {
        if (bytes[i] == 0) put(start / cap, Piece{i, 0, 0});
        for (size_t pos = start; pos < start + bytes[i];) {
            const size_t next = std::min(start + bytes[i], (pos / cap + 1) * cap);  // the next cut, or the end
            put(pos / cap, Piece{i, pos - start, next - pos});
            pos = next;
        }
        start += round256(bytes[i]);
    }
    return subs;
}

// Segments with distinct values in every field, so that a swapped or dropped field shows. The tensors
// and residuals are fake addresses: nothing is dereferenced.
std::vector<PlanSeg> make_plan(const std::vector<size_t> &bytes) {
    std::vector<PlanSeg> segs;
    for (size_t i = 0; i < bytes.size(); ++i) {
        PlanSeg s{reinterpret_cast<const void *>(0x10000000 + 0x100000 * i), reinterpret_cast<void *>(0x40000000 + 0x100000 * i),
                  bytes[i]};
        s.op = i % 2 ? DDL_ALLREDUCE_OP_AVG : DDL_ALLREDUCE_OP_SUM;
        s.prescale = 2.0f + (float)i;
        s.postscale = 0.5f / (float)(i + 1);
        s.residual = i % 3 == 1 ? nullptr : reinterpret_cast<void *>(0x70000000 + 0x100000 * i);
        s.stream = ddl::WireStream{0xabc0 + i, 1000 * (i + 1), i % 2};
        s.want = i % 3 != 0;
        segs.push_back(s);
    }
    return segs;
}

void check_plan(const std::vector<size_t> &bytes, size_t cap, size_t es, size_t ses) {
    const std::vector<PlanSeg> segs = make_plan(bytes);
    const std::vector<SubPlan> subs = ddl::cut_plan(segs, cap, es, ses);
    const std::vector<std::vector<Piece>> want = expected(bytes, cap);
    CHECK(subs.size() == want.size());
    std::vector<size_t> covered(bytes.size(), 0), pieces(bytes.size(), 0);  // per segment, in the order met
    for (size_t j = 0; j < subs.size() && j < want.size(); ++j) {
        const SubPlan &sb = subs[j];
        CHECK(sb.segs.size() == want[j].size() && sb.seg.size() == sb.segs.size() && sb.elem.size() == sb.segs.size());
        size_t flat = 0;
        for (size_t k = 0; k < sb.segs.size() && k < want[j].size(); ++k) {
            const PlanSeg &p = sb.segs[k];
            const size_t i = sb.seg[k];
            CHECK(i < segs.size());
            if (i >= segs.size()) continue;
            const PlanSeg &s = segs[i];
            const size_t off = covered[i];  // contiguous, in order
            CHECK((Piece{i, off, p.bytes} == want[j][k]));
            CHECK(off % 256 == 0);  // every cut a multiple of 256 from the segment start
            CHECK(p.src == static_cast<const char *>(s.src) + off / es * ses);
            CHECK(p.dst == static_cast<char *>(s.dst) + off / es * ses);
            if (s.residual) CHECK(p.residual == static_cast<char *>(s.residual) + off / es * ses);
            else CHECK(p.residual == nullptr);
            CHECK(p.stream.key == s.stream.key && p.stream.on == s.stream.on && p.stream.first == s.stream.first + off / es);
            CHECK(p.op == s.op && p.prescale == s.prescale && p.postscale == s.postscale && p.want == s.want);
            CHECK(sb.elem[k] == off / es);
            CHECK(p.bytes <= cap);
            covered[i] += p.bytes;
            ++pieces[i];
            flat += round256(p.bytes);
        }
        CHECK(sb.flat == flat && flat <= cap);
    }
    for (size_t i = 0; i < bytes.size(); ++i) CHECK(covered[i] == bytes[i] && pieces[i] >= 1);  // [0, bytes) covered
}

// bytes = {258, 0, 512, 2, 1026, 0} with cap 512: six sub-plans, the last one empty (flat 0)
void check_pinned() {
    const std::vector<size_t> bytes{258, 0, 512, 2, 1026, 0};
    const std::vector<std::vector<Piece>> want{{{0, 0, 258}}, {{1, 0, 0}, {2, 0, 512}}, {{3, 0, 2}, {4, 0, 256}},
                                               {{4, 256, 512}},  {{4, 768, 258}},        {{5, 0, 0}}};
    CHECK(expected(bytes, 512) == want);
    const std::vector<SubPlan> subs = ddl::cut_plan(make_plan(bytes), 512, 2, 4);
    CHECK(subs.size() == want.size());
    for (size_t j = 0; j < subs.size() && j < want.size(); ++j) {
        CHECK(subs[j].segs.size() == want[j].size());
        for (size_t k = 0; k < subs[j].segs.size() && k < want[j].size(); ++k)
            CHECK((Piece{subs[j].seg[k], subs[j].elem[k] * 2, subs[j].segs[k].bytes} == want[j][k]));
    }
    CHECK(subs.back().flat == 0);
    check_plan(bytes, 512, 2, 4);
}

}  // namespace

int main() {
    check_pinned();
    const size_t sizes[] = {0, 2, 4, 254, 256, 258, 510, 512, 514, 1022, 1026, 2050};
    std::mt19937 rng(20240607);
    int plans = 0;
    for (size_t cap : {size_t(256), size_t(512), size_t(768)})
        for (int wire = 0; wire < 2; ++wire) {
            const size_t es = wire ? 2 : 4, ses = 4;
            for (int rep = 0; rep < 80; ++rep) {
                std::vector<size_t> bytes(1 + rng() % 7);
                for (size_t &b : bytes) {
                    do b = sizes[rng() % (sizeof(sizes) / sizeof(sizes[0]))];
                    while (b % es != 0);  // whole elements on the wire
                }
                check_plan(bytes, cap, es, ses);
                ++plans;
            }
        }
    if (g_failed) std::fprintf(stderr, "%d checks failed over %d plans\n", g_failed, plans);
    return g_failed ? 1 : 0;
}
