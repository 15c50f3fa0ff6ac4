// fusion_cuts.cpp — how a fusion plan is cut into sub-plans (fusion.h). No HIP runtime call here, so
// tests/fusion_cuts_check.cpp checks it without a GPU.
#include "fusion.h"

namespace ddl {

PlanSeg PlanSeg::piece(size_t off, size_t len, size_t es, size_t ses) const {
    PlanSeg p = *this;
    const size_t e = off / es;  // the residual and the random bits are indexed like the tensor
    p.src = static_cast<const char *>(src) + e * ses;
    p.dst = static_cast<char *>(dst) + e * ses;
    p.bytes = len;
    if (residual) p.residual = static_cast<char *>(residual) + e * ses;
    p.stream.first += e;
    if (es == kE4m3Granule) {  // granules e .. e + len / es of the request's elements; the last one may be short
        const size_t e0 = e * kE4m3Elems, e1 = e0 + len / es * kE4m3Elems;
        p.elems = e0 >= elems ? 0 : (e1 < elems ? e1 : elems) - e0;
    }
    return p;
}

std::vector<SubPlan> cut_plan(const std::vector<PlanSeg> &segs, size_t cap, size_t es, size_t ses) {
    std::vector<SubPlan> subs(1);
    for (size_t i = 0; i < segs.size(); ++i) {
        size_t off = 0;
        do {
            if (subs.back().flat >= cap) subs.emplace_back();
            SubPlan &cur = subs.back();
            const size_t room = cap - cur.flat, left = segs[i].bytes - off;
            const size_t len = left <= room ? left : room;
            cur.segs.push_back(segs[i].piece(off, len, es, ses));
            cur.seg.push_back(i);
            cur.elem.push_back(es == kE4m3Granule ? off / es * kE4m3Elems : off / es);
            cur.flat += (len + 255) & ~size_t(255);
            off += len;
        } while (off < segs[i].bytes);
    }
    return subs;
}

}  // namespace ddl
