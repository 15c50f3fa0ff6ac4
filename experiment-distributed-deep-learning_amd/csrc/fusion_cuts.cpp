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
            cur.elem.push_back(off / es);
            cur.flat += (len + 255) & ~size_t(255);
            off += len;
        } while (off < segs[i].bytes);
    }
    return subs;
}

}  // namespace ddl
