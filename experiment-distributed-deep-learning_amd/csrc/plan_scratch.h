// plan_scratch.h — what a pipe of whole-request plans (sign.h, lowrank.h) keeps between runs: the ring of segment
// tables and the grow-and-retire device scratch. Everything is posted on the caller's stream; nothing here frees
// or synchronises the device on a data path (a buffer that grows is retired, common.h retire_device).
#pragma once

#include "common.h"

namespace ddl {

// A plan's segment table: written into pinned staging, uploaded on the stream. Four tables in rotation, each
// rewritten once the event behind its last upload has passed.
class PlanTables {
public:
    PlanTables() = default;
    ~PlanTables();
    PlanTables(const PlanTables &) = delete;
    PlanTables &operator=(const PlanTables &) = delete;
    // pinned staging of `bytes` for the next table
    void *stage(size_t bytes) {
        cur_ = &tab_[next_];
        next_ = (next_ + 1) % kTables;
        bytes_ = bytes;
        Table &tb = *cur_;
        if (!tb.ready) DDL_HIP(hipEventCreateWithFlags(&tb.ready, hipEventDisableTiming));
        else DDL_HIP(hipEventSynchronize(tb.ready));  // its last upload has been consumed
        if (bytes > tb.cap) {
            retire_host(tb.host);
            retire_device(tb.dev);
            tb.host = tb.dev = nullptr;
            tb.cap = bytes + bytes / 2;
            DDL_HIP(hipHostMalloc(&tb.host, tb.cap, hipHostMallocDefault));
            DDL_HIP(hipMalloc(&tb.dev, tb.cap));
        }
        return tb.host;
    }
    // what stage() returned, uploaded on `stream`: the device copy
    const void *upload(hipStream_t stream) {
        DDL_HIP(hipMemcpyAsync(cur_->dev, cur_->host, bytes_, hipMemcpyHostToDevice, stream));
        DDL_HIP(hipEventRecord(cur_->ready, stream));
        return cur_->dev;
    }

private:
    struct Table {
        void *host = nullptr, *dev = nullptr;
        size_t cap = 0;
        hipEvent_t ready = nullptr;
    };
    static constexpr int kTables = 4;
    Table tab_[kTables];
    Table *cur_ = nullptr;
    size_t bytes_ = 0;
    int next_ = 0;
};

inline PlanTables::~PlanTables() {
    for (Table &t : tab_) {
        if (t.ready) (void)hipEventSynchronize(t.ready);
        if (t.ready) (void)hipEventDestroy(t.ready);
        if (t.host) (void)hipHostFree(t.host);
        if (t.dev) (void)hipFree(t.dev);
    }
}

// Device scratch of at least `need` bytes that grows by half again; the old allocation may still be read on the
// device, so it is retired, not freed. The owner frees `buf` when it goes.
inline void *grow_retire(void *&buf, size_t &cap, size_t need) {
    if (need > cap) {
        if (buf) retire_device(buf);
        buf = nullptr;
        cap = 0;
        DDL_HIP(hipMalloc(&buf, need + need / 2));
        cap = need + need / 2;
    }
    return buf;
}

}  // namespace ddl
