// host_threads_check.cpp — stand-alone host check of csrc/host_threads.cpp (CopyPool, AsyncLane,
// numa_local_cpus), built by tests/test_host_threads_cpu.py under ThreadSanitizer and under
// AddressSanitizer + UBSan. No GPU, no HIP library. Exit status 0 and nothing on stderr: all held.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <memory>
#include <stdexcept>
#include <thread>
#include <vector>

#include "host_threads.h"

using namespace ddl;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                           \
        }                                                                           \
    } while (0)

namespace {

// 64 odd piece sizes, 11.6 MB in all (the threaded path of CopyPool::run starts at 2 MiB)
std::vector<size_t> piece_sizes() {
    const size_t cycle[8] = {1, 4095, (1u << 20) + 3, 7, 65537, 3, 4097, 333333};
    std::vector<size_t> s;
    for (int r = 0; r < 8; ++r)
        for (size_t c : cycle) s.push_back(c);
    return s;
}

// the same list cut where its sum reaches `limit` bytes
std::vector<size_t> cut_to(std::vector<size_t> sizes, size_t limit) {
    size_t total = 0;
    for (size_t i = 0; i < sizes.size(); ++i) {
        if (total + sizes[i] >= limit) {
            sizes[i] = limit - total;
            sizes.resize(sizes[i] ? i + 1 : i);
            break;
        }
        total += sizes[i];
    }
    return sizes;
}

// Copies the pieces (3 guard bytes between them on both sides) with `threads` workers and compares
// the whole destination, guards included, with what a plain memcpy of each piece gives.
void check_run(const std::vector<size_t> &sizes, int threads, bool expect_threaded_size) {
    size_t total = 0, span = 0;
    for (size_t s : sizes) {
        total += s;
        span += s + 3;
    }
    CHECK((total >= (4u << 20)) == expect_threaded_size && (total < (2u << 20)) == !expect_threaded_size);
    std::vector<unsigned char> src(span), got(span, 0xEE), want(span, 0xEE);
    uint32_t x = 12345u + (uint32_t)threads;
    for (unsigned char &b : src) b = (unsigned char)((x = x * 1664525u + 1013904223u) >> 24);
    std::vector<CopyPool::Piece> pieces;
    size_t off = 0;
    for (size_t s : sizes) {
        pieces.push_back(CopyPool::Piece{got.data() + off, src.data() + off, s});
        std::memcpy(want.data() + off, src.data() + off, s);
        off += s + 3;
    }
    CopyPool pool(threads);
    CHECK(pool.threads() == threads);
    pool.run(pieces);
    CHECK(std::memcmp(got.data(), want.data(), span) == 0);
}

void check_parallel() {
    CopyPool pool(7);
    for (size_t n : {0, 1, 7, 8, 9}) {
        std::vector<std::atomic<int>> hits(n);
        for (auto &h : hits) h = 0;
        std::atomic<int> calls{0};
        pool.parallel(n, [&](size_t lo, size_t hi) {
            CHECK(lo < hi && hi <= n);
            ++calls;
            for (size_t i = lo; i < hi; ++i) ++hits[i];
        });
        for (auto &h : hits) CHECK(h.load() == 1);  // [0, n) covered exactly once
        CHECK(calls.load() <= 8 && (n == 0) == (calls.load() == 0));
    }
}

void check_lane_order_and_wait() {
    AsyncLane lane;
    std::vector<int> order;  // written by the lane's thread only, read after wait()
    std::vector<uint64_t> seqs;
    for (int i = 0; i < 200; ++i) seqs.push_back(lane.submit([&order, i] { order.push_back(i); }));
    for (int i = 0; i < 200; ++i) CHECK(seqs[i] == (uint64_t)i + 1);
    lane.wait(seqs.back());
    CHECK(order.size() == 200);
    for (int i = 0; i < 200; ++i) CHECK(order[i] == i);
    // wait(seq) returns only after job seq: the job is held at a gate while another thread waits
    std::promise<void> gate;
    std::shared_future<void> open = gate.get_future().share();
    std::atomic<bool> ran{false}, returned{false};
    const uint64_t before = lane.submit([] {});
    const uint64_t held = lane.submit([open, &ran] {
        open.wait();
        ran = true;
    });
    lane.wait(before);  // an earlier job's wait does not need the held one
    std::thread waiter([&] {
        lane.wait(held);
        CHECK(ran.load());
        returned = true;
    });
    for (int i = 0; i < 100; ++i) std::this_thread::yield();
    CHECK(!returned.load());
    gate.set_value();
    waiter.join();
    CHECK(returned.load());
}

void check_lane_errors() {
    AsyncLane lane;
    const uint64_t bad = lane.submit([] { fail(DDL_STATUS_COMM_ERROR, "boom"); });
    const uint64_t good = lane.submit([] {});
    CHECK(good == bad + 1);
    int thrown = 0;
    try {
        lane.wait(good);
    } catch (const Error &e) {
        ++thrown;
        CHECK(e.status == DDL_STATUS_COMM_ERROR && e.msg == "boom");
    }
    CHECK(thrown == 1);
    lane.wait(good);  // rethrown exactly once
    lane.wait(bad);
    // drain() after a throwing job clears the error
    const uint64_t bad2 = lane.submit([] { fail(DDL_STATUS_COMM_ERROR, "boom 2"); });
    lane.drain();
    lane.wait(bad2);
    // a std::exception becomes an Error of unknown status
    const uint64_t bad3 = lane.submit([] { throw std::runtime_error("other"); });
    try {
        lane.wait(bad3);
        CHECK(!"no error from a job that threw");
    } catch (const Error &e) {
        CHECK(e.status == DDL_STATUS_ERROR_UNKNOWN && e.msg == "other");
    }
}

void check_lane_destroyed_with_jobs_queued() {
    std::atomic<int> ran{0};
    std::promise<void> gate;
    std::shared_future<void> open = gate.get_future().share();
    std::unique_ptr<AsyncLane> lane(new AsyncLane());
    lane->submit([open] { open.wait(); });  // holds the queue back
    for (int i = 0; i < 50; ++i) lane->submit([&ran] { ++ran; });
    CHECK(ran.load() == 0);
    std::thread opener([&gate] { gate.set_value(); });
    lane.reset();  // joins its thread once every queued job has run
    CHECK(ran.load() == 50);
    opener.join();
}

}  // namespace

int main() {
    const std::vector<size_t> big = piece_sizes(), small = cut_to(big, (2u << 20) - 1);
    CHECK(big.size() == 64 && small.size() < big.size());
    for (int threads : {0, 1, 7}) {
        check_run(big, threads, true);
        check_run(small, threads, false);
    }
    check_parallel();
    check_lane_order_and_wait();
    check_lane_errors();
    check_lane_destroyed_with_jobs_queued();
    CHECK(numa_local_cpus(0xffff, 0xff, 0x1f).empty());  // no such PCI function
    bind_this_thread({});                                 // empty set: a no-op
    return 0;
}
