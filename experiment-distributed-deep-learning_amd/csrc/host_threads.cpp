// host_threads.cpp — see host_threads.h.
#include "host_threads.h"

#include <pthread.h>
#include <sched.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace ddl {

std::vector<int> numa_local_cpus(int dom, int bus, int dev) {
    char path[128];
    std::snprintf(path, sizeof path, "/sys/bus/pci/devices/%04x:%02x:%02x.0/numa_node", dom, bus, dev);
    FILE *f = std::fopen(path, "r");
    int node = -1;
    if (f) {
        if (std::fscanf(f, "%d", &node) != 1) node = -1;
        std::fclose(f);
    }
    if (node < 0) return {};
    std::snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    f = std::fopen(path, "r");
    if (!f) return {};
    char buf[4096] = {};
    const size_t got = std::fread(buf, 1, sizeof buf - 1, f);
    std::fclose(f);
    buf[got] = 0;
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return {};
    std::vector<int> cpus;
    for (char *p = buf; *p;) {  // "0-63,128-191"
        char *end = nullptr;
        const long a = std::strtol(p, &end, 10);
        if (end == p) break;
        long b = a;
        if (*end == '-') b = std::strtol(end + 1, &end, 10);
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c)
            if (c >= 0 && CPU_ISSET((int)c, &allowed)) cpus.push_back((int)c);
        p = *end == ',' ? end + 1 : end;
        if (*p == '\n') break;
    }
    if (cpus.empty() || (int)cpus.size() == CPU_COUNT(&allowed)) return {};
    return cpus;
}

void bind_this_thread(const std::vector<int> &cpus) {
    if (cpus.empty()) return;
    cpu_set_t s;
    CPU_ZERO(&s);
    for (int c : cpus) CPU_SET(c, &s);
    (void)pthread_setaffinity_np(pthread_self(), sizeof s, &s);
}

AsyncLane::AsyncLane(std::vector<int> cpus) : cpus_(std::move(cpus)) {
    thread_ = std::thread(&AsyncLane::worker_, this);
}

AsyncLane::~AsyncLane() {
    {
        std::lock_guard<std::mutex> g(mu_);
        stop_ = true;
    }
    cv_.notify_all();
    if (thread_.joinable()) thread_.join();
}

uint64_t AsyncLane::submit(std::function<void()> job) {
    uint64_t seq;
    {
        std::lock_guard<std::mutex> g(mu_);
        q_.push_back(std::move(job));
        seq = ++submitted_;
    }
    cv_.notify_one();
    return seq;
}

void AsyncLane::wait(uint64_t seq) {
    std::unique_lock<std::mutex> g(mu_);
    done_cv_.wait(g, [&] { return done_ >= seq; });
    if (failed_) {
        failed_ = false;
        throw err_;
    }
}

void AsyncLane::drain() noexcept {
    std::unique_lock<std::mutex> g(mu_);
    done_cv_.wait(g, [&] { return done_ >= submitted_; });
    failed_ = false;
}

void AsyncLane::worker_() {
    bind_this_thread(cpus_);
    for (;;) {
        std::function<void()> job;
        {
            std::unique_lock<std::mutex> g(mu_);
            cv_.wait(g, [&] { return stop_ || !q_.empty(); });
            if (q_.empty()) return;  // stop_, nothing left
            job = std::move(q_.front());
            q_.pop_front();
        }
        bool bad = false;
        Error e{0, ""};
        try {
            job();
        } catch (const Error &x) {
            bad = true;
            e = x;
        } catch (const std::exception &x) {
            bad = true;
            e = Error{DDL_STATUS_ERROR_UNKNOWN, x.what()};
        }
        {
            std::lock_guard<std::mutex> g(mu_);
            if (bad && !failed_) {
                failed_ = true;
                err_ = e;
            }
            ++done_;
        }
        done_cv_.notify_all();
    }
}

CopyPool::CopyPool(int threads, std::vector<int> cpus) : cpus_(std::move(cpus)) {
    for (int i = 0; i < threads; ++i) threads_.emplace_back(&CopyPool::worker_, this);
}

CopyPool::~CopyPool() {
    {
        std::lock_guard<std::mutex> g(mu_);
        stop_ = true;
    }
    cv_.notify_all();
    for (std::thread &t : threads_) t.join();
}

void CopyPool::worker_() {
    bind_this_thread(cpus_);
    for (;;) {
        std::function<void()> task;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [this] { return stop_ || !queue_.empty(); });
            if (stop_ && queue_.empty()) return;
            task = std::move(queue_.back());
            queue_.pop_back();
        }
        task();
        {
            std::lock_guard<std::mutex> g(mu_);
            --outstanding_;
        }
        done_cv_.notify_all();
    }
}

void CopyPool::submit_and_wait_(std::vector<std::function<void()>> &tasks) {
    if (tasks.empty()) return;
    {
        std::lock_guard<std::mutex> g(mu_);
        for (size_t i = 1; i < tasks.size(); ++i) queue_.push_back(std::move(tasks[i]));
        outstanding_ += tasks.size() - 1;
    }
    cv_.notify_all();
    tasks[0]();
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [this] { return outstanding_ == 0; });
}

void CopyPool::parallel(size_t n, const std::function<void(size_t, size_t)> &fn) {
    const size_t T = std::min(threads_.size() + 1, n);
    if (T <= 1) {
        if (n) fn(0, n);
        return;
    }
    std::vector<std::function<void()>> tasks;
    for (size_t t = 0; t < T; ++t) {
        const size_t lo = n * t / T, hi = n * (t + 1) / T;
        tasks.push_back([&fn, lo, hi] { fn(lo, hi); });
    }
    submit_and_wait_(tasks);
}

void CopyPool::run(const std::vector<Piece> &pieces) {
    size_t total = 0;
    for (const Piece &p : pieces) total += p.bytes;
    const size_t T = threads_.size() + 1;
    if (threads_.empty() || total < (2u << 20)) {
        for (const Piece &p : pieces) std::memcpy(p.dst, p.src, p.bytes);
        return;
    }
    // T shares of about total / T bytes each, pieces cut where a share ends
    const size_t share = (total + T - 1) / T;
    std::vector<std::vector<Piece>> shares(1);
    size_t room = share;
    for (Piece p : pieces) {
        while (p.bytes) {
            if (room == 0) {
                shares.emplace_back();
                room = share;
            }
            const size_t n = p.bytes < room ? p.bytes : room;
            shares.back().push_back(Piece{p.dst, p.src, n});
            p.dst = static_cast<char *>(p.dst) + n;
            p.src = static_cast<const char *>(p.src) + n;
            p.bytes -= n;
            room -= n;
        }
    }
    std::vector<std::function<void()>> tasks;
    for (auto &sh : shares)
        tasks.push_back([work = std::move(sh)] {
            for (const Piece &p : work) std::memcpy(p.dst, p.src, p.bytes);
        });
    submit_and_wait_(tasks);
}

}  // namespace ddl
