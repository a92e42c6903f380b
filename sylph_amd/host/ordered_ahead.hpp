// ordered_ahead.hpp — the command's half of a sample's hand-over to the pipeline: jobs 0 .. n are PREPARED ahead on a pool of
// threads (a raw sample read and pushed into a session, a sketch file mapped and touched) and SUBMITTED and CONSUMED by the one
// calling thread, in input order.  What is decided stands first, as pure functions (tests/test_ordered_ahead.py reads them through
// tests/ordered_ahead_capi.cpp); the threads, the gate and the clean-up are written once below, over hooks, and
// tests/ordered_ahead_main.cpp drives them over a fake pipeline under ThreadSanitizer and AddressSanitizer + UBSan.
// Nothing of HIP or of the host library in here: a stand-alone program compiles it with g++ alone.
#pragma once

#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <exception>
#include <functional>
#include <future>
#include <mutex>
#include <optional>
#include <thread>
#include <utility>
#include <vector>

namespace sylph_host {
namespace ordered_ahead {

// ---- what is decided ----
// prepared jobs that may wait for their turn (a prepared raw sample holds HBM, a prepared sketch file its touched pages)
inline size_t ahead_limit(size_t n_workers) { return n_workers + 2; }
// ... and the pipeline's depth with it: all of them outstanding, and the one whose result is being reported
inline size_t pipeline_depth(size_t ahead_limit) { return ahead_limit + 1; }
// the gate a worker passes before it prepares job j: `released` jobs have been consumed
inline bool gate_open(size_t j, size_t released, size_t ahead_limit, bool cancelled) { return cancelled || j < released + ahead_limit; }
// the submit loop takes a job that is not ready yet only when waiting is all that is left to do: nothing is outstanding in the
// pipeline and nothing submitted waits to be consumed
inline bool must_wait(size_t outstanding, size_t submitted, size_t done) { return outstanding == 0 && submitted == done; }

// ---- the pool: n_workers threads prepare jobs 0 .. n_jobs in order, each behind the gate ----
// `worker()` is called once on every worker's own thread and returns that worker's prepare function, which owns the worker's state
// (a GPU context of its own, say) and is destroyed on that thread when it ends.  A worker whose factory threw stores that error
// for every job it takes; a prepare function that throws stores its error for that job.  `dispose(p)`: a prepared result nobody
// took, at the pool's end (a job cancelled there yields an empty P, so dispose sees those too).
template <class P>
class Pool {
   public:
    using Prepare = std::function<P(size_t)>;
    Pool(size_t n_jobs, size_t n_workers, std::function<Prepare()> worker, std::function<void(P&)> dispose)
        : limit_(ahead_limit(n_workers)), worker_(std::move(worker)), dispose_(std::move(dispose)), promises_(n_jobs) {
        for (auto& p : promises_) futures_.push_back(p.get_future());
        for (size_t w = 0; w < n_workers; w++) threads_.emplace_back([this] { work(); });
    }
    ~Pool() { stop(); dispose_unconsumed(); }
    Pool(const Pool&) = delete;
    Pool& operator=(const Pool&) = delete;

    size_t size() const { return futures_.size(); }
    size_t limit() const { return limit_; }
    size_t released() { std::lock_guard<std::mutex> lk(mu_); return released_; }
    bool ready(size_t j) { return futures_[j].wait_for(std::chrono::seconds(0)) == std::future_status::ready; }
    // job j's result, once; rethrows what its prepare (or its worker's factory) threw.  !wait: only a job that is ready
    std::optional<P> take(size_t j, bool wait) {
        if (!wait && !ready(j)) return std::nullopt;
        return futures_[j].get();
    }
    void release_one() {
        { std::lock_guard<std::mutex> lk(mu_); released_++; }
        gate_.notify_all();
    }
    // the workers stop taking work and are joined; every job one of them took has its result or its error stored then
    void stop() {
        { std::lock_guard<std::mutex> lk(mu_); cancelled_ = true; }
        gate_.notify_all();
        for (auto& t : threads_) if (t.joinable()) t.join();
    }
    // behind stop(): what was prepared and never taken goes to `dispose`, once
    void dispose_unconsumed() {
        for (size_t j = 0; j < futures_.size(); j++) {
            if (!futures_[j].valid() || !ready(j)) continue;
            try { P p = futures_[j].get(); dispose_(p); } catch (...) {}
        }
    }

   private:
    void work() {
        Prepare prepare;
        std::exception_ptr broken;
        try { prepare = worker_(); } catch (...) { broken = std::current_exception(); }
        for (;;) {
            size_t j;
            bool cancelled;
            {
                std::unique_lock<std::mutex> lk(mu_);
                if (next_job_ >= promises_.size()) return;
                j = next_job_++;
                gate_.wait(lk, [&] { return gate_open(j, released_, limit_, cancelled_); });
                cancelled = cancelled_;
            }
            if (cancelled) { promises_[j].set_value(P{}); continue; }
            if (broken) { promises_[j].set_exception(broken); continue; }
            try { promises_[j].set_value(prepare(j)); } catch (...) { promises_[j].set_exception(std::current_exception()); }
        }
    }
    const size_t limit_;
    const std::function<Prepare()> worker_;
    const std::function<void(P&)> dispose_;
    std::mutex mu_;                      // next_job_, released_, cancelled_
    std::condition_variable gate_;
    size_t next_job_ = 0, released_ = 0;
    bool cancelled_ = false;
    std::vector<std::promise<P>> promises_;
    std::vector<std::future<P>> futures_;
    std::vector<std::thread> threads_;
};

// ---- the ordered driver ----
// What `submit` made of a job.  Pipeline: handed over, `consume` takes its result.  Inline: `consume` does the work on this
// thread — nothing is submitted behind such a job until it has run, so every earlier job has returned and the pipeline is idle
// then.  Skip: `consume` only says so.  Failed is the driver's own: the job's prepare threw.
enum class Turn { Pipeline, Inline, Skip, Failed };

// Every prepared job that is ready is submitted, in input order, while fewer than `depth` are `outstanding()`; then the front
// job is consumed and one more may be prepared.  A job whose prepare failed fails the run WHEN ITS TURN HAS COME: nothing is
// submitted behind it, every job before it is consumed, then its error is rethrown.  An error out of `submit` or `consume` ends
// the run at once.  On every way out, in this order: the pool is stopped (no worker touches anything any more), `drain()` takes
// what is still outstanding in the pipeline (nothing reads a submitted job's memory after that), the prepared results nobody
// took are disposed of.  So whatever the caller keeps alive per submitted job may go once run() has returned or thrown.
template <class P, class Outstanding, class Submit, class Consume, class Drain>
void run(Pool<P>& pool, size_t depth, Outstanding&& outstanding, Submit&& submit, Consume&& consume, Drain&& drain) {
    struct End {
        Pool<P>& pool;
        Drain& drain;
        ~End() {
            pool.stop();
            try { drain(); } catch (...) {}
            pool.dispose_unconsumed();
        }
    } end{pool, drain};
    const size_t n = pool.size();
    std::vector<Turn> turn(n, Turn::Skip);
    std::exception_ptr failure;
    size_t submitted = 0, done = 0, submit_end = n;
    while (done < n) {
        while (submitted < submit_end && (size_t)outstanding() < depth) {
            std::optional<P> p;
            try { p = pool.take(submitted, must_wait((size_t)outstanding(), submitted, done)); }
            catch (...) { failure = std::current_exception(); }
            if (!p && !failure) break;
            const size_t j = submitted++;
            turn[j] = p ? submit(j, std::move(*p)) : Turn::Failed;
            if (turn[j] == Turn::Failed || turn[j] == Turn::Inline) { submit_end = submitted; break; }
        }
        if (done >= submitted) continue;          // (must_wait guarantees progress)
        if (turn[done] == Turn::Failed) std::rethrow_exception(failure);
        consume(done, turn[done]);
        if (turn[done] == Turn::Inline) submit_end = n;
        done++;
        pool.release_one();
    }
}

}  // namespace ordered_ahead
}  // namespace sylph_host
