// pipeline_core.h — the sample pipeline's threads and queues, host-compilable (no HIP): `n_workers` sketch threads take the
// submitted jobs in submission order, ONE profile thread probes the oldest sketched job together with the batch pipeline_plan.h
// grants it, and `next` hands the jobs back in submission order.  What the threads DO is the `Work` the owner supplies
// (pipeline.hip: the GPU work; tests/pipeline_core_main.cpp: a fake that sleeps and records):
//
//   void enter(int worker)                    a thread starts: worker w, or -1 for the profile thread
//   bool sketch(Job&, int worker)             -> whether the job is good; may set job.owner = worker (see dispose)
//   bool profile(const std::vector<Job*>& batch, Block&)      one probe over the batch's good jobs -> whether it succeeded
//   void dispose(Job&)                        the job's device objects go; runs on worker `job.owner`'s thread when there is
//                                             one (a worker's session must die on the thread that owns its context), else on
//                                             the thread that called next / the destructor
//
// Every decision goes through pipeline_plan.h; refusals come back as an enum, the owner words them.
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "pipeline_plan.h"

namespace sylph {
namespace pipeline_core {

using pipeline_plan::JobState;

enum class Refusal { None, Stopping, Full, NothingOutstanding, WouldBlock };

template <class Block>
struct Shared {      // one result block, shared by the jobs of one probe batch
    Block data;
    uint32_t users = 0;
};

template <class Block>
struct JobBase {     // what the core keeps of a job; the owner's Job derives from it
    uint64_t seq = 0;
    JobState state = JobState::Queued;
    bool sketch_ok = false, probe_ok = false;
    int owner = -1;              // the worker on whose thread the job is disposed of (-1: the caller's)
    uint32_t batch_size = 0;     // of the probe batch the job was part of
    int slot = -1;               // its slot in `block` (-1: none — it failed, or the probe did)
    Shared<Block>* block = nullptr;
};

template <class Job, class Block, class Work>
class Core {
public:
    std::atomic<uint32_t> min_batch{pipeline_plan::DEFAULT_MIN_BATCH}, batch_wait_us{pipeline_plan::DEFAULT_BATCH_WAIT_US};

    Core(Work& work, uint32_t n_workers, uint32_t depth, uint32_t max_batch, bool sharded)
        : work_(work), depth_(depth), max_batch_(max_batch), sharded_(sharded), trash_(n_workers) {
        for (uint32_t w = 0; w < n_workers; w++) workers_.emplace_back([this, w] { worker_main((int)w); });
        profiler_ = std::thread([this] { profile_main(); });
    }
    // outstanding jobs are finished first (their inputs are the caller's memory: nothing may still read them afterwards); sharded:
    // they go in a last, partial batch, as after flush (every rank ends its pipeline with the same number of jobs outstanding)
    ~Core() {
        flush();
        Job* j = nullptr;
        while (next(&j, nullptr) == Refusal::None) {}
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_work_.notify_all();
        cv_sketched_.notify_all();
        for (auto& t : workers_) t.join();
        profiler_.join();
    }
    Core(const Core&) = delete;
    Core& operator=(const Core&) = delete;

    Refusal submit(std::unique_ptr<Job>& j) {     // takes the job unless it refuses
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (stop_) return Refusal::Stopping;
            if (order_.size() >= depth_) return Refusal::Full;
            j->seq = next_seq_++;
            order_.push_back(j.get());
            to_sketch_.push_back(j.release());
        }
        cv_work_.notify_one();
        return Refusal::None;
    }
    void flush() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (next_seq_ > first_unprofiled_ && (flush_.empty() || flush_.back() < next_seq_)) flush_.push_back(next_seq_);
        }
        cv_sketched_.notify_all();
    }
    // Releases the job the previous call returned, then takes the front job once it is profiled: *out stays the caller's to read
    // until the next call.  WouldBlock: *unprofiled = the jobs not profiled yet.
    Refusal next(Job** out, uint64_t* unprofiled) {
        std::unique_lock<std::mutex> lk(mu_);
        if (Job* r = returned_) {
            returned_ = nullptr;
            if (r->block) r->block->users--;
            if (r->owner >= 0) { trash_[(size_t)r->owner].push_back(r); cv_work_.notify_all(); }
            else { lk.unlock(); dispose(r); lk.lock(); }
        }
        if (order_.empty()) return Refusal::NothingOutstanding;
        Job* j = order_.front();
        const uint64_t left = next_seq_ - first_unprofiled_;
        if (pipeline_plan::next_would_block(sharded_, j->state == JobState::Profiled, !flush_.empty() && flush_.back() > j->seq, left, max_batch_)) {
            if (unprofiled) *unprofiled = left;
            return Refusal::WouldBlock;
        }
        cv_done_.wait(lk, [&] { return j->state == JobState::Profiled; });
        order_.pop_front();
        *out = returned_ = j;
        return Refusal::None;
    }
    uint32_t outstanding() {
        std::lock_guard<std::mutex> lk(mu_);
        return (uint32_t)order_.size();
    }

private:
    void dispose(Job* j) { work_.dispose(*j); delete j; }
    void worker_main(int w) {
        work_.enter(w);
        for (;;) {
            Job* j = nullptr;
            std::vector<Job*> dead;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_work_.wait(lk, [&] { return stop_ || !to_sketch_.empty() || !trash_[(size_t)w].empty(); });
                dead.swap(trash_[(size_t)w]);
                if (!to_sketch_.empty()) {
                    j = to_sketch_.front();
                    to_sketch_.pop_front();
                    j->state = JobState::Sketching;
                } else if (stop_ && dead.empty()) return;      // (nothing lands in the trash after stop: it is set behind the last next)
            }
            for (Job* d : dead) dispose(d);
            if (!j) continue;
            const bool ok = work_.sketch(*j, w);
            {
                std::lock_guard<std::mutex> lk(mu_);
                j->sketch_ok = ok;
                j->state = JobState::Sketched;
            }
            cv_sketched_.notify_all();
        }
    }
    // mu held: the batch the plan grants now, from the first job that is not profiled (order_ holds consecutive sequence numbers)
    pipeline_plan::Batch decide() const {
        const size_t at = order_.empty() ? 0 : (size_t)(first_unprofiled_ - order_.front()->seq);
        return pipeline_plan::next_batch([&](size_t i) { return order_[at + i]->state; }, order_.size() - at, max_batch_, sharded_, first_unprofiled_,
                                         flush_.data(), flush_.size());
    }
    Shared<Block>* take_block() {                 // mu held
        for (auto& b : blocks_)
            if (b->users == 0) return b.get();
        blocks_.emplace_back(new Shared<Block>());
        return blocks_.back().get();
    }
    void profile_main() {
        work_.enter(-1);
        std::vector<Job*> batch;
        for (;;) {
            Shared<Block>* blk = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_sketched_.wait(lk, [&] { return stop_ || decide().go; });
                pipeline_plan::Batch b = decide();
                if (!b.go) return;                 // stop, and nothing left to do (the destructor drains the outstanding jobs first)
                auto coming = [&] {
                    size_t n = 0;
                    for (Job* j : order_) n += j->state == JobState::Queued || j->state == JobState::Sketching;
                    return n;
                };
                auto fuller = [&] { return !stop_ && pipeline_plan::wait_for_fuller(b.n, min_batch.load(), max_batch_, batch_wait_us.load(), sharded_, coming); };
                if (fuller()) {
                    const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(batch_wait_us.load());
                    while (fuller() && cv_sketched_.wait_until(lk, deadline) != std::cv_status::timeout) b = decide();
                    b = decide();
                }
                const size_t at = (size_t)(first_unprofiled_ - order_.front()->seq);
                batch.assign(order_.begin() + (std::ptrdiff_t)at, order_.begin() + (std::ptrdiff_t)(at + b.n));
                blk = take_block();
                blk->users = b.n;
            }
            const bool ok = work_.profile(batch, blk->data);
            {
                std::lock_guard<std::mutex> lk(mu_);
                pipeline_plan::Slots slots{ok};
                for (Job* j : batch) {
                    j->probe_ok = ok;
                    j->batch_size = (uint32_t)batch.size();
                    j->block = blk;
                    j->slot = slots.take(j->sketch_ok);
                    j->state = JobState::Profiled;
                }
                first_unprofiled_ = batch.back()->seq + 1;
                while (!flush_.empty() && pipeline_plan::flush_point_spent(flush_.front(), first_unprofiled_)) flush_.erase(flush_.begin());
            }
            cv_done_.notify_all();
        }
    }

    Work& work_;
    const uint32_t depth_, max_batch_;
    const bool sharded_;
    std::mutex mu_;
    std::condition_variable cv_work_, cv_sketched_, cv_done_;
    std::deque<Job*> to_sketch_;                  // submitted, not yet taken by a worker
    std::deque<Job*> order_;                      // every outstanding job in submission order (front = next to be returned)
    std::vector<std::vector<Job*>> trash_;        // per worker: returned jobs to dispose of on that worker's thread
    std::vector<std::unique_ptr<Shared<Block>>> blocks_;
    Job* returned_ = nullptr;                     // the job whose views the caller holds (released by the next call)
    uint64_t next_seq_ = 0, first_unprofiled_ = 0;
    std::vector<uint64_t> flush_;                 // pending flush points, oldest first, each beyond first_unprofiled_
    bool stop_ = false;
    std::vector<std::thread> workers_;
    std::thread profiler_;
};

}  // namespace pipeline_core
}  // namespace sylph
