// engine.cpp — the GPU engine's background bring-up, and the two background threads of the host side (the reaper behind the
// samples, the writer of finished sketches).
#include <condition_variable>

#include "host_internal.hpp"

namespace sylph_host {

// SYLPH_HIP_FEED_TRACE: "[sylph_hip t+123.4 ms] what" — milliseconds since this library was loaded (just behind the dynamic linker)
static const std::chrono::steady_clock::time_point g_loaded = std::chrono::steady_clock::now();
bool fast_exit() { static const bool f = getenv("SYLPH_HIP_CLEAN_EXIT") == nullptr; return f; }
// Work that nobody waits for (unmapping a sample's files, handing inflated copies back) runs on threads of its own; a command that
// leaves through exit() joins them first (they use function-local statics that exit() destroys), one that leaves through _exit does not.
namespace {
// ONE long-lived reaper thread and a queue (round 6): a thread per task, joined only at the end of the command, left a
// finished-but-unjoined thread (its stack mapping) behind every gzip sample — tens of thousands of samples in one command run into
// vm.max_map_count or the thread limit, and std::thread's constructor then throws inside a destructor.  A task that cannot be queued
// (no memory for the node, no thread) runs inline.
struct Reaper {
    std::mutex mu;
    std::condition_variable cv_work, cv_idle;
    std::vector<std::function<void()>> queue;
    bool running = false, started = false;
    void loop() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv_work.wait(lk, [&] { return !queue.empty(); });
            std::vector<std::function<void()>> todo;
            todo.swap(queue);
            running = true;
            lk.unlock();
            for (auto& f : todo) { try { f(); } catch (...) {} }
            todo.clear();
            lk.lock();
            running = false;
            if (queue.empty()) cv_idle.notify_all();
        }
    }
    void add(std::function<void()> f) {
        try {
            std::unique_lock<std::mutex> lk(mu);
            if (!started) { std::thread([this] { loop(); }).detach(); started = true; }   // (it ends with the process)
            queue.push_back(std::move(f));
            lk.unlock();
            cv_work.notify_one();
        } catch (...) { try { f(); } catch (...) {} }
    }
    void drain() {
        std::unique_lock<std::mutex> lk(mu);
        cv_idle.wait(lk, [&] { return queue.empty() && !running; });
    }
};
Reaper& reaper() { static Reaper* r = new Reaper(); return *r; }
Reaper& writers() { static Reaper* r = new Reaper(); return *r; }
}  // namespace
void background(std::function<void()> f) { reaper().add(std::move(f)); }
void join_background() { reaper().drain(); }
void write_behind(std::function<void()> f) { writers().add(std::move(f)); }
void drain_writers() { writers().drain(); }
void trace_mark(const char* what) {
    static const bool trace = getenv("SYLPH_HIP_FEED_TRACE") != nullptr;
    if (trace) fprintf(stderr, "[sylph_hip t+%.1f ms] %s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - g_loaded).count() * 1e3, what);
}

struct Engine::Gate { std::mutex mu; std::condition_variable cv; bool ready = false; };

Engine::Engine(int dev) : device(dev), gate_(new Gate()) {
    init_ = std::thread([this] {
        auto open_gate = [this] { { std::lock_guard<std::mutex> lk(gate_->mu); gate_->ready = true; } gate_->cv.notify_all(); };
        try {
            trace_mark("engine: bring-up begins");
            hip_check(sylph_ctx_create(device, nullptr, &ctx_), "sylph_ctx_create");
            trace_mark("engine: context created (runtime initialised, stream, pinned page)");
            if (getenv("SYLPH_HIP_NO_WARMUP")) { open_gate(); return; }
            // first use of a kernel loads its code object (~25 ms for the sketch kernels, the filter dedup's included): do it here, with
            // a few dummy pairs at a small c (so that the pairs really carry seeds and every kernel of a finish runs)
            sylph_sketch* sk = nullptr;
            hip_check(sylph_sketch_begin(ctx_, 5, 31, SYLPH_READS_PAIRED, 0, SYLPH_SEED_AVX2_COMPAT, &sk), "sylph_sketch_begin");
            int rc = sylph_sketch_set_option(sk, "dedup_fpr", "0.0001");
            std::vector<uint8_t> b(8 * 150, 'A');
            for (size_t i = 0; i < b.size(); i++) b[i] = "ACGT"[(i * 2654435761u >> 7) & 3];
            uint64_t* k = nullptr; uint32_t* c = nullptr; uint64_t n = 0, dup = 0;
            if (warm_text_route.load() && device_feed_enabled()) {
                // the process's first sample is a gzip one on the device route: its text is indexed and pushed by the route's own kernels
                // (csrc/fastq.hip) — the warm-up pairs go THAT way, as FASTQ text, so that those kernels' first launches (~20 ms of host-side
                // binding between the sample's inflate and its push otherwise) happen here; the seeding / dedup kernels behind them are the same
                std::string fq[2];
                for (int m = 0; m < 2; m++) {
                    fq[m] = std::string(16, '\n');
                    for (int r = 0; r < 4; r++) fq[m] += "@w\n" + std::string((const char*)b.data() + (size_t)(m * 4 + r) * 150, 150) + "\n+\n" + std::string(150, 'I') + "\n";
                    fq[m] += std::string(32, '\n');                                         // (readable 16 bytes either side of the text)
                }
                sylph_fastq *fa = nullptr, *fb = nullptr;
                rc = rc || sylph_fastq_index(ctx_, fq[0].data() + 16, fq[0].size() - 48, SYLPH_MEM_HOST, &fa) ||
                     sylph_fastq_index(ctx_, fq[1].data() + 16, fq[1].size() - 48, SYLPH_MEM_HOST, &fb) ||
                     sylph_sketch_set_option(sk, "borrow_until_finish", "1") || sylph_sketch_push_fastq(sk, fa, fb, 0, 4) ||
                     sylph_sketch_finish(sk, &k, &c, &n, &dup);
                sylph_sketch_destroy(sk);
                sk = nullptr;
                sylph_fastq_destroy(fa); sylph_fastq_destroy(fb);
            } else {
                std::vector<uint64_t> off(9);
                for (size_t i = 0; i < off.size(); i++) off[i] = i * 150;
                rc = rc || sylph_sketch_push(sk, b.data(), off.data(), 8, SYLPH_MEM_HOST) || sylph_sketch_finish(sk, &k, &c, &n, &dup);
            }
            sylph_free(k); sylph_free(c);
            if (sk) sylph_sketch_destroy(sk);
            if (rc) hip_check(rc, "warm-up");
            trace_mark("engine: sketch kernels loaded (warm-up sample done)");
            open_gate();             // sessions may be opened from here on ...
            // ... while the packed double buffers of the indexed feed are page-locked (~27 ms; round 5: BEHIND the gate — the first
            // sample of a process travels from pageable memory it was gathered into during the bring-up: PinnedBatch::gather_packed_early).
            // (Only these: the 256 MB ASCII batch of the sequential reader is page-locked by its first add() — most commands never need it.)
            // (using the device FASTQ route's kernels once from here, on a second context, so that their first launches are not the first
            //  sample's was tried: it takes 100-330 ms beside the sample's own work and doubled the sample's inflate — profiles/r06_gz_e2e_trace_final.txt)
            if (defer_pinned.load()) { trace_mark("engine: page-locked feed buffers left to their first user"); return; }
            batch.prealloc_packed();
            trace_mark("engine: packed double buffers page-locked");
            if (device_feed_enabled()) { text.prepare(ctx_); trace_mark("engine: text uploader's chunks page-locked"); }
        } catch (const Error& e) { init_error_ = e.msg; init_code_ = e.code ? e.code : 1; open_gate(); }
    });
}
bool Engine::ready() const {
    std::lock_guard<std::mutex> lk(gate_->mu);
    return gate_->ready;
}
sylph_ctx* Engine::context() {
    {
        std::unique_lock<std::mutex> lk(gate_->mu);
        gate_->cv.wait(lk, [&] { return gate_->ready; });
    }
    if (init_code_) throw Error{init_code_, init_error_};
    return ctx_;
}
void Engine::wait_pinned() {
    (void)context();
    static std::mutex join_mu;                       // (sample threads share the command's first engine only through run_job: one joiner)
    std::lock_guard<std::mutex> lk(join_mu);
    if (init_.joinable()) init_.join();
    if (init_code_) throw Error{init_code_, init_error_};
}
Engine::~Engine() {
    if (init_.joinable()) init_.join();
    if (ctx_) sylph_ctx_destroy(ctx_);
}

}  // namespace sylph_host
