// A stand-alone program over sylph_amd/host/ordered_ahead.hpp — the very header cmd_contain.cpp hands its samples over with — and
// nothing else: a fake pipeline (a queue of outstanding jobs with a depth, results in submission order) instead of the GPU's, prepare
// functions that sleep a seeded pseudo-random 0-2 ms.  tests/test_ordered_ahead.py builds it with -fsanitize=thread and with
// -fsanitize=address,undefined and runs both.  Per case, over fresh seeds:
//   * jobs are consumed in input order, each once, every turn the one its submit chose;
//   * no prepare begins further ahead of the consumer than the plan's ahead limit, and the pool does run that far ahead;
//   * never more outstanding than the depth;
//   * the driver waits for a job that is not ready only when nothing is outstanding and nothing submitted is unconsumed;
//   * an inline turn runs with the pipeline empty and nothing submitted behind it;
//   * a failed prepare fails the run at its turn, after every job before it; a throwing consumer ends it at once; either way the
//     workers are joined, then the pipeline is drained (what it reads of a job is still there), then every prepared result nobody
//     took is disposed of, once;
//   * worker state lives and dies on its worker's thread; a worker whose factory threw fails the jobs it takes, no others;
//   * the program ends: no thread is left waiting (the test runs it under a time limit).
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <stdexcept>
#include <string>

#include "../sylph_amd/host/ordered_ahead.hpp"

using namespace sylph_host::ordered_ahead;

namespace {

std::atomic<int> g_failures{0};
thread_local std::string g_case;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) {                                                            \
            if (g_failures++ < 20) { fprintf(stderr, "FAIL [%s] %s:%d %s: ", g_case.c_str(), __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
        }                                                                         \
    } while (0)

struct Rng {
    uint64_t s;
    uint64_t next() { s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    void nap(unsigned max_us) { std::this_thread::sleep_for(std::chrono::microseconds(next() % (max_us + 1))); }
};

struct Latch {                                  // (polled: a timed wait on a condition variable is not something every ThreadSanitizer follows)
    std::atomic<bool> is_open{false};
    void open() { is_open = true; }
    bool wait(int seconds) {
        const auto give_up = std::chrono::steady_clock::now() + std::chrono::seconds(seconds);
        while (!is_open && std::chrono::steady_clock::now() < give_up) std::this_thread::sleep_for(std::chrono::microseconds(50));
        return is_open;
    }
};

struct P { long tag = -1; };                    // a prepared result: its job (-1: the empty result of a cancelled job)
using FakePool = Pool<P>;

// The pipeline of the test: only the consumer's thread touches it.  `keep[j]` stands for what the caller keeps alive for a
// submitted job (a mapping the pipeline reads): taking a result, or draining, finds it there.
struct FakePipe {
    size_t depth;
    std::deque<size_t> q;
    size_t max_outstanding = 0;
    std::vector<std::unique_ptr<int>> keep;
    void submit(size_t j) {
        CHECK(q.size() < depth, "job %zu submitted with %zu outstanding, depth %zu", j, q.size(), depth);
        keep[j].reset(new int(1));
        q.push_back(j);
        max_outstanding = std::max(max_outstanding, q.size());
    }
    size_t next() {
        const size_t j = q.front();
        q.pop_front();
        CHECK(keep[j] != nullptr, "the pipeline reads job %zu after what the caller kept for it is gone", j);
        return j;
    }
};

constexpr long NONE = -1;
struct Case {
    std::string name;
    size_t n, workers;
    long blocked = NONE;            // this job's prepare waits for a latch that opens when the job before it has been consumed
    long inline_job = NONE;         // this job takes the inline turn
    long fails = NONE;              // this job's prepare throws
    long consumer_throws = NONE;    // consume throws at this job
    long broken_worker = NONE;      // this worker's factory throws
    bool hold_first = false;        // the consumer holds job 0 until the pool stands at the gate
};
Turn turn_of(const Case& c, size_t j) { return (long)j == c.inline_job ? Turn::Inline : j % 5 == 4 ? Turn::Skip : Turn::Pipeline; }

// what the threads of one run record
struct Run {
    const Case& c;
    uint64_t seed;
    std::mutex mu;                              // everything below
    std::vector<int> prepared, handed, disposed;
    size_t started = 0, active = 0, factories = 0;
    long max_ahead = -1;
    bool drained = false;
    std::atomic<FakePool*> pool{nullptr};
    std::atomic<size_t> worker_no{0};
    Latch latch;

    Run(const Case& cs, uint64_t sd) : c(cs), seed(sd), prepared(cs.n), handed(cs.n), disposed(cs.n) {}

    struct WorkerState {
        std::thread::id home = std::this_thread::get_id();
        Rng rng;
        explicit WorkerState(uint64_t s) : rng{s} {}
        ~WorkerState() { CHECK(std::this_thread::get_id() == home, "a worker's state is destroyed on another thread"); }
    };
    FakePool::Prepare worker() {
        const size_t w = worker_no++;
        g_case = c.name + " seed " + std::to_string(seed) + " worker " + std::to_string(w);
        { std::lock_guard<std::mutex> lk(mu); factories++; }
        if ((long)w == c.broken_worker) throw std::runtime_error("factory");
        auto st = std::make_shared<WorkerState>(seed * 977 + w);
        return [this, st](size_t j) { return prepare(*st, j); };
    }
    P prepare(WorkerState& st, size_t j) {
        CHECK(std::this_thread::get_id() == st.home, "job %zu is prepared on a thread that is not its worker's", j);
        FakePool* p;
        while (!(p = pool.load())) std::this_thread::yield();
        const long ahead = (long)j - (long)p->released();       // (`released` only grows: no more than at the gate)
        {
            std::lock_guard<std::mutex> lk(mu);
            started++;
            active++;
            max_ahead = std::max(max_ahead, ahead);
            CHECK(!drained, "job %zu is prepared after the pipeline was drained", j);
        }
        CHECK(ahead >= 0 && ahead < (long)ahead_limit(c.workers), "job %zu began %ld ahead of the consumer, the limit is %zu", j, ahead, ahead_limit(c.workers));
        if ((long)j == c.blocked) CHECK(latch.wait(20), "job %zu was waited for while jobs before it were not consumed", j);
        st.rng.nap(2000);
        std::lock_guard<std::mutex> lk(mu);
        active--;
        if ((long)j == c.fails) throw std::runtime_error("prepare");
        prepared[j] = 1;
        return P{(long)j};
    }
    void dispose(P& p) {
        std::lock_guard<std::mutex> lk(mu);
        CHECK(active == 0, "a result is disposed of while a worker still prepares");
        if (p.tag >= 0) disposed[(size_t)p.tag]++;
    }
    // what was prepared went to exactly one place
    void check_results(bool through_driver) {
        std::lock_guard<std::mutex> lk(mu);
        CHECK(factories == c.workers && active == 0, "%zu factories ran for %zu workers, %zu prepares still run", factories, c.workers, active);
        for (size_t j = 0; j < c.n; j++) {
            if (prepared[j]) CHECK(handed[j] + disposed[j] == 1, "job %zu: handed over %d times, disposed of %d times", j, handed[j], disposed[j]);
            else CHECK(handed[j] + disposed[j] == 0, "job %zu was never prepared, yet handed over or disposed of", j);
            if (through_driver && disposed[j]) CHECK(drained, "job %zu was disposed of before the pipeline was drained", j);
        }
        CHECK(max_ahead < (long)ahead_limit(c.workers), "the pool ran %ld ahead, the limit is %zu", max_ahead, ahead_limit(c.workers));
    }
};

// the pool and the driver over the fake pipeline
void drive(const Case& c, uint64_t seed) {
    Run run(c, seed);
    FakePipe pipe{pipeline_depth(ahead_limit(c.workers)), {}, 0, {}};
    pipe.keep.resize(c.n);                      // (declared before the pool: goes after it — the driver must not need that)
    size_t n_submitted = 0, n_consumed = 0;
    std::string thrown;
    {
        FakePool pool(c.n, c.workers, [&] { return run.worker(); }, [&](P& p) { run.dispose(p); });
        run.pool.store(&pool);
        CHECK(pool.limit() == ahead_limit(c.workers) && pool.size() == c.n, "the pool's limit or size");
        try {
            sylph_host::ordered_ahead::run(
                pool, pipe.depth, [&] { return pipe.q.size(); },
                [&](size_t j, P&& p) {
                    CHECK(p.tag == (long)j && j == n_submitted, "submit got job %ld as number %zu, after %zu", p.tag, j, n_submitted);
                    n_submitted++;
                    { std::lock_guard<std::mutex> lk(run.mu); run.handed[j]++; }
                    if ((long)j == c.blocked) CHECK(n_consumed == j && pipe.q.empty(), "the driver took a job that was not ready with %zu of %zu consumed, %zu outstanding", n_consumed, j, pipe.q.size());
                    if (c.inline_job != NONE && (long)j > c.inline_job) CHECK((long)n_consumed > c.inline_job, "job %zu was submitted behind an inline job that has not run", j);
                    const Turn t = turn_of(c, j);
                    if (t == Turn::Pipeline) pipe.submit(j);
                    return t;
                },
                [&](size_t j, Turn t) {
                    CHECK(j == n_consumed && t == turn_of(c, j), "consume got job %zu with turn %d, expected job %zu with turn %d", j, (int)t, n_consumed, (int)turn_of(c, j));
                    if (c.hold_first && j == 0) {
                        // with nothing released, exactly the jobs below the limit may begin — and they do
                        const size_t want = std::min(c.n, ahead_limit(c.workers));
                        const auto give_up = std::chrono::steady_clock::now() + std::chrono::seconds(20);
                        for (;;) {
                            { std::lock_guard<std::mutex> lk(run.mu); if (run.started >= want) break; }
                            if (std::chrono::steady_clock::now() > give_up) break;
                            std::this_thread::sleep_for(std::chrono::microseconds(50));
                        }
                        std::this_thread::sleep_for(std::chrono::milliseconds(1));      // (a job beyond the limit would have begun by now)
                        std::lock_guard<std::mutex> lk(run.mu);
                        CHECK(run.started == want && run.max_ahead == (long)want - 1, "%zu jobs began with none released, the plan says %zu", run.started, want);
                    }
                    if (t == Turn::Pipeline) {
                        const size_t got = pipe.next();
                        CHECK(got == j, "the pipeline returned job %zu at the turn of %zu", got, j);
                        pipe.keep[j].reset();
                    } else if (t == Turn::Inline) {
                        CHECK(pipe.q.empty() && n_submitted == j + 1, "an inline job runs with %zu outstanding and %zu submitted behind it", pipe.q.size(), n_submitted - j - 1);
                    }
                    if ((long)j == c.consumer_throws) throw std::runtime_error("consume");
                    n_consumed++;
                    if ((long)j + 1 == c.blocked) run.latch.open();
                },
                [&] {
                    // the workers are joined by now; what is outstanding still finds what the caller keeps for it
                    std::lock_guard<std::mutex> lk(run.mu);
                    CHECK(run.active == 0 && !run.drained, "the pipeline is drained while %zu prepares run, or twice", run.active);
                    while (!pipe.q.empty()) pipe.next();
                    run.drained = true;
                });
        } catch (const std::exception& e) { thrown = e.what(); }
        // the driver's clean-up is done when it returns: before the pool goes
        CHECK(pipe.q.empty(), "%zu jobs are outstanding after the run", pipe.q.size());
        { std::lock_guard<std::mutex> lk(run.mu); CHECK(run.drained, "the run ended without draining the pipeline"); }
        run.check_results(true);
    }
    run.check_results(true);                    // (the pool's destructor disposes of nothing twice)
    CHECK(pipe.max_outstanding <= pipe.depth, "%zu outstanding, depth %zu", pipe.max_outstanding, pipe.depth);
    if (c.fails != NONE) {
        CHECK(thrown == "prepare", "the run threw `%s`", thrown.c_str());
        CHECK((long)n_consumed == c.fails && (long)n_submitted == c.fails, "job %ld failed: %zu consumed, %zu submitted", c.fails, n_consumed, n_submitted);
    } else if (c.consumer_throws != NONE) {
        CHECK(thrown == "consume" && (long)n_consumed == c.consumer_throws, "the run threw `%s` after %zu jobs", thrown.c_str(), n_consumed);
    } else if (c.broken_worker != NONE) {
        // which jobs the broken worker took is a matter of timing: the first of them ends the run, at its turn
        if (thrown.empty()) CHECK(n_consumed == c.n, "%zu of %zu consumed", n_consumed, c.n);
        else CHECK(thrown == "factory" && n_submitted == n_consumed && !run.prepared[n_consumed], "the run threw `%s` at job %zu with %zu submitted", thrown.c_str(), n_consumed, n_submitted);
        if (c.workers == 1) CHECK(thrown == "factory" && n_consumed == 0, "the only worker is broken, yet %zu jobs were consumed", n_consumed);
    } else {
        CHECK(thrown.empty() && n_consumed == c.n && n_submitted == c.n, "the run threw `%s`; %zu of %zu consumed", thrown.c_str(), n_consumed, c.n);
    }
}

// the pool alone: every job is taken in order, waiting
void take_all(const Case& c, uint64_t seed) {
    Run run(c, seed);
    size_t ok = 0, failed = 0;
    {
        FakePool pool(c.n, c.workers, [&] { return run.worker(); }, [&](P& p) { run.dispose(p); });
        run.pool.store(&pool);
        for (size_t j = 0; j < c.n; j++) {
            try {
                const std::optional<P> p = pool.take(j, true);
                CHECK(p && p->tag == (long)j, "job %zu came back as %ld", j, p ? p->tag : -2);
                std::lock_guard<std::mutex> lk(run.mu);
                run.handed[j]++;
                ok++;
            } catch (const std::exception& e) {
                CHECK(!strcmp(e.what(), "factory") && !run.prepared[j], "job %zu threw `%s`", j, e.what());
                failed++;
            }
            pool.release_one();
        }
    }
    run.check_results(false);
    CHECK(ok + failed == c.n, "%zu + %zu of %zu jobs", ok, failed, c.n);
    if (c.broken_worker == NONE) CHECK(failed == 0, "%zu jobs failed", failed);
    if (c.broken_worker != NONE && c.workers == 1) CHECK(ok == 0, "%zu jobs came out of a pool whose only worker is broken", ok);
}

}  // namespace

int main(int argc, char** argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 200;
    std::vector<Case> drive_cases, pool_cases;
    for (size_t n : {0u, 1u, 2u, 7u, 40u})
        for (size_t w : {1u, 3u, 8u}) {
            Case c;
            c.name = "n" + std::to_string(n) + " w" + std::to_string(w);
            c.n = n;
            c.workers = w;
            drive_cases.push_back(c);
            c.name += " held at the gate";
            c.hold_first = true;
            if (n) drive_cases.push_back(c);
        }
    auto add = [&](const char* name, size_t n, size_t w, long Case::*what, long j) {
        Case c;
        c.name = std::string(name) + " w" + std::to_string(w);
        c.n = n;
        c.workers = w;
        c.*what = j;
        drive_cases.push_back(c);
        return c;
    };
    for (size_t w : {1u, 3u, 8u}) {
        add("a job that is late, 5 of 12", 12, w, &Case::blocked, 5);
        add("an inline job, 2 of 7", 7, w, &Case::inline_job, 2);
        add("an inline job first", 3, w, &Case::inline_job, 0);
        add("an inline job last", 7, w, &Case::inline_job, 6);
        add("a failing prepare, 3 of 7", 7, w, &Case::fails, 3);
        add("a failing prepare first", 7, w, &Case::fails, 0);
        add("a throwing consumer, 3 of 7", 7, w, &Case::consumer_throws, 3);
        add("a throwing consumer with everything ahead prepared", 40, w, &Case::consumer_throws, 1);
        pool_cases.push_back(add("a broken worker", 40, w, &Case::broken_worker, w == 1 ? 0 : 1));
        Case plain;
        plain.name = "the pool alone w" + std::to_string(w);
        plain.n = 7;
        plain.workers = w;
        pool_cases.push_back(plain);
    }
    // (case, seed) pairs dealt out to a few caller threads, each the consumer of its runs
    const int n_callers = argc > 2 ? atoi(argv[2]) : 8;
    const size_t n_units = (drive_cases.size() + pool_cases.size()) * (size_t)reps;
    std::atomic<size_t> next_unit{0};
    std::vector<std::thread> callers;
    for (int t = 0; t < n_callers; t++)
        callers.emplace_back([&] {
            for (size_t u; (u = next_unit++) < n_units;) {
                const size_t i = u / (size_t)reps, seed = (u % (size_t)reps) * 131 + i;
                const Case& c = i < drive_cases.size() ? drive_cases[i] : pool_cases[i - drive_cases.size()];
                g_case = c.name + " seed " + std::to_string(seed);
                if (i < drive_cases.size()) drive(c, seed); else take_all(c, seed);
            }
        });
    for (auto& t : callers) t.join();
    if (g_failures) { fprintf(stderr, "%d check(s) failed\n", g_failures.load()); return 1; }
    printf("ordered ahead run ok: %zu cases x %d seeds\n", drive_cases.size() + pool_cases.size(), reps);
    return 0;
}
