// A stand-alone program over sylph_amd/csrc/pipeline_core.h — the very header pipeline.hip includes — with a fake work interface
// instead of the GPU: `sketch` sleeps a pseudo-random 0-200 us, `profile` records its batch.  tests/test_pipeline_plan.py builds
// it with -fsanitize=thread and with -fsanitize=address,undefined and runs both.  Two cores play two ranks: the same call script,
// different sleep seeds, and a caller that dawdles differently between its calls.  Per script, 200 times with fresh seeds:
//   * results come back in submission order, refusals exactly where the script expects them;
//   * a sharded script's batches are the expected ones on both ranks (so: a function of the call sequence alone);
//   * every job is disposed of exactly once, on its owner's worker thread when it has one, else on the caller's;
//   * no result block is filled again while the caller still holds a job that points into it; slots are the plan's;
//   * the program ends: no thread is left waiting (the test runs it under a time limit).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

#include "../sylph_amd/csrc/pipeline_core.h"

using namespace sylph::pipeline_core;

namespace {

std::atomic<int> g_failures{0};
thread_local std::string g_script;       // (every script runs on a thread of its own, which is its pipelines' caller)
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) {                                                            \
            if (g_failures++ < 20) { fprintf(stderr, "FAIL [%s] %s:%d %s: ", g_script.c_str(), __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
        }                                                                         \
    } while (0)

struct Rng {
    uint64_t s;
    uint64_t next() { s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    void nap(unsigned max_us) { std::this_thread::sleep_for(std::chrono::microseconds(next() % (max_us + 1))); }
};

struct FakeBlock { int64_t batch = -1; };       // which probe filled it last
struct FakeJob : JobBase<FakeBlock> {
    uint64_t tag = 0;
    bool fail = false, adopted = false;
    int64_t batch = -1;                         // the probe this job was part of
};

struct Fake {
    std::mutex mu;                              // the fake's own records (workers and the profile thread write them)
    std::vector<Rng> rng;                       // one per worker
    std::vector<std::thread::id> worker_thread;
    std::thread::id caller = std::this_thread::get_id();
    std::vector<std::vector<uint64_t>> batches; // tags per probe, in probe order
    std::map<uint64_t, int> disposed;           // tag -> times
    std::map<uint64_t, bool> failed;            // tag -> the sketch failed
    int64_t fail_probe_with_tag = -1;
    std::atomic<const FakeBlock*> held{nullptr};    // the block the caller's current job points into

    Fake(uint64_t seed, uint32_t n_workers) : worker_thread(n_workers) {
        for (uint32_t w = 0; w < n_workers; w++) rng.push_back(Rng{seed * 977 + w});
    }
    void enter(int w) { if (w >= 0) { std::lock_guard<std::mutex> lk(mu); worker_thread[(size_t)w] = std::this_thread::get_id(); } }
    bool sketch(FakeJob& j, int w) {
        rng[(size_t)w].nap(200);
        if (!j.adopted) j.owner = w;
        return !j.fail;
    }
    bool profile(const std::vector<FakeJob*>& batch, FakeBlock& blk) {
        std::lock_guard<std::mutex> lk(mu);
        CHECK(held.load() != &blk, "a block is filled again while the caller holds a job in it");
        CHECK(!batch.empty(), "an empty batch");
        bool ok = true;
        blk.batch = (int64_t)batches.size();
        batches.emplace_back();
        for (FakeJob* j : batch) {
            CHECK(j->state == JobState::Sketched, "a job in a batch is not sketched");
            j->batch = blk.batch;
            batches.back().push_back(j->tag);
            if ((int64_t)j->tag == fail_probe_with_tag) ok = false;
        }
        return ok;
    }
    void dispose(FakeJob& j) {
        std::lock_guard<std::mutex> lk(mu);
        disposed[j.tag]++;
        const std::thread::id want = j.owner >= 0 ? worker_thread[(size_t)j.owner] : caller;
        CHECK(std::this_thread::get_id() == want, "job %llu (owner %d) disposed of on another thread", (unsigned long long)j.tag, j.owner);
    }
};

using FakeCore = Core<FakeJob, FakeBlock, Fake>;

// One step of a call script.  S: submit (arg: 1 = the sketch fails, 2 = adopted: no owner); D: submit, refused at depth;
// F: flush; N: next; B: next, refused because it would block; E: next, refused because nothing is outstanding.
struct Op { char kind; int arg; };

struct Config { uint32_t workers, depth, max_batch; bool sharded; };

struct Rank {
    Fake fake;
    Rng dawdle;
    std::unique_ptr<FakeCore> core;
    uint64_t submitted = 0, returned = 0;
    FakeJob* held = nullptr;
    std::map<uint64_t, int> slot_of;            // of the jobs next returned
    std::map<uint64_t, bool> probe_ok_of;

    Rank(const Config& c, uint64_t seed) : fake(seed, c.workers), dawdle{seed ^ 0xABCDEF}, core(new FakeCore(fake, c.workers, c.depth, c.max_batch, c.sharded)) {}
    void let_go() {                             // what the caller read of `held` must still be what its probe wrote
        if (!held) return;
        CHECK(held->block && held->block->data.batch == held->batch, "the block of a held job was filled again");
        fake.held.store(nullptr);
        held = nullptr;
    }
    void step(const Op& op) {
        if (op.kind == 'F' || dawdle.next() % 4 == 0) dawdle.nap(300);      // (one rank's profile thread runs between two flushes, the other's does not)
        if (op.kind == 'S' || op.kind == 'D') {
            std::unique_ptr<FakeJob> j(new FakeJob());
            j->tag = submitted;
            j->fail = op.arg & 1;
            j->adopted = op.arg & 2;
            const Refusal r = core->submit(j);
            CHECK(r == (op.kind == 'S' ? Refusal::None : Refusal::Full), "submit answered %d", (int)r);
            CHECK((j == nullptr) == (r == Refusal::None), "submit took a job it refused, or kept one it took");
            if (r == Refusal::None) fake.failed[submitted++] = op.arg & 1;
        } else if (op.kind == 'F') {
            core->flush();
        } else {
            let_go();
            FakeJob* j = nullptr;
            uint64_t unprofiled = 0;
            const Refusal r = core->next(&j, &unprofiled);
            const Refusal want = op.kind == 'N' ? Refusal::None : op.kind == 'B' ? Refusal::WouldBlock : Refusal::NothingOutstanding;
            CHECK(r == want, "next answered %d, the script expects %d", (int)r, (int)want);
            if (r == Refusal::WouldBlock) CHECK(unprofiled == submitted - returned, "would-block reports %llu unprofiled", (unsigned long long)unprofiled);
            if (r != Refusal::None) return;
            CHECK(j->tag == returned, "next returned sample %llu, expected %llu", (unsigned long long)j->tag, (unsigned long long)returned);
            CHECK(j->state == JobState::Profiled && j->block && j->sketch_ok == !j->fail, "a returned job is not done");
            returned++;
            held = j;
            fake.held.store(&j->block->data);
            slot_of[j->tag] = j->slot;
            probe_ok_of[j->tag] = j->probe_ok;
            CHECK(j->batch_size == fake_batch_size(j->batch), "batch_size %u", j->batch_size);
        }
    }
    uint32_t fake_batch_size(int64_t b) { std::lock_guard<std::mutex> lk(fake.mu); return (uint32_t)fake.batches[(size_t)b].size(); }
    // ends the pipeline with whatever is outstanding, then checks the whole run
    std::vector<uint32_t> finish(const Config& c) {
        let_go();
        core.reset();
        std::vector<uint32_t> sizes;
        uint64_t tag = 0;
        for (const auto& b : fake.batches) {
            sizes.push_back((uint32_t)b.size());
            CHECK(b.size() <= c.max_batch, "a batch of %zu", b.size());
            const bool probe_ok = std::find(b.begin(), b.end(), (uint64_t)fake.fail_probe_with_tag) == b.end();
            int slot = 0;
            for (uint64_t t : b) {
                CHECK(t == tag, "batches do not hold the samples in submission order");
                tag++;
                const int want = !fake.failed[t] && probe_ok ? slot++ : -1;
                if (slot_of.count(t)) CHECK(slot_of[t] == want && probe_ok_of[t] == probe_ok, "sample %llu got slot %d, the plan gives %d", (unsigned long long)t, slot_of[t], want);
            }
        }
        CHECK(tag == submitted, "%llu of %llu samples were profiled", (unsigned long long)tag, (unsigned long long)submitted);
        for (uint64_t t = 0; t < submitted; t++) CHECK(fake.disposed[t] == 1, "sample %llu disposed of %d times", (unsigned long long)t, fake.disposed[t]);
        CHECK(fake.disposed.size() == submitted, "a job nobody submitted was disposed of");
        return sizes;
    }
};

struct Script {
    std::string name;
    Config cfg;
    std::vector<Op> ops;
    std::vector<uint32_t> batches;              // sharded: the batch sizes every rank must record
    int64_t fail_probe_with_tag = -1;
};

std::string sizes_text(const std::vector<uint32_t>& v) {
    std::string s;
    for (uint32_t x : v) s += (s.empty() ? "" : ",") + std::to_string(x);
    return s;
}

void run(const Script& s, uint64_t seed) {
    Rank a(s.cfg, seed * 2 + 1), b(s.cfg, seed * 2 + 2);
    a.fake.fail_probe_with_tag = b.fake.fail_probe_with_tag = s.fail_probe_with_tag;
    for (const Op& op : s.ops) { a.step(op); b.step(op); }
    const std::vector<uint32_t> sa = a.finish(s.cfg), sb = b.finish(s.cfg);
    if (!s.cfg.sharded) return;
    CHECK(sa == s.batches, "rank 0 formed batches %s, expected %s", sizes_text(sa).c_str(), sizes_text(s.batches).c_str());
    CHECK(sb == s.batches, "rank 1 formed batches %s, expected %s", sizes_text(sb).c_str(), sizes_text(s.batches).c_str());
}

std::vector<Op> repeat(char kind, int n, int arg = 0) { return std::vector<Op>((size_t)n, Op{kind, arg}); }
std::vector<Op> operator+(std::vector<Op> a, const std::vector<Op>& b) { a.insert(a.end(), b.begin(), b.end()); return a; }

}  // namespace

int main(int argc, char** argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 200;
    std::vector<Script> scripts;
    // unsharded: nine samples through a full queue — fill to the depth, one refused there, take one, submit one, ...
    for (uint32_t workers = 1; workers <= 3; workers++)
        for (uint32_t depth : {1u, 4u, 6u}) {
            std::vector<Op> ops;
            uint32_t submitted = 0, out = 0;
            for (uint32_t done = 0; done < 9; done++) {
                for (; submitted < 9 && out < depth; submitted++, out++) ops.push_back(Op{'S', submitted % 4 == 3 ? 2 : 0});
                if (submitted < 9) ops.push_back(Op{'D', 0});
                ops.push_back(Op{'N', 0});
                out--;
            }
            ops.push_back(Op{'E', 0});
            scripts.push_back(Script{"unsharded w" + std::to_string(workers) + " d" + std::to_string(depth), Config{workers, depth, depth == 6 ? 2u : 8u, false}, ops, {}});
        }
    const Op S{'S', 0}, F{'F', 0}, N{'N', 0};
    scripts.push_back(Script{"sharded: 4, next x3, 1, flush, next x2, 1, destroy", Config{2, 4, 3, true}, repeat('S', 4) + repeat('N', 3) + std::vector<Op>{S, F, N, N, S}, {3, 2, 1}});
    scripts.push_back(Script{"sharded: 2, flush, 2, flush", Config{2, 6, 4, true}, std::vector<Op>{S, S, F, S, S, F, N, N, N, N}, {2, 2}});
    scripts.push_back(Script{"sharded: 3, flush, 2, destroy", Config{3, 8, 8, true}, std::vector<Op>{S, S, S, F, S, S}, {3, 2}});
    scripts.push_back(Script{"sharded: flush, flush, 5, flush, 4, destroy", Config{2, 9, 3, true}, std::vector<Op>{F, F} + repeat('S', 5) + std::vector<Op>{F} + repeat('S', 4), {3, 2, 3, 1}});
    scripts.push_back(Script{"sharded: next with too few and no flush", Config{2, 4, 3, true}, std::vector<Op>{S, S, Op{'B', 0}, S, N, N, N, S, Op{'B', 0}, F, N, Op{'E', 0}}, {3, 1}});
    scripts.push_back(Script{"sharded: next beyond a flush point", Config{2, 6, 4, true}, std::vector<Op>{S, S, F, S, N, N, Op{'B', 0}, F, N}, {2, 1}});
    scripts.push_back(Script{"sharded: submit at depth", Config{1, 3, 3, true}, std::vector<Op>{S, S, S, Op{'D', 0}, N, S, Op{'D', 0}, N, N, Op{'B', 0}}, {3, 1}});
    scripts.push_back(Script{"sharded: a failing sample in the middle of a batch", Config{3, 4, 4, true}, std::vector<Op>{S, Op{'S', 1}, Op{'S', 2}, S, N, N, N, N}, {4}});
    scripts.push_back(Script{"unsharded: failing samples and a failing probe", Config{2, 6, 3, false}, std::vector<Op>{S, Op{'S', 1}, S, Op{'S', 3}, S, S, N, N, N, N, N, N}, {}, 4});
    scripts.push_back(Script{"sharded: a failing probe", Config{2, 6, 3, true}, std::vector<Op>{S, Op{'S', 1}, S, S, S, S, N, N, N, N, N, N}, {3, 3}, 0});
    scripts.push_back(Script{"unsharded: destroy with samples outstanding", Config{3, 6, 2, false}, std::vector<Op>{S, S, Op{'S', 2}, S, N, S, S}, {}});
    scripts.push_back(Script{"unsharded: destroy with nothing taken", Config{1, 4, 8, false}, std::vector<Op>{S, Op{'S', 2}, S}, {}});
    const int n_callers = argc > 2 ? atoi(argv[2]) : 6;      // the scripts are dealt out to a few caller threads
    std::atomic<size_t> next_script{0};
    std::vector<std::thread> callers;
    for (int c = 0; c < n_callers; c++)
        callers.emplace_back([&] {
            for (size_t i; (i = next_script++) < scripts.size();) {
                g_script = scripts[i].name;
                for (int r = 0; r < reps; r++) run(scripts[i], (uint64_t)r * 131 + i);
            }
        });
    for (auto& t : callers) t.join();
    if (g_failures) { fprintf(stderr, "%d check(s) failed\n", g_failures.load()); return 1; }
    printf("pipeline core run ok: %zu scripts x %d seeds x 2 ranks\n", scripts.size(), reps);
    return 0;
}
