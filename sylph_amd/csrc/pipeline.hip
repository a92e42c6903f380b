// pipeline.hip — a stream of samples through both stages, overlapped inside the library: the GPU work of the sample pipeline.
//
// The reference runs its samples on the rayon pool: sketch.rs:313,371 sketches files on parallel workers, contain.rs:267-289
// walks sample chunks x genomes on all threads.  On the GPU the same overlap has to come from several HIP streams: the seeding
// kernel is VALU-bound and leaves HBM idle, the dedup/count and profile stages are strings of small memory- or latency-bound
// dispatches — with the samples of several steps in flight the small kernels of one sample run beside the seeding kernel of
// another, and result copies and host-side assembly disappear behind them.  A Rust (or any) host gets it with three calls:
//
//   sylph_pipeline_submit*()   hand over a sample (batches of records, a session the caller has been pushing into, or entries)
//   sylph_pipeline_next()      the oldest outstanding sample's results: table size, containment counts, coverage vectors
//
// Three pieces.  pipeline_plan.h DECIDES (the probe batch, the wait for a fuller one, the refusals, the slots of a result block,
// the router's choice, the defaults) and pipeline_core.h RUNS the threads and queues over it (`n_workers` sketch threads, ONE
// profile thread, results in submission order) — both host-compilable and tested without a GPU.  This file is what the threads
// DO, and the two things behind the one opaque handle:
//   Engine   a core + its work: every worker has a context of its own (stream + memory pool) and sketches on it (begin -> push ->
//            finish_device, one seeding kernel at a time: SeedingTurn); the profile thread owns the database's context and probes
//            a batch of tables per launch (one sample per launch leaves the probe at 22 % of the HBM roofline, eight reach 30 %)
//            into a pinned result block.  With a sharded database (cfg.comm) the batches are the same on every rank — a function
//            of the call sequence alone (pipeline_plan.h) — and the probe is the exchange of shard.hip.
//   Router   one Engine per replica of the database (sylph_pipeline_create_multi); samples come back in submission order
//            whichever GPU had them.
#include <atomic>
#include <memory>

#include "contain_index.h"
#include "pipeline_core.h"
#include "sketch_session.h"
#include "sylsp_table.h"
#include "table_summary.h"

using namespace sylph;
namespace plan = sylph::pipeline_plan;

namespace {

double now_s() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + ts.tv_nsec * 1e-9;
}

struct Block {   // one pinned result block (+ its layout), shared by the samples of one probe batch
    HostBlock mem;
    uint32_t width = 4;
    int status = SYLPH_OK;       // of the probe that filled it
    std::string error;
    std::vector<uint32_t> cand_first;   // with a row filter: the candidates of slot s are cand_first[s] .. cand_first[s + 1] of the block's
};

struct Job : pipeline_core::JobBase<Block> {     // (owner: the worker whose context owns `sk`; adopted sessions and tables: none)
    uint64_t tag = 0;
    std::vector<sylph_read_batch> batches;
    int mem = SYLPH_MEM_DEVICE, enc = SYLPH_ENC_ASCII;
    sylph_sketch* sk = nullptr;      // the caller's session (sylph_pipeline_submit_session), or the one a worker opens
    bool is_entries = false;         // a sample that is sketched already (sylph_pipeline_submit_entries): entries / n_entries in `mem`
    const void* entries = nullptr;
    uint64_t n_entries = 0;
    sylph_table* table = nullptr;    // ... and the table a worker unpacked them into, on its context
    sylph_ctx* table_ctx() const { return table ? table->ctx : sk->ctx; }   // the context the sample's table lives on
    int status = SYLPH_OK;           // of the sketch
    std::string error;
    const uint64_t* dev_k = nullptr;
    const uint32_t* dev_c = nullptr;
    uint64_t n_table = 0, dup_removed = 0;
    std::vector<uint64_t> host_k;    // want_table
    std::vector<uint32_t> host_c;
    table_summary_plan::Summary summary{};   // "table_summary"
    bool has_summary = false;
    double t_submit = 0, t_sketch0 = 0, t_sketch1 = 0, t_profile0 = 0, t_done = 0;
};

// What a caller hands to sylph_pipeline_submit*: one of batches / a session / entries.
struct Sample {
    const char* what;                // the entry point, for messages
    const char* whose;               // "batch's" / "entries'"
    const sylph_read_batch* batches = nullptr;
    uint32_t n_batches = 0;
    sylph_sketch* sk = nullptr;
    const void* entries = nullptr;
    uint64_t n_entries = 0;
    bool is_entries = false;
    int mem = SYLPH_MEM_DEVICE, enc = SYLPH_ENC_ASCII;
    uint64_t tag = 0;
    // the device the sample's memory lives on (-1: host memory, any device will do)
    int device() const {
        if (sk) return sk->ctx->device;
        const void* ptr = is_entries ? entries : n_batches ? (batches[0].bases ? (const void*)batches[0].bases : (const void*)batches[0].rec_off) : nullptr;
        if (mem != SYLPH_MEM_DEVICE || !(is_entries ? n_entries : n_batches)) return -1;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
            (void)hipGetLastError();
            throw ArgError{std::string(what) + ": cannot tell the device of the " + whose + " memory"};
        }
        return at.device;
    }
};

// rc of the first item that fails, for every "the same call on each of them"
template <class Items, class Fn>
int for_each_ok(const Items& items, Fn&& fn) {
    for (auto* it : items) { const int rc = fn(it); if (rc != SYLPH_OK) return rc; }
    return SYLPH_OK;
}
// kernel timers summed over contexts, or over replicas
template <class Items, class Fn>
int sum_stats(const Items& items, Fn&& one, double* total_ms, uint64_t* launches) {
    double ms = 0;
    uint64_t n = 0;
    const int rc = for_each_ok(items, [&](auto* it) {
        double m = 0;
        uint64_t l = 0;
        const int r = one(it, &m, &l);
        ms += m;
        n += l;
        return r;
    });
    if (rc != SYLPH_OK) return rc;
    if (total_ms) *total_ms = ms;
    if (launches) *launches = n;
    return SYLPH_OK;
}

}  // namespace

struct sylph_pipeline {      // the opaque handle: an Engine or a Router
    virtual ~sylph_pipeline() {}
    virtual int submit(const Sample& s) = 0;
    virtual void flush() = 0;
    virtual int next(sylph_pipeline_result* out) = 0;
    virtual uint32_t outstanding() = 0;
    virtual int set_option(const char* key, const char* value) = 0;
    virtual int profile(int enable) = 0;
    virtual int kernel_stats(const char* family, double* total_ms, uint64_t* launches) = 0;
    virtual int replica_of_last() = 0;
    virtual int ascending_of_last() = 0;
    virtual int set_row_filter(const sylph_row_filter* f) = 0;
    virtual int rows_of_last(const sylph_row_summary** rows, uint32_t* n, const uint64_t** row_cov_off, const void** row_covs, uint32_t* cov_width) = 0;
    virtual int summary_of_last(sylph_table_summary_t* out) = 0;
};

namespace {

struct Engine final : sylph_pipeline {
    using Core = pipeline_core::Core<Job, Block, Engine>;
    sylph_db* db;
    sylph_comm* comm;
    const uint32_t n_workers, max_batch, depth;
    const uint32_t c, k;
    const int reads_mode, no_dedup, seed_mode, want_table;
    const double min_number_kmers;
    std::vector<sylph_ctx*> wctx;
    bool db_ref = false;                         // the profile thread works on the database's context
    // sylph_pipeline_set_row_filter: set before the first submit and never again, so the profile thread reads it without a lock
    std::unique_ptr<row_stats_plan::Filter> row_filter;
    std::atomic<bool> submitted{false};
    struct LastRows { const sylph_row_summary* rows = nullptr; uint32_t n = 0; const uint64_t* off = nullptr; const void* covs = nullptr; uint32_t width = 0; };
    LastRows last_rows;                          // of the sample next returned last (the caller's thread only)
    std::atomic<uint32_t> table_summary{0};      // "table_summary" = 1: the profile thread summarises every sample's counts on the device (table_summary.hip)
    table_summary_plan::Summary last_summary{};  // of the sample next returned last (the caller's thread only)
    bool last_has_summary = false;
    std::atomic<int> last_ascending{-1};         // of the sample next returned last: its entries ascended (1) / were sorted (0); -1: not an entries job
    // tuning (sylph_pipeline_set_option): see the option table in include/sylph_hip.h
    std::atomic<uint32_t> serial_outside{0};     // "serialize_outside" = 1: the r01-r04 placement of that wait (A/B; profiles/r05_ab_seed_turn.txt)
    std::atomic<uint32_t> serialize_seeding{1};  // 1 (default, r04: +3 %, profiles/r04_ab_pipeline_sweep.txt): one worker at a time runs its seeding kernel —
                                                 // two VALU-bound seeding kernels side by side only slow each other; the others are in their dedup/count tails
    std::mutex opt_mu;
    std::string dedup_fpr, dedup_capacity;       // "dedup_fpr" / "dedup_capacity": handed to every session the pipeline opens (sylph_sketch_set_option; a10.hip)
    // "min_batch" / "batch_wait_us" live in the core.  r04: 2 (+1.2 %).  Round 6: 1 — with the seeding tail, tables probed one by one are 0.5 %
    // (default flags: 2.4 %) FASTER, and the samples no longer complete in pairs: completion intervals p99 2.0 -> 1.3 ms (profiles/r06_ab_latency.txt)
    // serialize_seeding on the DEVICE: a push with a deferred verdict returns as soon as its kernels are queued, so holding a
    // mutex around it orders nothing on the GPU — the next worker's stream waits for the event the previous worker recorded
    // behind its seeding kernel instead (hosts never block on it)
    std::mutex seed_mu;
    std::vector<hipEvent_t> seed_ev;             // one per worker
    hipEvent_t last_seed_ev = nullptr;           // guarded by seed_mu
    std::unique_ptr<Core> core;                  // last: its threads use everything above

    Engine(sylph_db* db_, const sylph_pipeline_config& cfg)
        : db(db_), comm(cfg.comm), n_workers(plan::workers_or_default(cfg.n_workers)), max_batch(plan::max_batch_or_default(cfg.max_batch)),
          depth(plan::depth_or_default(cfg.depth, n_workers)), c(cfg.c), k(cfg.k), reads_mode(cfg.reads_mode), no_dedup(cfg.no_dedup),
          seed_mode(cfg.seed_mode), want_table(cfg.want_table), min_number_kmers(cfg.min_number_kmers) {}
    void start() {
        for (uint32_t w = 0; w < n_workers; w++) {
            sylph_ctx* cx = nullptr;
            if (sylph_ctx_create(db->ctx->device, nullptr, &cx) != SYLPH_OK) throw ArgError{sylph_last_error()};
            wctx.push_back(cx);
            hipEvent_t ev = nullptr;
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) throw ArgError{"hipEventCreate failed"};
            seed_ev.push_back(ev);
        }
        db->ctx->refs++;
        db_ref = true;
        core.reset(new Core(*this, n_workers, depth, max_batch, comm != nullptr));
    }
    ~Engine() override {
        core.reset();                            // finishes what is outstanding, stops the threads
        for (sylph_ctx* cx : wctx) sylph_ctx_destroy(cx);
        for (hipEvent_t ev : seed_ev) (void)hipEventDestroy(ev);
        if (db_ref) ctx_unref(db->ctx);
    }

    // ---- the core's work ----
    void enter(int w) { (void)hipSetDevice(w < 0 ? db->ctx->device : wctx[(size_t)w]->device); }
    void dispose(Job& j) {
        if (j.sk) sylph_sketch_destroy(j.sk);
        if (j.table) sylph_table_destroy(j.table);   // (takes its context's lock itself)
    }
    // One push's turn at the seeding kernel ("serialize_seeding"): armed before the push, settled behind it.  The library waits and
    // records around the seeding kernel itself (common.h SeedTurn), not around the whole push.
    struct SeedingTurn {
        Engine& e;
        sylph_ctx* cx;
        hipEvent_t mine;
        std::unique_lock<std::mutex> lock;
        const bool on;                           // read ONCE per push: the option may change between the two ends
        SeedingTurn(Engine& e_, int w) : e(e_), cx(e_.wctx[(size_t)w]), mine(e_.seed_ev[(size_t)w]), lock(e_.seed_mu, std::defer_lock), on(e_.serialize_seeding.load() != 0) {
            if (!on) return;
            lock.lock();
            hipEvent_t prev = (e.last_seed_ev && e.last_seed_ev != mine) ? e.last_seed_ev : nullptr;
            if (e.serial_outside.load()) {       // A/B knob: rounds 1-4 waited in front of the whole push and recorded behind it
                if (prev) (void)hipStreamWaitEvent(cx->stream, prev, 0);
            } else {
                cx->turn.gate = prev;
                cx->turn.done = mine;
                cx->turn.recorded = false;
            }
        }
        ~SeedingTurn() {
            if (!on) return;
            // (a push that launched no seeding kernel: nothing to order; one whose kernel did not record: behind the whole push)
            if (cx->turn.recorded || hipEventRecord(mine, cx->stream) == hipSuccess) e.last_seed_ev = mine;
            cx->turn = sylph_ctx::SeedTurn{};
        }
    };
    int sketch_rc(Job& j, int w) {
        sylph_ctx* cx = wctx[(size_t)w];
        if (j.is_entries) {                      // nothing to sketch: the entries become the table on this worker's context
            const int rc = sylph_table_from_entries(cx, j.entries, j.n_entries, j.mem, &j.table);
            return rc != SYLPH_OK ? rc : sylph_table_view(j.table, &j.dev_k, &j.dev_c, &j.n_table, nullptr);
        }
        int rc = SYLPH_OK;
        if (!j.sk) {
            rc = sylph_sketch_begin(cx, c, k, reads_mode, no_dedup, seed_mode, &j.sk);
            j.owner = w;
            // device batches are borrowed until sylph_pipeline_next has returned the sample: the seeding verdict may wait for finish
            if (rc == SYLPH_OK && j.mem == SYLPH_MEM_DEVICE && j.batches.size() == 1) rc = sylph_sketch_set_option(j.sk, "borrow_until_finish", "1");
            std::string fpr, cap;
            { std::lock_guard<std::mutex> lk(opt_mu); fpr = dedup_fpr; cap = dedup_capacity; }
            if (rc == SYLPH_OK && !fpr.empty()) rc = sylph_sketch_set_option(j.sk, "dedup_fpr", fpr.c_str());
            if (rc == SYLPH_OK && !cap.empty()) rc = sylph_sketch_set_option(j.sk, "dedup_capacity", cap.c_str());
            for (size_t i = 0; rc == SYLPH_OK && i < j.batches.size(); i++) {
                const sylph_read_batch& b = j.batches[i];
                SeedingTurn turn(*this, w);
                rc = sylph_sketch_push_enc(j.sk, b.bases, b.rec_off, b.n_records, b.n_bases, j.mem, j.enc);
            }
        }
        return rc != SYLPH_OK ? rc : sylph_sketch_finish_device(j.sk, &j.dev_k, &j.dev_c, &j.n_table, &j.dup_removed);
    }
    bool sketch(Job& j, int w) {
        j.t_sketch0 = now_s();
        j.status = sketch_rc(j, w);
        if (j.status != SYLPH_OK) j.error = sylph_last_error();
        j.t_sketch1 = now_s();
        return j.status == SYLPH_OK;
    }
    // one probe launch over the batch's good samples, into `blk`
    bool profile(const std::vector<Job*>& batch, Block& blk) {
        const double t0 = now_s();
        std::vector<sylph_sample_ref> refs;
        std::vector<Job*> good;
        for (Job* j : batch)
            if (j->sketch_ok) { refs.push_back(sylph_sample_ref{j->dev_k, j->dev_c, j->n_table}); good.push_back(j); }
        int rc = SYLPH_OK;
        blk.width = 4;
        if (!good.empty() || comm) {
            rc = guarded([&] {
                if (comm) contain_batch_sharded_impl(db, comm, refs.data(), (uint32_t)refs.size(), SYLPH_MEM_DEVICE, min_number_kmers, &blk.width, &blk.mem);
                else contain_batch_impl(db, refs.data(), (uint32_t)refs.size(), SYLPH_MEM_DEVICE, min_number_kmers, &blk.width, &blk.mem, nullptr, row_filter.get());
            });
        }
        if (rc == SYLPH_OK && row_filter && blk.mem.cand.on) {
            // The candidates come in ascending block row = slot * n_genomes + genome: where every slot's begin, then `row` becomes the genome
            auto* rows = (sylph_row_summary*)blk.mem.p;
            const uint64_t G = db->n_genomes;
            const uint32_t n = blk.mem.cand.n;
            blk.cand_first.assign(refs.size() + 1, n);
            uint32_t at = 0;
            for (size_t s = 0; s < refs.size(); s++) {
                while (at < n && rows[at].row < s * G) at++;
                blk.cand_first[s] = at;
            }
            for (uint32_t i = 0; i < n; i++) rows[i].row = (uint32_t)(rows[i].row % G);
        }
        if (rc == SYLPH_OK && want_table) {
            rc = guarded([&] {
                for (Job* j : good) {
                    sylph_ctx* cx = j->table_ctx();
                    std::lock_guard<std::mutex> lock(cx->mu);
                    DeviceGuard dg(cx->device);
                    j->host_k.resize(j->n_table);
                    j->host_c.resize(j->n_table);
                    if (j->n_table) {
                        cx->d2h(j->host_k.data(), j->dev_k, j->n_table * 8);
                        cx->d2h(j->host_c.data(), j->dev_c, j->n_table * 4);
                    }
                }
            });
        }
        if (rc == SYLPH_OK && table_summary.load()) {
            // every table where it lies: on the context that sketched or unpacked it (its ladder knobs are that context's)
            rc = guarded([&] {
                for (Job* j : good) {
                    sylph_ctx* cx = j->table_ctx();
                    std::lock_guard<std::mutex> lock(cx->mu);
                    DeviceGuard dg(cx->device);
                    table_summary_device(cx, j->dev_c, j->n_table, j->summary);
                    j->has_summary = true;
                    // a summary that declines brings the counts along (result.counts, as with want_table): the caller walks them
                    if ((j->summary.flags & table_summary_plan::DECLINED) && !want_table) {
                        j->host_c.resize(j->n_table);
                        if (j->n_table) cx->d2h(j->host_c.data(), j->dev_c, j->n_table * 4);
                    }
                }
            });
        }
        blk.status = rc;
        if (rc != SYLPH_OK) blk.error = sylph_last_error();
        const double t1 = now_s();
        for (Job* j : batch) { j->t_profile0 = t0; j->t_done = t1; }
        return rc == SYLPH_OK;
    }

    // ---- the handle ----
    int submit(const Sample& s) override {
        if (s.sk && s.sk->ctx->device != db->ctx->device) { set_error("the session lives on another device than the database"); return SYLPH_ERR_INVALID; }
        std::unique_ptr<Job> j(new Job());
        j->batches.assign(s.batches, s.batches + s.n_batches);
        j->sk = s.sk;
        j->is_entries = s.is_entries; j->entries = s.entries; j->n_entries = s.n_entries;
        j->mem = s.mem; j->enc = s.enc; j->tag = s.tag;
        j->t_submit = now_s();
        submitted.store(true);
        switch (core->submit(j)) {
        case pipeline_core::Refusal::None: return SYLPH_OK;
        case pipeline_core::Refusal::Full:
            set_error("sylph_pipeline_submit: %u samples are outstanding already (depth): call sylph_pipeline_next first", depth);
            return SYLPH_ERR_STATE;
        default: set_error("pipeline is shutting down"); return SYLPH_ERR_INVALID;
        }
    }
    void flush() override { core->flush(); }
    int next(sylph_pipeline_result* out) override {
        Job* j = nullptr;
        uint64_t unprofiled = 0;
        switch (core->next(&j, &unprofiled)) {
        case pipeline_core::Refusal::None: break;
        case pipeline_core::Refusal::WouldBlock:
            // sharded: the profile thread waits for a batch of a fixed size (the probe batches must be the same on every rank); with
            // fewer outstanding and no flush nobody would ever wake this call — refuse instead of hanging a one-thread caller
            set_error("sylph_pipeline_next: %llu sample(s) outstanding, the sharded probe batch needs %u: submit more or call sylph_pipeline_flush",
                      (unsigned long long)unprofiled, max_batch);
            return SYLPH_ERR_STATE;
        default: set_error("sylph_pipeline_next: nothing is outstanding"); return SYLPH_ERR_INVALID;
        }
        const Block& b = j->block->data;
        const bool probe_failed = j->sketch_ok && !j->probe_ok;
        memset(out, 0, sizeof(*out));
        out->tag = j->tag;
        out->status = probe_failed ? b.status : j->status;
        out->error = out->status == SYLPH_OK ? nullptr : (probe_failed ? b.error : j->error).c_str();
        out->n_table = j->n_table;
        out->dup_removed = j->dup_removed;
        last_ascending.store(j->table ? j->table->was_ascending : -1);
        out->dev_kmers = j->dev_k;
        out->dev_counts = j->dev_c;
        if (want_table && out->status == SYLPH_OK) { out->kmers = j->host_k.data(); out->counts = j->host_c.data(); }
        else if (j->has_summary && (j->summary.flags & table_summary_plan::DECLINED) && out->status == SYLPH_OK) out->counts = j->host_c.data();
        out->t_submit = j->t_submit; out->t_sketch_begin = j->t_sketch0; out->t_sketch_end = j->t_sketch1;
        out->t_profile_begin = j->t_profile0; out->t_done = j->t_done;
        out->probe_batch = j->batch_size;
        last_has_summary = j->has_summary && out->status == SYLPH_OK;
        last_summary = j->summary;
        last_rows = LastRows{};
        if (j->slot >= 0 && b.mem.cand.on) {     // a row filter: the candidates only (sylph_pipeline_rows_of_last)
            const char* h = (const char*)b.mem.p;
            const CandidateLayout& c = b.mem.cand;
            const uint64_t* sample_off = (const uint64_t*)(h + c.sample_off);
            const uint32_t lo = b.cand_first[(size_t)j->slot], hi = b.cand_first[(size_t)j->slot + 1];
            out->cov_width = b.width;
            out->n_covs = sample_off[j->slot + 1] - sample_off[j->slot];
            last_rows = LastRows{(const sylph_row_summary*)h + lo, hi - lo, (const uint64_t*)(h + c.off) + lo, h + c.covs, b.width};
        } else if (j->slot >= 0) {
            const char* h = (const char*)b.mem.p;
            const uint64_t G = db->n_genomes, row0 = (uint64_t)j->slot * G;
            out->cov_off = (const uint64_t*)h + row0;                  // G + 1 entries; values index `covs`
            out->contain_count = (const uint32_t*)(h + b.mem.lay.ccount) + row0;
            out->covs = h + b.mem.lay.covs;
            out->cov_width = b.width;
            out->n_covs = out->cov_off[G] - out->cov_off[0];
        }
        return SYLPH_OK;
    }
    uint32_t outstanding() override { return core->outstanding(); }
    int set_option(const char* key, const char* value) override {
        // the pipeline's own knobs; everything else goes to the workers' contexts
        std::atomic<uint32_t>* knob = !strcmp(key, "serialize_seeding") ? &serialize_seeding : !strcmp(key, "serialize_outside") ? &serial_outside
                                    : !strcmp(key, "table_summary") ? &table_summary : !strcmp(key, "min_batch") ? &core->min_batch : !strcmp(key, "batch_wait_us") ? &core->batch_wait_us : nullptr;
        if (knob) { knob->store((uint32_t)strtoul(value, nullptr, 10)); return SYLPH_OK; }
        if (!strcmp(key, "shard_reduce")) return sylph_ctx_set_option(db->ctx, key, value);      // (the database's context only: "alltoall" | "allgather")
        if (!strcmp(key, "dedup_fpr") || !strcmp(key, "dedup_capacity")) {      // for the sessions opened from now on (checked by the session)
            std::lock_guard<std::mutex> lk(opt_mu);
            (key[6] == 'f' ? dedup_fpr : dedup_capacity) = value;
            return SYLPH_OK;
        }
        const int rc = for_each_ok(wctx, [&](sylph_ctx* cx) { return sylph_ctx_set_option(cx, key, value); });
        if (rc != SYLPH_OK || strcmp(key, "profile_only")) return rc;
        return sylph_ctx_set_option(db->ctx, key, value);      // the profile thread's timers live there
    }
    std::vector<sylph_ctx*> contexts() const { std::vector<sylph_ctx*> all(wctx); all.push_back(db->ctx); return all; }
    int profile(int enable) override { return for_each_ok(contexts(), [&](sylph_ctx* cx) { return sylph_ctx_profile(cx, enable); }); }
    int kernel_stats(const char* family, double* total_ms, uint64_t* launches) override {
        return sum_stats(contexts(), [&](sylph_ctx* cx, double* m, uint64_t* l) { return sylph_ctx_kernel_stats(cx, family, m, l); }, total_ms, launches);
    }
    int replica_of_last() override { return 0; }
    int ascending_of_last() override { return last_ascending.load(); }
    int set_row_filter(const sylph_row_filter* f) override {
        return guarded([&] {
            SY_REQUIRE(f, "sylph_pipeline_set_row_filter: null filter");
            SY_REQUIRE(f->struct_size == sizeof(sylph_row_filter), "sylph_pipeline_set_row_filter: filter of %u bytes, this library's has %zu", f->struct_size,
                       sizeof(sylph_row_filter));
            SY_REQUIRE(!comm, "sylph_pipeline_set_row_filter: a sharded pipeline takes no row filter");
            SY_REQUIRE_STATE(!submitted.load(), "sylph_pipeline_set_row_filter: call it before the first submit");
            static_assert(sizeof(row_stats_plan::Filter) == sizeof(sylph_row_filter), "the ABI's filter is the plan's");
            std::unique_ptr<row_stats_plan::Filter> mine(new row_stats_plan::Filter());
            memcpy(mine.get(), f, sizeof(*f));
            row_filter = std::move(mine);
        });
    }
    int rows_of_last(const sylph_row_summary** rows, uint32_t* n, const uint64_t** row_cov_off, const void** row_covs, uint32_t* cov_width) override {
        *rows = last_rows.n ? last_rows.rows : nullptr;
        *n = last_rows.n;
        *row_cov_off = last_rows.off;
        *row_covs = last_rows.n ? last_rows.covs : nullptr;
        if (cov_width) *cov_width = last_rows.width;
        return SYLPH_OK;
    }
    int summary_of_last(sylph_table_summary_t* out) override {
        return guarded([&] {
            SY_REQUIRE_STATE(last_has_summary, "sylph_pipeline_summary_of_last: no summary of the last sample (set the option \"table_summary\" before submitting it)");
            static_assert(sizeof(table_summary_plan::Summary) == sizeof(sylph_table_summary_t), "the ABI's summary is the plan's");
            memcpy(out, &last_summary, sizeof(*out));
        });
    }
};

// A pipeline over several replicas of one database (sylph_pipeline_create_multi: one per GPU of the node) is only a router:
// `children` are engines, one per replica; `route` holds the replica of every outstanding sample in submission order, so
// that next returns the samples in the order they were submitted whichever GPU had them.
struct Router final : sylph_pipeline {
    std::vector<Engine*> children;
    std::mutex mu;                               // orders submissions against each other; guards route and last_replica
    std::vector<uint32_t> route;                 // (short: at most the replicas' depths together)
    uint32_t last_replica = 0;                   // replica of the sample next returned last

    ~Router() override { for (Engine* c : children) delete c; }      // they finish what they have and go
    // a sample goes to a replica on the device its memory is on, or (host memory) to the least busy one
    int submit(const Sample& s) override {
        const int device = s.device();
        std::lock_guard<std::mutex> lk(mu);
        plan::Replica reps[64];
        for (size_t i = 0; i < children.size(); i++) reps[i] = plan::Replica{children[i]->db->ctx->device, children[i]->outstanding(), children[i]->depth};
        const int r = plan::pick_replica(reps, children.size(), device);
        if (r == plan::NO_REPLICA_ON_DEVICE) { set_error("%s: no replica of the database lives on device %d, where the sample's memory is", s.what, device); return SYLPH_ERR_INVALID; }
        if (r == plan::ALL_FULL) {
            set_error("%s: every replica%s has its `depth` samples outstanding: call sylph_pipeline_next first", s.what, device >= 0 ? " on the sample's device" : "");
            return SYLPH_ERR_STATE;
        }
        const int rc = children[(size_t)r]->submit(s);
        if (rc == SYLPH_OK) route.push_back((uint32_t)r);
        return rc;
    }
    void flush() override { for (Engine* c : children) c->flush(); }
    int next(sylph_pipeline_result* out) override {
        uint32_t r;
        {
            std::lock_guard<std::mutex> lk(mu);
            if (route.empty()) { set_error("sylph_pipeline_next: nothing is outstanding"); return SYLPH_ERR_INVALID; }
            r = route.front();
        }
        // (the replica's own pipeline hands its samples back in ITS submission order, which is the order they were routed in)
        const int rc = children[r]->next(out);
        if (rc == SYLPH_OK) { std::lock_guard<std::mutex> lk(mu); route.erase(route.begin()); last_replica = r; }
        return rc;
    }
    uint32_t outstanding() override { std::lock_guard<std::mutex> lk(mu); return (uint32_t)route.size(); }
    int set_option(const char* key, const char* value) override { return for_each_ok(children, [&](Engine* c) { return c->set_option(key, value); }); }
    int profile(int enable) override { return for_each_ok(children, [&](Engine* c) { return c->profile(enable); }); }
    int kernel_stats(const char* family, double* total_ms, uint64_t* launches) override {
        return sum_stats(children, [&](Engine* c, double* m, uint64_t* l) { return c->kernel_stats(family, m, l); }, total_ms, launches);
    }
    int replica_of_last() override { std::lock_guard<std::mutex> lk(mu); return (int)last_replica; }
    int ascending_of_last() override { return children[(size_t)replica_of_last()]->ascending_of_last(); }
    int set_row_filter(const sylph_row_filter* f) override { return for_each_ok(children, [&](Engine* c) { return c->set_row_filter(f); }); }
    int rows_of_last(const sylph_row_summary** rows, uint32_t* n, const uint64_t** row_cov_off, const void** row_covs, uint32_t* cov_width) override {
        return children[(size_t)replica_of_last()]->rows_of_last(rows, n, row_cov_off, row_covs, cov_width);
    }
    int summary_of_last(sylph_table_summary_t* out) override { return children[(size_t)replica_of_last()]->summary_of_last(out); }
};

void require_config(const sylph_pipeline_config* cfg) {
    SY_REQUIRE(cfg->struct_size == sizeof(sylph_pipeline_config), "sylph_pipeline_config.struct_size is %u, this library expects %zu",
               cfg->struct_size, sizeof(sylph_pipeline_config));
}
int submit_sample(sylph_pipeline* p, const Sample& s) {
    int rc = SYLPH_OK;
    const int thrown = guarded([&] { rc = p->submit(s); });
    return thrown != SYLPH_OK ? thrown : rc;
}
int null_argument() { set_error("null argument"); return SYLPH_ERR_INVALID; }

}  // namespace

extern "C" {

int sylph_pipeline_create(sylph_db* db, const sylph_pipeline_config* cfg, sylph_pipeline** out) {
    return guarded([&] {
        SY_REQUIRE(db && cfg && out, "null argument");
        require_config(cfg);
        SY_REQUIRE(cfg->c >= 1 && (cfg->k == 21 || cfg->k == 31), "bad c / k");
        SY_REQUIRE(cfg->reads_mode == SYLPH_READS_SINGLE || cfg->reads_mode == SYLPH_READS_PAIRED, "bad reads_mode %d", cfg->reads_mode);
        SY_REQUIRE(cfg->seed_mode == SYLPH_SEED_SCALAR || cfg->seed_mode == SYLPH_SEED_AVX2_COMPAT, "bad seed_mode %d", cfg->seed_mode);
        SY_REQUIRE(cfg->n_workers <= 16 && cfg->max_batch <= 64 && cfg->depth <= 4096, "n_workers <= 16, max_batch <= 64, depth <= 4096");
        SY_REQUIRE((cfg->comm != nullptr) == (db->world > 1 || !db->bounds.empty()), "a sharded database needs cfg.comm (and only a sharded one takes it)");
        std::unique_ptr<Engine> e(new Engine(db, *cfg));
        SY_REQUIRE(!e->comm || plan::sharded_depth_ok(e->depth, e->max_batch), "sharded: depth (%u) must reach max_batch (%u), the fixed batch of the exchange", e->depth, e->max_batch);
        e->start();
        *out = e.release();
    });
}

// One sample loop over the GPUs of a node, in ONE process (the reference's sample loop uses the whole machine through its rayon
// pool: contain.rs:252-295, sketch.rs:313,371).  dbs[i]: the database's replica on GPU i (sylph_db_replicate: the index copied over
// xGMI, not uploaded N times).  Every replica gets a pipeline of its own (cfg: per replica); a sample goes to the replica on the
// device its memory lives on (device batches, sessions) or to the least busy one (host batches), and comes back in submission order.
int sylph_pipeline_create_multi(sylph_db* const* dbs, uint32_t n_dbs, const sylph_pipeline_config* cfg, sylph_pipeline** out) {
    return guarded([&] {
        SY_REQUIRE(dbs && cfg && out && n_dbs >= 1 && n_dbs <= 64, "null argument, or not 1..64 replicas");
        require_config(cfg);
        SY_REQUIRE(!cfg->comm, "replicas take no communicator (a sharded database runs one pipeline per rank)");
        for (uint32_t i = 0; i < n_dbs; i++) {
            SY_REQUIRE(dbs[i] && dbs[i]->world == 1 && dbs[i]->bounds.empty(), "replica %u is null or a shard", i);
            SY_REQUIRE(dbs[i]->n_genomes == dbs[0]->n_genomes && dbs[i]->n_kmers == dbs[0]->n_kmers, "replica %u is not a copy of replica 0", i);
        }
        std::unique_ptr<Router> r(new Router());
        for (uint32_t i = 0; i < n_dbs; i++) {
            sylph_pipeline* c = nullptr;
            if (sylph_pipeline_create(dbs[i], cfg, &c) != SYLPH_OK) throw ArgError{sylph_last_error()};
            r->children.push_back(static_cast<Engine*>(c));
        }
        *out = r.release();
    });
}

int sylph_pipeline_replica_of_last(sylph_pipeline* p) { return p ? p->replica_of_last() : -1; }
int sylph_pipeline_ascending_of_last(sylph_pipeline* p) { return p ? p->ascending_of_last() : -1; }
int sylph_pipeline_set_row_filter(sylph_pipeline* p, const sylph_row_filter* filter) { return p ? p->set_row_filter(filter) : null_argument(); }
int sylph_pipeline_rows_of_last(sylph_pipeline* p, const sylph_row_summary** rows, uint32_t* n, const uint64_t** row_cov_off, const void** row_covs,
                                uint32_t* cov_width) {
    return p && rows && n && row_cov_off && row_covs ? p->rows_of_last(rows, n, row_cov_off, row_covs, cov_width) : null_argument();
}

int sylph_pipeline_summary_of_last(sylph_pipeline* p, sylph_table_summary_t* out) { return p && out ? p->summary_of_last(out) : null_argument(); }

int sylph_pipeline_submit(sylph_pipeline* p, const sylph_read_batch* batches, uint32_t n_batches, int mem, int enc, uint64_t tag) {
    if (!p || (n_batches && !batches)) return null_argument();
    Sample s{"sylph_pipeline_submit", "batch's"};
    s.batches = batches; s.n_batches = n_batches; s.mem = mem; s.enc = enc; s.tag = tag;
    return submit_sample(p, s);
}

int sylph_pipeline_submit_session(sylph_pipeline* p, sylph_sketch* sk, uint64_t tag) {
    if (!p || !sk) return null_argument();
    Sample s{"sylph_pipeline_submit_session", "session's"};
    s.sk = sk; s.tag = tag;
    return submit_sample(p, s);
}

int sylph_pipeline_submit_entries(sylph_pipeline* p, const void* entries, uint64_t n_entries, int mem, uint64_t tag) {
    if (!p || (n_entries && !entries)) return null_argument();
    Sample s{"sylph_pipeline_submit_entries", "entries'"};
    s.is_entries = true; s.entries = entries; s.n_entries = n_entries; s.mem = mem; s.tag = tag;
    return submit_sample(p, s);
}

int sylph_pipeline_flush(sylph_pipeline* p) {
    if (!p) return null_argument();
    p->flush();
    return SYLPH_OK;
}

int sylph_pipeline_next(sylph_pipeline* p, sylph_pipeline_result* out) { return p && out ? p->next(out) : null_argument(); }
uint32_t sylph_pipeline_outstanding(sylph_pipeline* p) { return p ? p->outstanding() : 0; }
int sylph_pipeline_set_option(sylph_pipeline* p, const char* key, const char* value) { return p && key && value ? p->set_option(key, value) : null_argument(); }
int sylph_pipeline_profile(sylph_pipeline* p, int enable) { return p ? p->profile(enable) : null_argument(); }
int sylph_pipeline_kernel_stats(sylph_pipeline* p, const char* family, double* total_ms, uint64_t* launches) {
    return p && family ? p->kernel_stats(family, total_ms, launches) : null_argument();
}
void sylph_pipeline_destroy(sylph_pipeline* p) { delete p; }

}  // extern "C"
