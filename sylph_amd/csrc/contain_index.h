// contain_index.h — the k-mer -> genomes "line index" of a database (shard) and the database object, shared by line_index.hip
// (build, upload), contain.hip (probe, reassignment, finish), hits.hip (row assembly) and shard.hip (multi-GPU exchange).  The
// index's arithmetic is index_plan.h.  Internal, not part of the ABI.
#pragma once
#include "common.h"
#include "hits_plan.h"
#include "index_plan.h"
#include "row_stats_plan.h"

namespace sylph {

using index_plan::LINE_SLOTS;
using index_plan::LINE_QUADS;
using index_plan::SLOT_EMPTY;
using index_plan::LONG_RUN_MIN;
using index_plan::DEFAULT_INDEX_LAMBDA;

// What the kernels need to probe an index (POD, passed by value).
//   bucket(km) = (km - base) / div, remainder = (km - base) % div (index_plan::bucket_rem); slots and descriptors: index_plan.h
struct LineView {
    const uint64_t* lines;   // n_buckets x LINE_SLOTS
    const uint64_t* ovf;     // overflow runs, each closed by SLOT_EMPTY
    uint64_t base, div, magic;   // magic = floor(2^64 / div) for div >= 2
    uint64_t n_ovf;          // entries of ovf (the wavefront-wide walk of a long run reads 64 at a time)
    uint32_t n_buckets;
    int gshift;
};

struct LineIndex {
    DevBuf lines, ovf;
    uint64_t base = 0, div = 1, magic = 0, n_postings = 0, n_ovf = 0;
    uint32_t n_buckets = 0;
    int gshift = 2;
    LineIndex() = default;
    explicit LineIndex(sylph_ctx* c) : lines(c), ovf(c) {}
    LineView view() const { return LineView{lines.as<uint64_t>(), ovf.as<uint64_t>(), base, div, magic, n_ovf, n_buckets, gshift}; }
};

// One sample table of a batch: n (k-mer, count) entries; chunk0 = index of its first 256-entry chunk in the batch.
struct SampleRef {
    const uint64_t* k;
    const uint32_t* c;
    uint64_t n;
    uint32_t chunk0, pad;
};

// Up to REFS_INLINE tables travel in the kernel arguments (no host->device copy of the descriptor array, no wait for it).
constexpr uint32_t REFS_INLINE = 8;
struct RefPack { SampleRef r[REFS_INLINE]; };

#ifdef __HIPCC__
// A k-mer's postings in two halves, so that a lane can have the lines of several k-mers in flight before it looks at any of them
// (the probe is latency-bound: random 64 B reads): line_fetch computes the bucket and issues the LINE_QUADS 16-byte loads of its
// line; line_scan calls f(genome id) for every posting of the k-mer (index_plan::scan_slots: the line, then the overflow run of a
// crowded bucket when the postings kept in the line do not already exceed the remainder looked for).  An overflow run of at least
// LONG_RUN_MIN entries is not walked by the lane: its first entry is returned through *long_start (else ~0) with the remainder in
// *long_rem, and the caller's wavefront walks it, 64 entries per long_run_step (for_each_long_run hands the runs over).
struct LineFetch {
    uint4 v[LINE_QUADS];
    uint64_t rem;
    bool live;
};
// the bucket line of k-mer km and its remainder there; false: the index has no bucket for it
__device__ __forceinline__ bool line_locate(const LineView& v, uint64_t km, const uint4*& line, uint64_t& rem) {
    if (km < v.base) return false;
    uint64_t q;
    index_plan::bucket_rem(km - v.base, v.div, v.magic, q, rem);
    if (q >= v.n_buckets) return false;
    line = reinterpret_cast<const uint4*>(v.lines + q * LINE_SLOTS);
    return true;
}
// the slots of a line read as LINE_QUADS 16-byte quads (global_load_dwordx4)
__device__ __forceinline__ void line_unpack(const uint4 (&qd)[LINE_QUADS], uint64_t (&s)[LINE_SLOTS]) {
#pragma unroll
    for (int t = 0; t < LINE_QUADS; t++) { s[2 * t] = ((uint64_t)qd[t].y << 32) | qd[t].x; s[2 * t + 1] = ((uint64_t)qd[t].w << 32) | qd[t].z; }
}
__device__ __forceinline__ LineFetch line_fetch(const LineView& v, uint64_t km, bool wanted) {
    LineFetch f;
    f.live = false;
    f.rem = 0;
#pragma unroll
    for (int t = 0; t < LINE_QUADS; t++) f.v[t] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    const uint4* lp;
    uint64_t rem;
    if (!wanted || !line_locate(v, km, lp, rem)) return f;
#pragma unroll
    for (int t = 0; t < LINE_QUADS; t++) f.v[t] = lp[t];
    f.rem = rem;
    f.live = true;
    return f;
}
template <class F>
__device__ __forceinline__ void line_scan(const LineView& v, const LineFetch& l, F&& f, uint64_t* long_start, uint64_t* long_rem) {
    *long_start = index_plan::NO_LONG_RUN;
    if (!l.live) return;
    uint64_t s[LINE_SLOTS];
    line_unpack(l.v, s);
    index_plan::scan_slots(s, l.rem, v.gshift, v.ovf, f, long_start, long_rem);
}
// The same steps in one go, for a caller with nothing to overlap the line read with (the reassignment pass; written without the
// LineFetch in between: carrying the line through it cost that kernel 7 VGPRs, profiles/index_plan_census.txt).
template <class F>
__device__ __forceinline__ void for_each_posting(const LineView& v, uint64_t km, F&& f, uint64_t* long_start, uint64_t* long_rem) {
    *long_start = index_plan::NO_LONG_RUN;
    const uint4* lp;
    uint64_t rem;
    if (!line_locate(v, km, lp, rem)) return;
    uint4 qd[LINE_QUADS];
#pragma unroll
    for (int t = 0; t < LINE_QUADS; t++) qd[t] = lp[t];
    uint64_t s[LINE_SLOTS];
    line_unpack(qd, s);
    index_plan::scan_slots(s, rem, v.gshift, v.ovf, f, long_start, long_rem);
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t x, int src) {
    return ((uint64_t)(uint32_t)__shfl((int)(x >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)x, src);
}
// The long runs the lanes of a wavefront came back from line_scan with, one after the other: f(lane that owns the run, first entry,
// remainder) with the same arguments in every lane (a uniform loop: the ballot is the same in every lane).
template <class F>
__device__ __forceinline__ void for_each_long_run(uint64_t long_start, uint64_t long_rem, F&& f) {
    for (unsigned long long todo = __ballot(long_start != index_plan::NO_LONG_RUN); todo; todo &= todo - 1) {
        const int src = __ffsll((long long)todo) - 1;
        f(src, shfl_u64(long_start, src), shfl_u64(long_rem, src));
    }
}
// One step of the wavefront's walk of an overflow run: the 64 entries from `base`, one per lane.  match: this lane's entry is a
// posting of the remainder looked for (genome in g); ended: the relevant part of the run ends inside the step.
struct LongRunStep { bool match, ended; uint32_t g; };
__device__ __forceinline__ LongRunStep long_run_step(const LineView& v, uint64_t base, uint64_t rem) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t idx = base + lane;
    const uint64_t y = idx < v.n_ovf ? v.ovf[idx] : SLOT_EMPTY;
    const unsigned long long stop = __ballot(index_plan::run_stops(y, rem, v.gshift));   // the run is sorted by (remainder, genome)
    const uint32_t first_stop = stop ? (uint32_t)__ffsll((long long)stop) - 1 : 64u;
    LongRunStep r;
    r.g = index_plan::slot_genome(y, v.gshift);
    r.ended = stop != 0;
    r.match = lane < first_stop && index_plan::slot_rem(y, v.gshift) == rem;
    return r;
}
// every matching posting of a long overflow run, 64 entries per step, for the whole wavefront (same arguments in every lane):
// f(genome id) is called by the lane that holds the match
template <class F>
__device__ __forceinline__ void long_run_for_each(const LineView& v, uint64_t start, uint64_t rem, F&& f) {
    for (uint64_t base = start;; base += 64) {
        const LongRunStep r = long_run_step(v, base, rem);
        if (r.match) f(r.g);
        if (r.ended) break;
    }
}

// The winner table (contain.rs:410-430), asked per k-mer: the passing genome with the highest first-pass ANI among those that hold
// the k-mer in genome_kmers (the kept index) or in pseudotax_tracked_nonused_kmers (the tracked index), ties to the lowest rank in
// the passing list (the reference replaces only on strictly greater ANI, :417).  rank[g] = position of genome g in the passing list
// or ~0, ani[rank].  Called by every lane of a wavefront together (live: this lane has a k-mer): the line and short overflow runs
// are taken lane by lane; long runs (k-mers shared by hundreds of genomes) are handed to the whole wavefront, one after the other,
// and their outcome is merged into the owning lane before the tracked pass begins.  -> the winner's rank or ~0; n_kept = the
// k-mer's postings in the kept index, passing or not.  TRACKED_NEEDS_KEPT: the tracked index is looked at only for a k-mer some
// genome holds in genome_kmers (the reassignment pass: nothing else can be lost or kept); otherwise for every live k-mer.
__device__ __forceinline__ bool winner_beats(double a, uint32_t r, double ba, uint32_t br) { return a > ba || (a == ba && r < br); }
template <bool TRACKED_NEEDS_KEPT>
__device__ __forceinline__ uint32_t winner_of(const LineView& kept, const LineView& tracked, int have_tracked, uint64_t km, bool live,
                                              const uint32_t* __restrict__ rank, const double* __restrict__ ani, uint32_t& n_kept) {
    const int lane = (int)(threadIdx.x & 63);
    auto consider = [&](uint32_t g, double& ba, uint32_t& br) {
        const uint32_t r = rank[g];
        if (r == 0xFFFFFFFFu) return;
        const double a = ani[r];
        if (winner_beats(a, r, ba, br)) { ba = a; br = r; }
    };
    uint32_t best_rank = 0xFFFFFFFFu;
    double best_ani = -1.0;
    n_kept = 0;
    uint64_t ls = ~0ull, lr = 0;
    if (live) for_each_posting(kept, km, [&](uint32_t g) { n_kept++; consider(g, best_ani, best_rank); }, &ls, &lr);
    for_each_long_run(ls, lr, [&](int src, uint64_t rs, uint64_t rm) {
        uint32_t c_l = 0, r_l = 0xFFFFFFFFu;
        double a_l = -1.0;
        long_run_for_each(kept, rs, rm, [&](uint32_t g) { c_l++; consider(g, a_l, r_l); });
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const uint32_t c_o = (uint32_t)__shfl_xor((int)c_l, d), r_o = (uint32_t)__shfl_xor((int)r_l, d);
            const double a_o = __shfl_xor(a_l, d);
            c_l += c_o;
            if (winner_beats(a_o, r_o, a_l, r_l)) { a_l = a_o; r_l = r_o; }
        }
        if (lane == src) {
            n_kept += c_l;
            if (winner_beats(a_l, r_l, best_ani, best_rank)) { best_ani = a_l; best_rank = r_l; }
        }
    });
    uint64_t lts = ~0ull, ltr = 0;
    if ((TRACKED_NEEDS_KEPT ? n_kept != 0 : live) && have_tracked)
        for_each_posting(tracked, km, [&](uint32_t g) { consider(g, best_ani, best_rank); }, &lts, &ltr);
    for_each_long_run(lts, ltr, [&](int src, uint64_t rs, uint64_t rm) {
        uint32_t r_l = 0xFFFFFFFFu;
        double a_l = -1.0;
        long_run_for_each(tracked, rs, rm, [&](uint32_t g) { consider(g, a_l, r_l); });
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const uint32_t r_o = (uint32_t)__shfl_xor((int)r_l, d);
            const double a_o = __shfl_xor(a_l, d);
            if (winner_beats(a_o, r_o, a_l, r_l)) { a_l = a_o; r_l = r_o; }
        }
        if (lane == src && winner_beats(a_l, r_l, best_ani, best_rank)) { best_ani = a_l; best_rank = r_l; }
    });
    return best_rank;
}
#endif

// Layout of the result block, identical on the device (one buffer, ONE device->host copy) and in pinned host memory:
// [cov_off (R+1) u64 | contain_count R u32 | covs n_hits x width | pad to 8 | kmers_lost G u32 (reassign only, second copy)]
// with R = n_samples x n_genomes rows (row = sample * n_genomes + genome).
struct ResultLayout {
    size_t ccount = 0, covs = 0, lost = 0, end = 0;
    ResultLayout() = default;
    ResultLayout(uint64_t R, uint64_t n_hits, uint32_t width, uint64_t lost_entries)
        : ccount((R + 1) * 8), covs(ccount + R * 4), lost((covs + n_hits * width + 7) & ~(size_t)7), end(lost + lost_entries * 4) {}
};

// Layout of the block a call with a row filter leaves instead (row_stats.hip: only the candidates travel):
// [rows n x sylph_row_summary | pad to 8 | cov_off (n+1) u64 | covs n_vals x width | pad to 8 | sample_off (S+1) u64]
// with sample_off[s] = the full block's cov_off[s * n_genomes]: where the values of sample s began, for its n_covs.
struct CandidateLayout {
    bool on = false;
    uint32_t n = 0;
    uint64_t n_vals = 0;
    size_t off = 0, covs = 0, sample_off = 0, end = 0;
    CandidateLayout() = default;
    CandidateLayout(uint32_t n_, uint64_t n_vals_, uint32_t width, uint64_t n_samples)
        : on(true), n(n_), n_vals(n_vals_), off(((size_t)n_ * sizeof(row_stats_plan::RowSummary) + 7) & ~(size_t)7), covs(off + ((size_t)n_ + 1) * 8),
          sample_off((covs + n_vals_ * width + 7) & ~(size_t)7), end(sample_off + (n_samples + 1) * 8) {}
};

// A block of page-locked host memory that results are copied into (grow-only).
struct HostBlock {
    void* p = nullptr;
    size_t cap = 0;
    ResultLayout lay;            // layout of the result block it holds
    CandidateLayout cand;        // cand.on: it holds the candidates of the block instead
    HostBlock() = default;
    HostBlock(const HostBlock&) = delete;
    HostBlock& operator=(const HostBlock&) = delete;
    ~HostBlock() { if (p) (void)hipHostFree(p); }
    void ensure(size_t need) {
        if (need <= cap) return;
        if (p) SY_HIP(hipHostFree(p));
        p = nullptr;
        cap = 0;
        SY_HIP(hipHostMalloc(&p, need + need / 2, hipHostMallocDefault));
        cap = need + need / 2;
    }
};

}  // namespace sylph

struct sylph_db {
    sylph_ctx* ctx;
    uint64_t n_genomes = 0, n_kmers = 0;     // n_kmers: postings resident on this shard
    uint32_t min_glen = 0;                   // smallest genome (k-mers): the contain.rs:627 test is skipped when nothing can fail it
    sylph::LineIndex kept, tracked;          // genome_kmers; pseudotax_tracked_nonused_kmers (winner table only, types.rs:166)
    sylph::DevBuf glen;
    // k-mer-range sharding (sylph_db_upload_shard): this shard holds k-mers in [bounds[rank], bounds[rank + 1])
    std::vector<uint64_t> bounds;
    uint32_t world = 1, rank = 0;
    // genome sharding (sylph_db_upload_genome_shard): this shard indexes ALL k-mers of the genomes [g_bounds[rank], g_bounds[rank + 1])
    // under their global ids; `bounds` is then {0, ~0, .., ~0} — a table's slice for any shard is the whole table (shard_plan.h)
    bool by_genome = false;
    std::vector<uint64_t> g_bounds;
    uint64_t shard_hit_cap = 1ull << 20;     // hits per rank in the all-gathered block; doubles identically on every rank
    uint64_t x_batches = 0, x_table_bytes = 0, x_hit_bytes = 0;   // exchange totals (sylph_db_exchange_stats): batches, bytes sent to OTHER ranks
    sylph::DevBuf rank_of, ani, lost;        // reassign pass: rank[g] in the passing list (or ~0), ANI per rank, kmers_lost[g]
    // per-query scratch (owned by the db so concurrent dbs on one ctx do not alias)
    sylph::DevBuf q_kmers, q_counts, q_refs, hits, hits_sorted, res, counter;   // res: device copy of the result block
    sylph::DevBuf x_send, x_recv, x_meta;    // shard exchange buffers (shard.hip)
    // row assembly of the hits (hits.hip): row counters (rc_rows of them) + tile totals / snapshot / row lists.  *_dirty = the counters
    // / the probe's two counter words must be cleared before their next use: the record of hits_plan.h, kept by finish_driver
    sylph::DevBuf row_counters, row_meta;
    bool rc_dirty = true, cnt_dirty = true;
    uint32_t rc_rows = 0;
    hipEvent_t ev_cnt = nullptr;             // "the probe's counter words have arrived in pinned host memory"
    const sylph::row_stats_plan::Filter* row_filter = nullptr;   // for the length of one contain_batch_impl call: summarise the rows, copy out the candidates only
    sylph::HostBlock h_block;                // pinned host results of the plain entry points (the pipeline brings its own blocks)
    explicit sylph_db(sylph_ctx* cx)
        : ctx(cx), kept(cx), tracked(cx), glen(cx), rank_of(cx), ani(cx), lost(cx), q_kmers(cx), q_counts(cx), q_refs(cx), hits(cx),
          hits_sorted(cx), res(cx), counter(cx), x_send(cx), x_recv(cx), x_meta(cx), row_counters(cx), row_meta(cx) {}
    ~sylph_db() { if (ev_cnt) (void)hipEventDestroy(ev_cnt); }
};

namespace sylph {
// Probes a batch of device-resident sample tables (refs: host array of n_samples entries with k, c, n filled in) against the
// kept index and leaves unsorted hits ((row << 32) | count, row = sample * n_genomes + genome) in db->hits.
// Returns the number of hits; *max_count = largest count among them.
uint32_t probe_batch(sylph_db* db, std::vector<SampleRef>& refs, double min_number_kmers, uint32_t* max_count);
// hits.hip: hit list in db->hits -> cov_off / contain_count / per-row ascending coverage values in the device result block, five
// launches over a geometry that is taken, sizes from device memory (d_cnt) or from the host (n_imm, max_imm).
void launch_row_assembly(sylph_db* db, const hits_plan::Geometry& g, const uint32_t* d_cnt, uint32_t n_imm, uint32_t max_imm, uint32_t cap,
                         int want_narrow, char* d_res, size_t covs_offset, size_t ccount_offset);
// The hit finish (contain.hip finish_driver, planned by hits_plan.h): what one call of it is to do.
struct ProbeStep {                   // a caller's launch(cap, attempt), by reference: fills db->hits (cap entries), counts into db->counter
    void* self = nullptr;
    void (*call)(void*, uint64_t, int) = nullptr;
    ProbeStep() = default;
    template <class L>
    explicit ProbeStep(L& launch) : self(&launch), call([](void* p, uint64_t cap, int attempt) { (*static_cast<L*>(p))(cap, attempt); }) {}
};
struct HitFinish {
    ProbeStep probe;                 // empty: n_hits hits with a largest count of max_count lie in db->hits already
    uint64_t total = 0;              // the sample k-mers the probe walks (sizes its first hit array)
    hits_plan::Sizes sizes = hits_plan::Sizes::Host;   // Device: assemble behind the probe, sizes from its two words
    uint32_t n_hits = 0, max_count = 0;
    bool finish = true;              // false: the hit list only
    uint64_t n_rows = 0;             // rows of the result block (hits of rows beyond it are dropped) into `dst` (nullptr: the database's own)
    uint32_t* cov_width = nullptr;
    bool with_lost = false;
    HostBlock* dst = nullptr;
};
struct HitSizes { uint32_t n_hits, max_count; };
HitSizes finish_driver(sylph_db* db, const HitFinish& job);
// The bodies of sylph_db_contain_batch / sylph_db_contain_batch_sharded (they take the context lock themselves); the result
// block lands in `dst` (nullptr: the database's own).  Return the number of coverage values.
// `views` (optional): the three result pointers into the block the call filled, taken while the context lock is still held —
// a pipeline's profile thread working on the same database between the lock's release and the caller's own look at
// db->h_block would otherwise hand the caller somebody else's layout.
// `row_filter` (optional, with `dst`): the rows are summarised on the device and only the candidates land in `dst` (dst->cand).
struct ResultViews { const uint64_t* cov_off = nullptr; const uint32_t* contain_count = nullptr; const void* covs = nullptr; };
uint32_t contain_batch_impl(sylph_db* db, const sylph_sample_ref* samples, uint32_t n_samples, int mem, double min_number_kmers,
                            uint32_t* cov_width, HostBlock* dst, ResultViews* views = nullptr, const row_stats_plan::Filter* row_filter = nullptr);
uint32_t contain_batch_sharded_impl(sylph_db* db, sylph_comm* comm, const sylph_sample_ref* samples, uint32_t n_local, int mem,
                                    double min_number_kmers, uint32_t* cov_width, HostBlock* dst, ResultViews* views = nullptr);
inline void fill_views(const HostBlock& b, ResultViews* v) {
    if (!v) return;
    const char* h = (const char*)b.p;
    v->cov_off = (const uint64_t*)h;
    v->contain_count = (const uint32_t*)(h + b.lay.ccount);
    v->covs = h + b.lay.covs;
}
}  // namespace sylph
