// contain.hip — sample-vs-database containment on gfx950 (probe half of get_stats, contain.rs:601-656).
//
// The reference walks every genome's k-mers and probes the sample's FxHashMap (contain.rs:632-652): ~1.4e9 random
// probes per sample at GTDB-R220 scale.  Here the database lives in HBM as an inverted index, k-mer -> genomes, and the
// (much smaller, already sorted) sample tables are streamed against it: O(sample) work per sample instead of O(database).
//
// Index layout: the "line index" (contain_index.h, built by line_index.hip, arithmetic in index_plan.h) — every bucket of the k-mer
// space owns ONE 64-byte line of 8 slots, the HBM access granule, so a probe is exactly one line read; crowded buckets continue in
// an overflow run.
//
// Hits are (row = sample * G + genome, count) keys, radix-sorted: that yields contain_count[sample][genome] and every
// coverage vector already in the ascending order the reference sorts it into (contain.rs:661).  A batch of S samples is ONE
// probe launch over the concatenated tables, one sort, one device->host copy (sylph_db_contain_batch; contain.rs:267-289 is
// the reference's sample-chunk x genome loop).  Pure integer work, HBM-latency bound.
//
// Multi-GPU: a database shard holds the postings of one k-mer RANGE (sylph_db_upload_shard); sample tables are sorted, so
// the part of a sample a rank must probe is a contiguous slice; shard.hip does the exchange.
#include <algorithm>
#include <memory>

#include "contain_index.h"
#include "shard_plan.h"
#include "device_common.h"
#include "row_stats.h"

namespace sylph {
namespace {

// ---- probe -----------------------------------------------------------------------------------------------------------
// One lane per sample k-mer, persistent workgroups striding over 256-k-mer chunks of the concatenated batch.  Hits are
// (row << 32 | count), staged per workgroup in LDS and flushed with one global atomic per ~PROBE_FLUSH hits (one atomic per
// chunk on a single word made the atomic unit 40 % of the kernel: ~88 single-address atomics/us on this chip).
constexpr int PROBE_TPB = 256;
#ifndef SYLPH_PROBE_STAGE
#define SYLPH_PROBE_STAGE 4096
#endif
constexpr int PROBE_STAGE = SYLPH_PROBE_STAGE;
constexpr int PROBE_FLUSH = 2048;
constexpr int PROBE_GRID = 1024;

struct HitStage {
    uint64_t stage[PROBE_STAGE];
    uint32_t cnt, base, max_count;   // max_count: largest count among this workgroup's hits since the last flush
};
__device__ __forceinline__ void hit_stage_init(HitStage& st) {
    if (threadIdx.x == 0) { st.cnt = 0; st.max_count = 0; }
    __syncthreads();
}
__device__ __forceinline__ void hit_stage_push(HitStage& st, uint64_t hit, uint64_t* __restrict__ hits, uint32_t hit_cap,
                                               uint32_t* __restrict__ hit_count) {
    const uint32_t slot = atomicAdd(&st.cnt, 1u);
    if ((uint32_t)hit > st.max_count) atomicMax(&st.max_count, (uint32_t)hit);   // (plain read first: almost never true)
    if (slot < PROBE_STAGE) st.stage[slot] = hit;
    else {                                       // a k-mer shared by thousands of genomes: straight to HBM
        const uint32_t o = atomicAdd(hit_count, 1u);
        if (o < hit_cap) hits[o] = hit;
    }
}
// called by all threads after a chunk; flushes when the stage is filling up or `force`
__device__ __forceinline__ void hit_stage_flush(HitStage& st, bool force, uint64_t* __restrict__ hits, uint32_t hit_cap,
                                                uint32_t* __restrict__ hit_count) {
    __syncthreads();
    const uint32_t n = min(st.cnt, (uint32_t)PROBE_STAGE);
    __syncthreads();                                     // everyone has read cnt before anyone pushes again
    if (n == 0 || (!force && n < PROBE_FLUSH)) return;   // uniform: all lanes saw the same cnt
    if (threadIdx.x == 0) {
        st.base = atomicAdd(hit_count, n);
        atomicMax(hit_count + 1, st.max_count);          // [1] = largest count of any hit (sizes the sort keys)
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < n; t += PROBE_TPB) {
        const uint32_t o = st.base + t;
        if (o < hit_cap) hits[o] = st.stage[t];
    }
    __syncthreads();
    if (threadIdx.x == 0) st.cnt = 0;
    __syncthreads();
}

// The overflow run of a crowded bucket, walked by the whole wavefront: a k-mer that thousands of genomes share (strains of one
// species in an undereplicated database) has thousands of postings behind one descriptor.  One lane walking them one by one,
// each hit a push into the workgroup's stage — or, once that is full, a global atomic on the single hit counter — made the
// probe quadratic in practice (5,000 strains: 1.4 s for one sample).  Here the 64 lanes read 64 entries at a time, count the
// matches (same remainder, genome long enough), take the space for all of them with ONE atomic and write them, coalesced.
// Uniform over the wavefront: every lane gets the same arguments.
__device__ __forceinline__ void probe_long_run(HitStage& st, const LineView& v, uint64_t start, uint64_t rem, uint64_t row0, uint32_t cnt,
                                               const uint32_t* __restrict__ glen, double min_number_kmers, int check_len,
                                               uint64_t* __restrict__ hits, uint32_t hit_cap, uint32_t* __restrict__ hit_count) {
    const uint32_t lane = threadIdx.x & 63;
    // one step: 64 entries from `base`; -> this lane's entry matches and its genome is long enough; ended: the run ends inside the step
    auto step = [&](uint64_t base, uint32_t& g, bool& ended) {
        const LongRunStep r = long_run_step(v, base, rem);
        g = r.g;
        ended = r.ended;
        return r.match && !(check_len && (double)glen[g] < min_number_kmers);          // contain.rs:627
    };
    // room for `total` hits: in the workgroup's stage as far as it reaches (ONE LDS atomic; the stage is flushed with one
    // global atomic per ~2048 hits), the rest straight in the hit array (one global atomic — a single word sustains ~90/us)
    uint32_t stage_at = 0, n_stage = 0, global_at = 0;
    auto reserve = [&](uint32_t total) {
        uint32_t slot = 0, o = 0;
        if (lane == 0) {
            slot = atomicAdd(&st.cnt, total);
            if (cnt > st.max_count) atomicMax(&st.max_count, cnt);
            const uint32_t room = slot < (uint32_t)PROBE_STAGE ? min(total, (uint32_t)PROBE_STAGE - slot) : 0u;
            if (total > room) { o = atomicAdd(hit_count, total - room); atomicMax(hit_count + 1, cnt); }
        }
        stage_at = (uint32_t)__shfl((int)slot, 0);
        global_at = (uint32_t)__shfl((int)o, 0);
        n_stage = stage_at < (uint32_t)PROBE_STAGE ? min(total, (uint32_t)PROBE_STAGE - stage_at) : 0u;
        return 0u;
    };
    auto put = [&](bool match, unsigned long long mm, uint32_t g, uint32_t at) {   // at: matches of the run before this step
        if (!match) return;
        const uint32_t p = at + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
        const uint64_t hit = index_plan::hit_key(row0 + g, cnt);
        if (p < n_stage) st.stage[stage_at + p] = hit;
        else { const uint32_t o = global_at + (p - n_stage); if (o < hit_cap) hits[o] = hit; }
    };
    // first step kept in registers: a run that ends inside it (up to 64 entries from its start) needs no second read
    uint32_t g0;
    bool ended;
    const bool m0 = step(start, g0, ended);
    const unsigned long long mm0 = __ballot(m0);
    uint32_t total = (uint32_t)__popcll(mm0);
    if (ended) {
        if (total) put(m0, mm0, g0, reserve(total));
        return;
    }
    for (uint64_t base = start + 64; !ended; base += 64) {
        uint32_t g;
        total += (uint32_t)__popcll(__ballot(step(base, g, ended)));
    }
    if (total == 0) return;
    uint32_t at = reserve(total);
    put(m0, mm0, g0, at);
    at += (uint32_t)__popcll(mm0);
    ended = false;
    for (uint64_t base = start + 64; !ended; base += 64) {
        uint32_t g;
        const bool m = step(base, g, ended);
        const unsigned long long mm = __ballot(m);
        put(m, mm, g, at);
        at += (uint32_t)__popcll(mm);
    }
}

// PROBE_ILP k-mers per lane and step: their index lines are requested back to back (16 outstanding 16-byte loads per lane
// at ILP 4) before the first one is looked at — with one line per lane in flight the wavefronts sat waiting 80 % of their
// cycles (SQ_WAIT_ANY / SQ_WAVE_CYCLES, round 2) and a single-sample launch reached 22 % of the HBM roofline.
template <int PROBE_ILP>
__global__ __launch_bounds__(PROBE_TPB) void probe_kernel(const SampleRef* __restrict__ refs_mem, RefPack pack, uint32_t n_samples,
                                                          uint32_t n_chunks, LineView v, uint32_t n_genomes, const uint32_t* __restrict__ glen,
                                                          double min_number_kmers, int check_len, uint64_t* __restrict__ hits,
                                                          uint32_t hit_cap, uint32_t* __restrict__ hit_count) {
    __shared__ HitStage st;
    hit_stage_init(st);
    const SampleRef* __restrict__ refs = n_samples <= REFS_INLINE ? pack.r : refs_mem;   // (kernel-argument segment, or HBM)
    // a chunk = PROBE_TPB * PROBE_ILP consecutive entries of ONE sample table (chunk0 counts such chunks)
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        uint32_t s = 0, hi = n_samples;                  // sample of this chunk: largest s with chunk0[s] <= chunk (uniform)
        while (hi - s > 1) {
            const uint32_t mid = s + ((hi - s) >> 1);
            if (refs[mid].chunk0 <= chunk) s = mid; else hi = mid;
        }
        const uint64_t* __restrict__ sk = refs[s].k;
        const uint32_t* __restrict__ sc = refs[s].c;
        const uint64_t n_s = refs[s].n;
        const uint64_t i0 = (uint64_t)(chunk - refs[s].chunk0) * (PROBE_TPB * PROBE_ILP) + threadIdx.x;
        const uint64_t row0 = (uint64_t)s * n_genomes;
        uint32_t cnt[PROBE_ILP];
        uint64_t km[PROBE_ILP];
#pragma unroll
        for (int e = 0; e < PROBE_ILP; e++) {
            const uint64_t i = i0 + (uint64_t)e * PROBE_TPB;
            cnt[e] = i < n_s ? sc[i] : 0u;               // contain.rs:634: nothing for a zero count
            km[e] = i < n_s ? sk[i] : 0ull;
        }
        LineFetch lf[PROBE_ILP];
#pragma unroll
        for (int e = 0; e < PROBE_ILP; e++) lf[e] = line_fetch(v, km[e], cnt[e] != 0);
#pragma unroll
        for (int e = 0; e < PROBE_ILP; e++) {
            uint64_t long_start = ~0ull, long_rem = 0;
            const uint32_t c_e = cnt[e];
            line_scan(v, lf[e], [&](uint32_t g) {
                if (check_len && (double)glen[g] < min_number_kmers) return;     // contain.rs:627
                hit_stage_push(st, index_plan::hit_key(row0 + g, c_e), hits, hit_cap, hit_count);
            }, &long_start, &long_rem);
            for_each_long_run(long_start, long_rem, [&](int src, uint64_t rs, uint64_t rm) {   // by the whole wavefront
                probe_long_run(st, v, rs, rm, row0, (uint32_t)__shfl((int)c_e, src), glen, min_number_kmers, check_len, hits, hit_cap, hit_count);
            });
        }
        hit_stage_flush(st, chunk + gridDim.x >= n_chunks, hits, hit_cap, hit_count);
    }
}

// Profile reassignment on device: winner_table (contain.rs:410-430) + the second get_stats pass (contain.rs:300-307 with
// the winner map, :637-646).  A k-mer belongs to the passing genome with the highest first-pass ANI among those that
// hold it in genome_kmers or in pseudotax_tracked_nonused_kmers; ties go to the genome that comes first in the passing
// list (the reference replaces only on strictly greater ANI, :417).  For every passing genome, sample k-mers of its
// genome_kmers that it does not own count as kmers_lost, the others yield (genome, count) hits as in the first pass.
// The winner search itself is winner_of (contain_index.h), shared with the reassignment log (reassign_edges.hip).
__global__ __launch_bounds__(PROBE_TPB) void reassign_kernel(const uint64_t* __restrict__ s_kmers, const uint32_t* __restrict__ s_counts,
                                                             uint32_t n_sample, LineView kept, LineView tracked, int have_tracked,
                                                             const uint32_t* __restrict__ rank, const double* __restrict__ ani,
                                                             uint32_t* __restrict__ lost, uint64_t* __restrict__ hits, uint32_t hit_cap,
                                                             uint32_t* __restrict__ hit_count) {
    __shared__ HitStage st;
    hit_stage_init(st);
    const uint32_t n_chunks = (n_sample + PROBE_TPB - 1) / PROBE_TPB;
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t i = chunk * PROBE_TPB + threadIdx.x;
        const uint32_t cnt = i < n_sample ? s_counts[i] : 0;                         // contain.rs:634: nothing for a zero count
        const uint64_t km = cnt != 0 ? s_kmers[i] : 0;
        // Three passes over the k-mer's postings, as in the reference: the winner among kept + tracked (winner_of), then lost / kept
        // per genome.  Each pass takes the line and short overflow runs lane by lane; long runs are handed to the whole wavefront.
        uint32_t n_kept;
        const uint32_t best_rank = winner_of<true>(kept, tracked, have_tracked, km, cnt != 0, rank, ani, n_kept);
        auto settle = [&](uint32_t g, uint32_t winner, uint32_t c) {
            const uint32_t r = rank[g];
            if (r == 0xFFFFFFFFu) return;                                            // not in remaining_genomes
            if (r != winner) { atomicAdd(&lost[g], 1u); return; }                    // contain.rs:639-642
            hit_stage_push(st, index_plan::hit_key(g, c), hits, hit_cap, hit_count);
        };
        uint64_t ls3 = ~0ull, lr3 = 0;
        if (n_kept) for_each_posting(kept, km, [&](uint32_t g) { settle(g, best_rank, cnt); }, &ls3, &lr3);
        for_each_long_run(ls3, lr3, [&](int src, uint64_t rs, uint64_t rm) {
            const uint32_t winner = (uint32_t)__shfl((int)best_rank, src), c_s = (uint32_t)__shfl((int)cnt, src);
            long_run_for_each(kept, rs, rm, [&](uint32_t g) { settle(g, winner, c_s); });
        });
        hit_stage_flush(st, chunk + gridDim.x >= n_chunks, hits, hit_cap, hit_count);
    }
}

// Sorted hit keys of type K = (row << shift) | count -> cov_off[r] = first hit with row >= r, contain_count[r] = hits of row r.
// 64-bit keys have shift 32; compact 32-bit keys (index_plan::compact_key) have shift cb, the bit length of the largest count:
// the radix sort of the hit list then moves 4-byte keys through 3-4 passes instead of 8-byte keys through 8.
template <class K>
__global__ __launch_bounds__(256) void hit_offsets_kernel(const K* __restrict__ keys, uint32_t n_hits, uint32_t n_rows, int shift,
                                                          uint64_t* __restrict__ cov_off, uint32_t* __restrict__ contain_count) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > n_rows) return;
    auto lower = [&](uint64_t key) {   // first hit whose key is >= key
        uint32_t lo = 0, hi = n_hits;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if ((uint64_t)keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    const uint32_t a = lower((uint64_t)g << shift);
    cov_off[g] = a;
    if (g < n_rows) contain_count[g] = lower(((uint64_t)g + 1) << shift) - a;
}
__global__ __launch_bounds__(256) void pack_hits32_kernel(const uint64_t* __restrict__ hits, uint32_t n, int cb, uint32_t* __restrict__ k32) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const uint64_t h = hits[i]; k32[i] = ((uint32_t)(h >> 32) << cb) | (uint32_t)h; }
}
// covs[i] = the count of sorted key i (its low `shift` bits), as T
template <class K, class T>
__global__ __launch_bounds__(256) void narrow_kernel(const K* __restrict__ keys, uint32_t n, int shift, T* __restrict__ covs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) covs[i] = (T)(keys[i] & (((K)1 << shift) - 1));
}

}  // namespace

static uint32_t probe_grid() {
    static const uint32_t g = getenv("SYLPH_HIP_PROBE_GRID") ? (uint32_t)atoi(getenv("SYLPH_HIP_PROBE_GRID")) : PROBE_GRID;
    return std::max<uint32_t>(1, g);
}

// common front of the two probe entry points: chunk numbering, limits, descriptors; returns the number of chunks (0: nothing to do)
static uint64_t probe_prepare(sylph_db* db, std::vector<SampleRef>& refs, uint64_t* total_out, RefPack* pack, uint64_t* ilp_out) {
    sylph_ctx* ctx = db->ctx;
    const uint64_t G = db->n_genomes;
    uint64_t total = 0, chunks = 0;
    static const int ilp_env = getenv("SYLPH_HIP_PROBE_ILP") ? atoi(getenv("SYLPH_HIP_PROBE_ILP")) : 0;   // tuning knob
    const uint64_t ilp = ilp_env == 1 || ilp_env == 2 || ilp_env == 4 ? (uint64_t)ilp_env : 2;   // measured: 2 is best (profiles/r03_probe_ilp.txt)
    for (auto& r : refs) {
        SY_REQUIRE(r.n < (1ull << 32), "sample table larger than 2^32-1 entries");
        SY_REQUIRE(chunks < (1ull << 32), "batch too large");
        r.chunk0 = (uint32_t)chunks;
        r.pad = 0;
        chunks += (r.n + PROBE_TPB * ilp - 1) / (PROBE_TPB * ilp);
        total += r.n;
    }
    SY_REQUIRE(chunks < (1ull << 32) && total < (1ull << 32), "batch holds more than 2^32-1 k-mers: split it");
    SY_REQUIRE((uint64_t)refs.size() * std::max<uint64_t>(G, 1) < (1ull << 32) - 1, "samples x genomes must stay below 2^32: split the batch");
    *total_out = total;
    *ilp_out = ilp;
    if (!total || !db->kept.n_postings) return 0;
    if (refs.size() <= REFS_INLINE) {
        for (size_t i = 0; i < refs.size(); i++) pack->r[i] = refs[i];
    } else {
        db->q_refs.reserve(refs.size() * sizeof(SampleRef));
        ctx->h2d(db->q_refs.p, refs.data(), refs.size() * sizeof(SampleRef));
    }
    return chunks;
}

static void probe_launch(sylph_db* db, const std::vector<SampleRef>& refs, const RefPack& pack, uint64_t chunks, uint64_t ilp, double min_number_kmers,
                         uint64_t cap) {
    sylph_ctx* ctx = db->ctx;
    const uint64_t G = db->n_genomes;
    uint32_t* d_cnt = db->counter.as<uint32_t>();   // [0] = number of hits, [1] = largest count among the hits
    const int check_len = (double)db->min_glen < min_number_kmers;
    SY_REQUIRE(hits_plan::fits(cap), "more than 2^32-1 hits for one batch: split it");
    db->hits.reserve(cap * 8);
    if (db->cnt_dirty) SY_HIP(hipMemsetAsync(d_cnt, 0, 8, ctx->stream));   // (the flag: finish_driver, from the plan's record)
    ScopedKernelTimer t(ctx, "probe");
#define SY_LAUNCH_PROBE(I)                                                                                                                   \
    hipLaunchKernelGGL(probe_kernel<I>, dim3(std::min<uint32_t>((uint32_t)chunks, probe_grid())), dim3(PROBE_TPB), 0, ctx->stream,            \
                       db->q_refs.as<SampleRef>(), pack, (uint32_t)refs.size(), (uint32_t)chunks, db->kept.view(), (uint32_t)G,               \
                       db->glen.as<uint32_t>(), min_number_kmers, check_len, db->hits.as<uint64_t>(), (uint32_t)cap, d_cnt)
    if (ilp == 4) SY_LAUNCH_PROBE(4); else if (ilp == 2) SY_LAUNCH_PROBE(2); else SY_LAUNCH_PROBE(1);
#undef SY_LAUNCH_PROBE
    SY_HIP(hipGetLastError());
}

// copies the block assembled in db->res out — straight into pinned host memory (the db's own block or the caller's, which carries its
// layout itself; no staging copy, nothing pageable registered with HIP), one copy, + kmers_lost — and waits for it
// With a row filter (db->row_filter, a pipeline's probe batch): the rows of the block in db->res are summarised on the device
// (row_stats.hip) and only the candidates travel — their summaries, offsets and values, and where every sample's values began
// (CandidateLayout).  The sizes come from the device: row_stats_device reads its two totals back, which is one small synchronisation
// more than the plain road's; the copy is sized by them.
static void copy_out_candidates(sylph_db* db, uint32_t n_hits, uint32_t width, uint64_t n_rows, HostBlock* dst) {
    sylph_ctx* ctx = db->ctx;
    const uint64_t G = db->n_genomes, n_samples = G ? n_rows / G : 0;
    const ResultLayout lay(n_rows, n_hits, width, 0);
    const char* d = db->res.as<char>();
    RowStatsResult res(ctx);
    row_stats_device(ctx, d + lay.covs, width, (const uint64_t*)d, db->glen.as<uint32_t>(), (uint32_t)G, (uint32_t)n_rows, n_hits, *db->row_filter, res);
    const CandidateLayout c(res.n, res.n_vals, width, n_samples);
    dst->ensure(c.end + 64);
    dst->lay = lay;
    dst->cand = c;
    char* h = (char*)dst->p;
    if (res.n) SY_HIP(hipMemcpyAsync(h, res.rows.p, (size_t)res.n * sizeof(row_stats_plan::RowSummary), hipMemcpyDeviceToHost, ctx->stream));
    SY_HIP(hipMemcpyAsync(h + c.off, res.cov_off.p, ((size_t)res.n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (res.n_vals) SY_HIP(hipMemcpyAsync(h + c.covs, res.covs.p, (size_t)res.n_vals * width, hipMemcpyDeviceToHost, ctx->stream));
    if (n_rows) SY_HIP(hipMemcpyAsync(h + c.sample_off, res.sample_off.p, ((size_t)n_samples + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    else memset(h + c.sample_off, 0, 8);
    SY_HIP(hipStreamSynchronize(ctx->stream));
    if (!ctx->pending.empty()) profile_collect(ctx);
}

static void copy_out_rows(sylph_db* db, uint32_t n_hits, uint32_t width, uint64_t n_rows, bool with_lost, HostBlock* dst) {
    sylph_ctx* ctx = db->ctx;
    const uint64_t G = db->n_genomes;
    if (db->row_filter && dst && !with_lost) { copy_out_candidates(db, n_hits, width, n_rows, dst); return; }
    if (dst) dst->cand = CandidateLayout();
    const ResultLayout lay(n_rows, n_hits, width, with_lost ? G : 0);
    if (!dst) dst = &db->h_block;
    dst->ensure(lay.end + 64);
    dst->lay = lay;
    char* h = (char*)dst->p;
    SY_HIP(hipMemcpyAsync(h, db->res.p, lay.covs + (size_t)n_hits * width, hipMemcpyDeviceToHost, ctx->stream));
    if (with_lost && G) SY_HIP(hipMemcpyAsync(h + lay.lost, db->lost.p, G * 4, hipMemcpyDeviceToHost, ctx->stream));
    SY_HIP(hipStreamSynchronize(ctx->stream));
    if (!ctx->pending.empty()) profile_collect(ctx);
}

// The sorted finish: the hit list radix-sorted by (row, count), offsets by binary search.
// cov_width: nullptr = coverage values as u32; else in/out — the values are stored with the narrowest of 1, 2 or 4 bytes
// that holds the batch's largest count (7.4 MB -> 1.9 MB over PCIe per sample at GTDB scale) and the width is returned.
static void finish_hits_sorted(sylph_db* db, uint32_t n_hits, uint32_t max_count, uint64_t n_rows, uint32_t* cov_width, bool with_lost, HostBlock* dst) {
    sylph_ctx* ctx = db->ctx;
    SY_REQUIRE(n_rows < (1ull << 32) - 1, "too many result rows");
    const index_plan::CompactKey ck = index_plan::compact_key(max_count, n_rows);
    const bool compact = n_hits && ck.fits;
    const uint32_t width = index_plan::coverage_width(cov_width && compact, max_count);   // (64-bit hit keys report u32)
    const ResultLayout lay(n_rows, n_hits, width, with_lost ? db->n_genomes : 0);
    db->res.reserve(lay.lost + 64);
    char* d_res = db->res.as<char>();
    uint64_t* d_cov_off = reinterpret_cast<uint64_t*>(d_res);
    uint32_t* d_ccount = reinterpret_cast<uint32_t*>(d_res + lay.ccount);
    void* d_covs = d_res + lay.covs;
    const dim3 g_hits(grid_for64(n_hits)), g_rows(grid_for64(n_rows + 1)), tpb(256);
    if (compact) {
        db->hits_sorted.reserve((size_t)n_hits * 8);   // two u32 arrays: packed keys, sorted keys
        uint32_t* k32 = db->hits_sorted.as<uint32_t>();
        uint32_t* k32s = k32 + n_hits;
        hipLaunchKernelGGL(pack_hits32_kernel, g_hits, tpb, 0, ctx->stream, db->hits.as<uint64_t>(), n_hits, ck.cb, k32);
        sort_keys_u32(ctx, k32, k32s, n_hits, 0, ck.cb + ck.rb);
        if (width == 1) hipLaunchKernelGGL((narrow_kernel<uint32_t, uint8_t>), g_hits, tpb, 0, ctx->stream, k32s, n_hits, ck.cb, (uint8_t*)d_covs);
        else if (width == 2) hipLaunchKernelGGL((narrow_kernel<uint32_t, uint16_t>), g_hits, tpb, 0, ctx->stream, k32s, n_hits, ck.cb, (uint16_t*)d_covs);
        else hipLaunchKernelGGL((narrow_kernel<uint32_t, uint32_t>), g_hits, tpb, 0, ctx->stream, k32s, n_hits, ck.cb, (uint32_t*)d_covs);
        hipLaunchKernelGGL(hit_offsets_kernel<uint32_t>, g_rows, tpb, 0, ctx->stream, k32s, n_hits, (uint32_t)n_rows, ck.cb, d_cov_off, d_ccount);
    } else {
        const uint64_t* d_sorted = nullptr;
        if (n_hits) {
            db->hits_sorted.reserve((size_t)n_hits * 8);
            sort_keys_u64(ctx, db->hits.as<uint64_t>(), db->hits_sorted.as<uint64_t>(), n_hits, 0, 64);
            d_sorted = db->hits_sorted.as<uint64_t>();
            hipLaunchKernelGGL((narrow_kernel<uint64_t, uint32_t>), g_hits, tpb, 0, ctx->stream, d_sorted, n_hits, 32, (uint32_t*)d_covs);
        }
        hipLaunchKernelGGL(hit_offsets_kernel<uint64_t>, g_rows, tpb, 0, ctx->stream, d_sorted, n_hits, (uint32_t)n_rows, 32, d_cov_off, d_ccount);
    }
    SY_HIP(hipGetLastError());
    if (cov_width) *cov_width = width;
    copy_out_rows(db, n_hits, width, n_rows, with_lost, dst);
}

// The hit finish: from "probe this" or "these many hits lie in db->hits" to the result block in `dst`, one loop over the plan
// (hits_plan.h).  The plan names the step — probe, assemble, read the two words, probe once more with room for all the hits, the sorted
// finish, copy out — from the road the job asks for and the verdict on the list's sizes; this function only carries the steps out,
// and sets the database's two clean-on-entry flags from the plan's record behind every step.  SYLPH_HIP_HIT_SORT (A/B knob: the sorted
// path of rounds 1-3 for every call) is read here and nowhere else.
HitSizes finish_driver(sylph_db* db, const HitFinish& job) {
    namespace hp = hits_plan;
    sylph_ctx* ctx = db->ctx;
    static const bool force_sorted = getenv("SYLPH_HIP_HIT_SORT") != nullptr;
    const bool to_probe = job.probe.call != nullptr;
    uint32_t n_hits = job.n_hits, max_count = job.max_count;
    uint64_t cap = to_probe ? hp::first_capacity(job.total) : std::max<uint32_t>(n_hits, 1);
    const ResultLayout lay0(job.n_rows, 0, 4, 0);
    hp::State s = hp::start(to_probe, job.sizes, force_sorted, hp::geometry(job.n_rows, 1, 0).taken, job.finish, db->rc_dirty, db->cnt_dirty,
                            hp::verdict(n_hits, max_count, (uint32_t)cap));
    auto record = [&] { db->rc_dirty = s.rc_dirty; db->cnt_dirty = s.cnt_dirty; };
    try {
        for (;;) {
            const hp::Step step = hp::next(s);
            hp::Verdict answer = hp::Verdict::Rows;
            switch (step) {
            case hp::Step::RegrowProbe:
                cap = n_hits;
                [[fallthrough]];
            case hp::Step::Probe:
                job.probe.call(job.probe.self, cap, (int)s.probes);
                if (hp::behind_probe(s)) {                       // the two words on their way to pinned memory, in front of the assembly
                    if (!db->ev_cnt) SY_HIP(hipEventCreateWithFlags(&db->ev_cnt, hipEventDisableTiming));
                    SY_HIP(hipMemcpyAsync((char*)ctx->pinned + 256, db->counter.p, 8, hipMemcpyDeviceToHost, ctx->stream));
                    SY_HIP(hipEventRecord(db->ev_cnt, ctx->stream));
                }
                break;
            case hp::Step::Assemble: {
                const bool behind = !s.read;                     // sizes from the device words; else the host's, in an array of just that size
                const uint64_t room = behind ? cap : std::max<uint32_t>(n_hits, 1);
                const hp::Geometry g = hp::geometry(job.n_rows, room, behind ? room / 2 : n_hits);
                db->res.reserve(lay0.covs + (size_t)room * 4 + 64);
                ScopedKernelTimer t(ctx, "assemble");
                launch_row_assembly(db, g, behind ? db->counter.as<uint32_t>() : nullptr, n_hits, max_count, (uint32_t)room, job.cov_width ? 1 : 0,
                                    db->res.as<char>(), lay0.covs, lay0.ccount);
                break;
            }
            case hp::Step::ReadWords: {
                uint32_t hc[2];
                if (hp::behind_probe(s)) {
                    SY_HIP(hipEventSynchronize(db->ev_cnt));     // (the assembly's kernels are still running)
                    memcpy(hc, (const char*)ctx->pinned + 256, 8);
                } else ctx->read_back(hc, db->counter.p, 8);
                n_hits = hc[0];
                max_count = hc[1];
                answer = hp::verdict(n_hits, max_count, (uint32_t)cap);
                break;
            }
            case hp::Step::Sorted:
                // (host-known sizes that the row road turns down have always counted one empty "assemble" interval)
                if (s.sizes == hp::Sizes::Host && !force_sorted && job.n_rows) { ScopedKernelTimer t(ctx, "assemble"); }
                finish_hits_sorted(db, n_hits, max_count, job.n_rows, job.cov_width, job.with_lost, job.dst);
                return HitSizes{n_hits, max_count};
            case hp::Step::CopyOut: {
                const uint32_t width = index_plan::coverage_width(job.cov_width != nullptr, max_count);
                if (job.cov_width) *job.cov_width = width;
                copy_out_rows(db, n_hits, width, job.n_rows, job.with_lost, job.dst);
                return HitSizes{n_hits, max_count};
            }
            case hp::Step::Done:
                return HitSizes{n_hits, max_count};
            case hp::Step::Fail:
                SY_REQUIRE(false, "hit buffer overflow persisted");
            }
            s = hp::after(s, step, answer);
            record();
        }
    } catch (...) {
        s = hp::failed(s);
        record();
        throw;
    }
}

// "probe these refs": the driver over probe_launch
static HitSizes drive_refs(sylph_db* db, std::vector<SampleRef>& refs, double min_number_kmers, HitFinish job) {
    uint64_t total = 0, ilp = 2;
    RefPack pack{};
    const uint64_t chunks = refs.empty() ? 0 : probe_prepare(db, refs, &total, &pack, &ilp);
    auto launch = [&](uint64_t cap, int) { probe_launch(db, refs, pack, chunks, ilp, min_number_kmers, cap); };
    if (chunks) { job.probe = ProbeStep(launch); job.total = total; }
    return finish_driver(db, job);
}

uint32_t probe_batch(sylph_db* db, std::vector<SampleRef>& refs, double min_number_kmers, uint32_t* max_count) {
    HitFinish job;
    job.finish = false;
    const HitSizes z = drive_refs(db, refs, min_number_kmers, job);
    *max_count = z.max_count;
    return z.n_hits;
}

// Probe + finish of a batch of device-resident tables into `dst` (nullptr: the database's block): the assembly runs behind the probe,
// without a host round trip between them.  Returns the number of hits.
static uint32_t contain_refs(sylph_db* db, std::vector<SampleRef>& refs, double min_number_kmers, uint64_t n_rows, uint32_t* cov_width, HostBlock* dst) {
    SY_REQUIRE(n_rows < (1ull << 32) - 1, "too many result rows");
    HitFinish job;
    job.sizes = hits_plan::Sizes::Device;
    job.n_rows = n_rows;
    job.cov_width = cov_width;
    job.dst = dst;
    return drive_refs(db, refs, min_number_kmers, job).n_hits;
}

}  // namespace sylph

using namespace sylph;

struct ReassignArgs { const uint32_t* passing_gids; const double* passing_ani; uint32_t n_passing; };

// single-sample entry points (and the reassignment pass): results in db->h_res, returns the number of hits
static uint32_t contain_impl(sylph_db* db, const uint64_t* sample_kmers, const uint32_t* sample_counts, uint64_t n, int mem,
                             double min_number_kmers, const ReassignArgs* re = nullptr, uint32_t* cov_width = nullptr) {
    SY_REQUIRE(mem == SYLPH_MEM_HOST || mem == SYLPH_MEM_DEVICE, "bad mem kind %d", mem);
    SY_REQUIRE(n < (1ull << 32), "sample table larger than 2^32-1 entries");
    SY_REQUIRE(db->world == 1, "this database is one shard of %u: use sylph_db_contain_batch_sharded", db->world);
    sylph_ctx* ctx = db->ctx;
    const uint64_t G = db->n_genomes;
    const uint64_t* d_k = sample_kmers;
    const uint32_t* d_c = sample_counts;
    if (n && mem == SYLPH_MEM_HOST) {
        SY_REQUIRE(sample_kmers && sample_counts, "null sample");
        db->q_kmers.reserve(n * 8);
        db->q_counts.reserve(n * 4);
        ctx->h2d(db->q_kmers.p, sample_kmers, n * 8);
        ctx->h2d(db->q_counts.p, sample_counts, n * 4);
        d_k = db->q_kmers.as<uint64_t>();
        d_c = db->q_counts.as<uint32_t>();
    }
    if (!re) {
        if (n) SY_REQUIRE(d_k && d_c, "null sample");
        std::vector<SampleRef> refs(1);
        refs[0].k = d_k; refs[0].c = d_c; refs[0].n = n;
        return contain_refs(db, refs, min_number_kmers, G, cov_width, nullptr);
    }
    // rank[g] = position of genome g in the passing list (or ~0), ani[rank], lost[g] = 0
    SY_REQUIRE(re->n_passing == 0 || (re->passing_gids && re->passing_ani), "null passing list");
    std::vector<uint32_t> rank(std::max<uint64_t>(1, G), 0xFFFFFFFFu);
    for (uint32_t r = 0; r < re->n_passing; r++) {
        SY_REQUIRE(re->passing_gids[r] < G, "passing genome id %u out of range", re->passing_gids[r]);
        SY_REQUIRE(rank[re->passing_gids[r]] == 0xFFFFFFFFu, "genome %u listed twice", re->passing_gids[r]);
        rank[re->passing_gids[r]] = r;
    }
    db->rank_of.reserve(rank.size() * 4);
    db->ani.reserve(std::max<size_t>(1, re->n_passing) * 8);
    db->lost.reserve(rank.size() * 4);
    ctx->h2d(db->rank_of.p, rank.data(), rank.size() * 4);
    if (re->n_passing) ctx->h2d(db->ani.p, re->passing_ani, (size_t)re->n_passing * 8);
    SY_HIP(hipMemsetAsync(db->lost.p, 0, rank.size() * 4, ctx->stream));
    // the pass's launch is the driver's probe step: it counts into the probe's two words, and the host waits for them
    uint32_t* d_cnt = db->counter.as<uint32_t>();
    auto launch = [&](uint64_t cap, int attempt) {
        SY_REQUIRE(hits_plan::fits(cap), "more than 2^32-1 hits for one sample");
        db->hits.reserve(cap * 8);
        SY_HIP(hipMemsetAsync(d_cnt, 0, 8, ctx->stream));
        if (attempt) SY_HIP(hipMemsetAsync(db->lost.p, 0, std::max<uint64_t>(1, G) * 4, ctx->stream));
        ScopedKernelTimer t(ctx, "probe");
        hipLaunchKernelGGL(reassign_kernel, dim3(std::min<uint32_t>(grid_for64(n, PROBE_TPB), probe_grid())), dim3(PROBE_TPB), 0, ctx->stream,
                           d_k, d_c, (uint32_t)n, db->kept.view(), db->tracked.view(), db->tracked.n_postings ? 1 : 0,
                           db->rank_of.as<uint32_t>(), db->ani.as<double>(), db->lost.as<uint32_t>(), db->hits.as<uint64_t>(),
                           (uint32_t)cap, d_cnt);
        SY_HIP(hipGetLastError());
    };
    HitFinish job;
    job.n_rows = G;
    job.cov_width = cov_width;
    job.with_lost = true;
    if (n && db->kept.n_postings && re->n_passing) {
        SY_REQUIRE(d_k && d_c, "null sample");
        job.probe = ProbeStep(launch);
        job.total = n;
    }
    return finish_driver(db, job).n_hits;
}

uint32_t sylph::contain_batch_impl(sylph_db* db, const sylph_sample_ref* samples, uint32_t n_samples, int mem, double min_number_kmers,
                                   uint32_t* cov_width, HostBlock* dst, ResultViews* views, const row_stats_plan::Filter* row_filter) {
    SY_REQUIRE(db && cov_width, "null argument");
    SY_REQUIRE(!row_filter || dst, "a row filter needs a block of the caller's");
    SY_REQUIRE(n_samples == 0 || samples, "null samples");
    SY_REQUIRE(mem == SYLPH_MEM_HOST || mem == SYLPH_MEM_DEVICE, "bad mem kind %d", mem);
    SY_REQUIRE(db->world == 1, "this database is one shard of %u: use sylph_db_contain_batch_sharded", db->world);
    sylph_ctx* ctx = db->ctx;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard dg(ctx->device);
    struct FilterScope {      // the filter holds for this call alone
        sylph_db* db;
        FilterScope(sylph_db* d, const row_stats_plan::Filter* f) : db(d) { db->row_filter = f; }
        ~FilterScope() { db->row_filter = nullptr; }
    } filter_scope(db, row_filter);
    std::vector<SampleRef> refs(n_samples);
    uint64_t total = 0;
    for (uint32_t s = 0; s < n_samples; s++) {
        SY_REQUIRE(samples[s].n == 0 || (samples[s].kmers && samples[s].counts), "null sample %u", s);
        total += samples[s].n;
    }
    if (mem == SYLPH_MEM_HOST && total) {   // stage the tables back to back
        db->q_kmers.reserve(total * 8);
        db->q_counts.reserve(total * 4);
        uint64_t o = 0;
        for (uint32_t s = 0; s < n_samples; s++) {
            const uint64_t n = samples[s].n;
            if (n) {
                ctx->h2d(db->q_kmers.as<uint64_t>() + o, samples[s].kmers, n * 8);
                ctx->h2d(db->q_counts.as<uint32_t>() + o, samples[s].counts, n * 4);
            }
            refs[s].k = db->q_kmers.as<uint64_t>() + o;
            refs[s].c = db->q_counts.as<uint32_t>() + o;
            refs[s].n = n;
            o += n;
        }
    } else {
        for (uint32_t s = 0; s < n_samples; s++) { refs[s].k = samples[s].kmers; refs[s].c = samples[s].counts; refs[s].n = samples[s].n; }
    }
    const uint32_t n_hits = contain_refs(db, refs, min_number_kmers, (uint64_t)n_samples * db->n_genomes, cov_width, dst);
    fill_views(dst ? *dst : db->h_block, views);
    return n_hits;
}

// the three result pointers into the database's own block
template <class T>
static void own_views(const sylph_db* db, const uint64_t** cov_off, const uint32_t** contain_count, const T** covs) {
    ResultViews v;
    fill_views(db->h_block, &v);
    *cov_off = v.cov_off;
    *contain_count = v.contain_count;
    *covs = (const T*)v.covs;
}

extern "C" {

int sylph_db_contain_view(sylph_db* db, const uint64_t* sample_kmers, const uint32_t* sample_counts, uint64_t n, int mem,
                          double min_number_kmers, const uint32_t** contain_count, const uint64_t** cov_off,
                          const uint32_t** covs, uint64_t* out_n_covs) {
    return guarded([&] {
        SY_REQUIRE(db && contain_count && cov_off && covs, "null argument");
        std::lock_guard<std::mutex> lock(db->ctx->mu);
        DeviceGuard dg(db->ctx->device);
        const uint32_t n_hits = contain_impl(db, sample_kmers, sample_counts, n, mem, min_number_kmers);
        own_views(db, cov_off, contain_count, covs);
        if (out_n_covs) *out_n_covs = n_hits;
    });
}

int sylph_db_contain_view_packed(sylph_db* db, const uint64_t* sample_kmers, const uint32_t* sample_counts, uint64_t n, int mem,
                                 double min_number_kmers, const uint32_t** contain_count, const uint64_t** cov_off,
                                 const void** covs, uint32_t* cov_width, uint64_t* out_n_covs) {
    return guarded([&] {
        SY_REQUIRE(db && contain_count && cov_off && covs && cov_width, "null argument");
        std::lock_guard<std::mutex> lock(db->ctx->mu);
        DeviceGuard dg(db->ctx->device);
        const uint32_t n_hits = contain_impl(db, sample_kmers, sample_counts, n, mem, min_number_kmers, nullptr, cov_width);
        own_views(db, cov_off, contain_count, covs);
        if (out_n_covs) *out_n_covs = n_hits;
    });
}

int sylph_db_contain_batch(sylph_db* db, const sylph_sample_ref* samples, uint32_t n_samples, int mem, double min_number_kmers,
                           const uint32_t** contain_count, const uint64_t** cov_off, const void** covs, uint32_t* cov_width,
                           uint64_t* out_n_covs) {
    return guarded([&] {
        SY_REQUIRE(db && contain_count && cov_off && covs && cov_width, "null argument");
        ResultViews v;   // taken under the context lock inside the call (a pipeline may share this database)
        const uint32_t n_hits = contain_batch_impl(db, samples, n_samples, mem, min_number_kmers, cov_width, nullptr, &v);
        *cov_off = v.cov_off;
        *contain_count = v.contain_count;
        *covs = v.covs;
        if (out_n_covs) *out_n_covs = n_hits;
    });
}

int sylph_db_reassign_view(sylph_db* db, const uint64_t* sample_kmers, const uint32_t* sample_counts, uint64_t n, int mem,
                           const uint32_t* passing_gids, const double* passing_ani, uint32_t n_passing,
                           const uint32_t** contain_count, const uint64_t** cov_off, const uint32_t** covs, uint64_t* out_n_covs,
                           const uint32_t** kmers_lost) {
    return guarded([&] {
        SY_REQUIRE(db && contain_count && cov_off && covs && kmers_lost, "null argument");
        std::lock_guard<std::mutex> lock(db->ctx->mu);
        DeviceGuard dg(db->ctx->device);
        ReassignArgs re{passing_gids, passing_ani, n_passing};
        const uint32_t n_hits = contain_impl(db, sample_kmers, sample_counts, n, mem, 0.0, &re);
        own_views(db, cov_off, contain_count, covs);
        *kmers_lost = (const uint32_t*)((const char*)db->h_block.p + db->h_block.lay.lost);
        if (out_n_covs) *out_n_covs = n_hits;
    });
}

int sylph_db_contain(sylph_db* db, const uint64_t* sample_kmers, const uint32_t* sample_counts, uint64_t n, int mem,
                     double min_number_kmers, uint32_t* contain_count, uint64_t* cov_off, uint32_t** out_covs) {
    return guarded([&] {
        SY_REQUIRE(db && contain_count && cov_off && out_covs, "null argument");
        std::lock_guard<std::mutex> lock(db->ctx->mu);
        DeviceGuard dg(db->ctx->device);
        const uint32_t n_hits = contain_impl(db, sample_kmers, sample_counts, n, mem, min_number_kmers);
        const uint64_t G = db->n_genomes;
        ResultViews v;
        fill_views(db->h_block, &v);
        uint32_t* hcov = (uint32_t*)malloc(std::max<size_t>(1, n_hits) * 4);
        if (!hcov) throw std::bad_alloc();
        memcpy(cov_off, v.cov_off, (G + 1) * 8);
        if (G) memcpy(contain_count, v.contain_count, G * 4);
        if (n_hits) memcpy(hcov, v.covs, (size_t)n_hits * 4);
        *out_covs = hcov;
    });
}

void sylph_db_destroy(sylph_db* db) {
    if (!db) return;
    sylph_ctx* ctx = db->ctx;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        delete db;
    }
    ctx_unref(ctx);
}

}  // extern "C"

