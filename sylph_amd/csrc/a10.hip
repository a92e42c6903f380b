// a10.hip — the reference's DEFAULT paired-end dedup: dup_removal_lsh_full (sketch.rs:733-769) over a scalable cuckoo filter (built at
// sketch.rs:796-804: initial capacity 10^7, false-positive probability --fpr; cmdline.rs:77).  The argument is DESIGN.md §1's; in short: as
// long as no insertion fails (the filters run at <= 60 % load), contains(x) <=> some item inserted earlier has the same reduced key
// g(x) = (fingerprint, smaller of its two buckets), whatever the evictions did.  The walk — test, insert when absent — therefore reduces to
// "x is contained iff it is not the FIRST operation of its reduced-key class", over all operations of the sample in file order (two per
// occurrence: (k-mer, markers.0) then (k-mer, markers.1); classes span k-mers — that is what a false positive is).  The phase walk enters
// every operation into a device-wide table keyed by g with an atomic minimum of its place, a second pass compares; the occurrence whose
// test came back "contained" gets RID_A10_BIT, which the replay reads where the exact path compares markers.  Growth: filter j holds
// cap0 * 2^j items at fpr * 0.9^j, and the operation that opens filter j + 1 has cap_j inserting operations of phase j before it: the
// phases are resolved one after the other.  The crate (scalable_cuckoo_filter 0.2.4) is not in the reference tree: structure and growth
// follow its documentation, the hash bits are this repository's (the tests' CPU model; the two agree bit for bit, tests/test_gpu_parity.py).
#include <memory>

#include "common.h"
#include "device_common.h"
#include "sketch_session.h"
#include "partition.h"

namespace sylph {
namespace {

using namespace a10_plan;     // hashes and keys, filter and table geometry, ranges, slots, slices, grid, cut search: a10_plan.h (tested on the CPU)

struct alignas(16) Ent { unsigned long long key; unsigned long long inv_op; };   // inv_op = NO_OP - earliest operation of the class (0: none yet)
static_assert(sizeof(Ent) == 16, "table entry");

struct Filter {
    Ent* tab;
    uint32_t tab_shift;       // slot of a key = table_home(key, tab_shift)
    uint32_t tab_mask;
    FilterGeom geo;           // fingerprint and bucket masks: reduced_key
    uint64_t cut;             // operations >= cut did not insert into this filter (NO_OP while it is the current one)
};
struct Filters { Filter f[MAX_FILTERS]; int n; uint64_t begin, end; };   // operations in [begin, end) are this phase's

// Lookups run in kernels of their own, behind the one that filled the table (or on closed tables): one plain 16-byte load per slot.
__device__ __forceinline__ uint64_t table_first_op(const Filter& d, uint64_t g) {
    uint32_t s = table_home(g, d.tab_shift);
    for (;;) {
        const ulonglong2 e = *reinterpret_cast<const ulonglong2*>(&d.tab[s]);
        if (e.x == g) return NO_OP - e.y;
        if (e.x == 0) return NO_OP;
        s = (s + 1) & d.tab_mask;
    }
}
// The slot's key is read first (an agent-scope load: the table is written with device-scope atomics, which act behind the XCDs'
// L2s) and claimed only when it is empty; a later operation of a class whose earlier one is already in place leaves without the
// second atomic (threads run roughly in file order).  (Claiming first — one compare-and-swap that also tells whose slot it is —
// measured 6 % slower for the whole sample: a failed compare-and-swap costs more than the load it replaces.)
__device__ __forceinline__ void table_enter(const Filter& d, uint64_t g, uint64_t op) {
    uint32_t s = table_home(g, d.tab_shift);
    const unsigned long long mine = NO_OP - op;
    for (;;) {
        unsigned long long k = __hip_atomic_load(&d.tab[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0) k = atomicCAS(&d.tab[s].key, 0ull, (unsigned long long)g);
        if (k == 0 || k == g) {
            if (k == 0 || __hip_atomic_load(&d.tab[s].inv_op, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine) atomicMax(&d.tab[s].inv_op, mine);
            return;
        }
        s = (s + 1) & d.tab_mask;
    }
}

struct Occs { const uint64_t* hash; OccRec* recs; uint32_t n; const uint8_t* part; };   // part[i]: occurrence i takes part (a10_part_kernel)

// Occurrence i takes part in the filter's bookkeeping iff it is valid, its pair has markers (sketch.rs:745) and it is not a
// mate-2 occurrence of a k-mer that mate 1 of the same pair produced too (:852).  The dense arrays are in file order record by
// record: the pair's mate-1 occurrences lie right before its mate-2 occurrences.
// (The walk is linear in the pair's seeds in front of i — quadratic per pair, which only shows for pairs of long reads at c = 1: it
//  is done ONCE per sample, by a10_part_kernel; every other kernel reads its verdict.)
__device__ __forceinline__ bool walk_takes_part(const Occs& o, uint32_t i, uint64_t km, uint64_t rid) {
    if (km == INVALID_HASH || !(rid & RID_MARKER_BIT)) return false;
    const uint64_t rec = rid & RID_MASK;
    bool mate1_has_it = false;
    if (rec & 1) {
        for (uint32_t j = i; j > 0 && !mate1_has_it;) {
            j--;
            const uint64_t hj = o.hash[j];
            if (hj == INVALID_HASH) continue;
            const uint64_t rj = o.recs[j].rid & RID_MASK;
            if ((rj >> 1) != (rec >> 1)) break;
            mate1_has_it = !(rj & 1) && hj == km;
        }
    }
    return !mate1_has_it;
}
__global__ __launch_bounds__(WALK_TPB) void a10_part_kernel(Occs o, uint8_t* __restrict__ part) {
    const uint32_t i = blockIdx.x * WALK_TPB + threadIdx.x;
    if (i >= o.n) return;
    const uint64_t rid = o.recs[i].rid;
    part[i] = walk_takes_part(o, i, o.hash[i], rid) ? 1 : 0;
    if (rid & RID_A10_BIT) o.recs[i].rid = rid & ~RID_A10_BIT;     // a mark the partitioned pass left before it was found unfit (a10_verdict)
}
// true: an earlier, closed filter holds the operation's reduced key
__device__ __forceinline__ bool in_closed_filters(const Filters& F, uint64_t h) {
    for (int q = 0; q + 1 < F.n; q++)
        if (table_first_op(F.f[q], reduced_key(F.f[q].geo, h)) < F.f[q].cut) return true;
    return false;
}
// 0: contained (an earlier operation of its class, or a closed filter);  1: this operation inserts into the current filter
__device__ __forceinline__ int op_inserts(const Filters& F, uint64_t h, uint64_t op) {
    if (in_closed_filters(F, h)) return 0;
    const Filter& cur = F.f[F.n - 1];
    return table_first_op(cur, reduced_key(cur.geo, h)) == op ? 1 : 0;
}
// f(op, item hash) for the operations of occurrence i from the phase's begin on -> its rid; 0: no such occurrence, or it takes no part
template <class Fn>
__device__ __forceinline__ uint64_t for_ops(const Occs& o, const Filters& F, uint32_t i, Fn&& f) {
    if (i >= o.n || !o.part[i]) return 0;
    const OccRec r = o.recs[i];
    for (uint32_t w = 0; w < 2; w++) {
        const uint64_t op = op_key(r.rid, w);
        if (op >= F.begin) f(op, item_hash(r.hash, w ? r.m1 : r.m0));
    }
    return r.rid;
}
__global__ __launch_bounds__(WALK_TPB) void a10_enter_kernel(Occs o, Filters F) {
    const Filter& cur = F.f[F.n - 1];
    for_ops(o, F, blockIdx.x * WALK_TPB + threadIdx.x, [&](uint64_t op, uint64_t h) {
        if (!in_closed_filters(F, h)) table_enter(cur, reduced_key(cur.geo, h), op);
    });
}
__global__ __launch_bounds__(WALK_TPB) void a10_flag_kernel(Occs o, Filters F) {
    const uint32_t i = blockIdx.x * WALK_TPB + threadIdx.x;
    bool contained = false;
    const uint64_t rid = for_ops(o, F, i, [&](uint64_t op, uint64_t h) { if (op < F.end && !op_inserts(F, h, op)) contained = true; });
    if (contained) o.recs[i].rid = rid | RID_A10_BIT;      // (the thread's own record; other threads read it through RID_MASK)
}
// inserting operations of the phase per tile of TILE_OCC occurrences
__global__ __launch_bounds__(WALK_TPB) void a10_count_kernel(Occs o, Filters F, uint32_t* __restrict__ tile_count) {
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t e = threadIdx.x; e < TILE_OCC; e += WALK_TPB)
        for_ops(o, F, blockIdx.x * TILE_OCC + e, [&](uint64_t op, uint64_t h) { mine += (uint32_t)op_inserts(F, h, op); });
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (threadIdx.x == 0) tile_count[blockIdx.x] = s_n;
}
// The operation that opens the next filter: the one with `rank` inserting operations of the phase before it, counted from the start of
// tile `tile`.  Tiles follow the dense arrays, which are in file order record by record but not inside a record (see op_key): the workgroup
// finds the occurrence that holds inserting operation `rank` in ARRAY order; the operation wanted is in the same record — the records before
// it hold the same inserting operations in either order — and one lane picks it among the record's inserting operations by their keys.
__global__ __launch_bounds__(WALK_TPB) void a10_find_kernel(Occs o, Filters F, uint32_t tile, uint32_t rank, unsigned long long* __restrict__ run_keys,
                                                            uint32_t run_cap, uint64_t* __restrict__ out_op) {
    constexpr uint32_t PER = TILE_OCC / WALK_TPB;
    __shared__ uint32_t s_cnt[WALK_TPB];
    uint32_t mine = 0;
    uint8_t ins[PER];          // inserting operations (0..2) of the lane's PER consecutive occurrences
    for (uint32_t e = 0; e < PER; e++) {
        ins[e] = 0;
        for_ops(o, F, tile * TILE_OCC + threadIdx.x * PER + e, [&](uint64_t op, uint64_t h) { ins[e] += (uint8_t)op_inserts(F, h, op); });
        mine += ins[e];
    }
    s_cnt[threadIdx.x] = mine;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t t = 0; t < threadIdx.x; t++) before += s_cnt[t];
    // one lane holds inserting operation `rank` in array order: it names the occurrence and its record's run of occurrences
    // [lo, hi) in the dense arrays (invalid entries in between belong to no record: skipped)
    __shared__ uint32_t s_run[3];                         // at, lo, hi
    __shared__ uint32_t s_t;                              // the record's inserting operations before number `rank` in array order
    if (rank >= before && rank < before + mine) {
        uint32_t at = 0, r = before;
        for (uint32_t e = 0; e < PER; e++) {
            if (rank < r + ins[e]) { at = tile * TILE_OCC + threadIdx.x * PER + e; break; }
            r += ins[e];
        }
        const uint64_t rec = o.recs[at].rid & RID_MASK;
        uint32_t lo = at, hi = at + 1;
        while (lo > 0 && (o.hash[lo - 1] == INVALID_HASH || (o.recs[lo - 1].rid & RID_MASK) == rec)) lo--;
        while (hi < o.n && (o.hash[hi] == INVALID_HASH || (o.recs[hi].rid & RID_MASK) == rec)) hi++;
        s_run[0] = at; s_run[1] = lo; s_run[2] = hi;
        s_t = rank - r;                                   // (those of `at` itself that come before number `rank`)
    }
    __syncthreads();
    const uint32_t at = s_run[0], lo = s_run[1], hi = s_run[2];
    // The operation wanted is the record's inserting operation with exactly t of the record's inserting operations before it BY
    // KEY, t = those before number `rank` in array order (the records in front hold the same inserting operations in either
    // order).  The record's keys go to a scratch array (a record of a long read pair at c = 1 has thousands).
    if (2 * (hi - lo) > run_cap) return;                  // (out_op stays unset: the host reports it)
    for (uint32_t i = lo + threadIdx.x; i < hi; i += WALK_TPB) {
        const OccRec r = o.recs[i];
        const bool part = o.part[i] != 0;
        for (uint32_t w = 0; w < 2; w++) {
            const uint64_t op = op_key(r.rid, w);
            const bool in = part && op >= F.begin && op_inserts(F, item_hash(r.hash, w ? r.m1 : r.m0), op);
            run_keys[2 * (i - lo) + w] = in ? op : NO_OP;
            if (in && i < at) atomicAdd(&s_t, 1u);
        }
    }
    __syncthreads();                                      // (one workgroup: its own global writes are visible to it behind the barrier)
    const uint32_t t = s_t, n_keys = 2 * (hi - lo);
    for (uint32_t e = threadIdx.x; e < n_keys; e += WALK_TPB) {
        const unsigned long long key = run_keys[e];
        if (key == NO_OP) continue;
        uint32_t smaller = 0;
        for (uint32_t q = 0; q < n_keys; q++) smaller += run_keys[q] < key ? 1u : 0u;
        if (smaller == t) *out_op = key;
    }
}

// Debug aids of the walk for tools/a10_debug.py / a10_dump.py (`make CXXFLAGS+=-DSYLPH_A10_DEBUG`).  SYLPH_HIP_A10_DUMP=<file>: the records
// the walk works on, <file>.table: the table of phase 0 as the enter kernel left it; SYLPH_HIP_A10_TRACE: a line per phase and cut on stderr.
#ifdef SYLPH_A10_DEBUG
// [0] occurrences taking part, [1] operations of the phase, [2] inserting, [3] first_op < op, [4] first_op > op
__global__ __launch_bounds__(WALK_TPB) void a10_debug_kernel(Occs o, Filters F, unsigned long long* __restrict__ out) {
    const Filter& cur = F.f[F.n - 1];
    if (for_ops(o, F, blockIdx.x * WALK_TPB + threadIdx.x, [&](uint64_t op, uint64_t h) {
            atomicAdd(&out[1], 1ull);
            const uint64_t fo = table_first_op(cur, reduced_key(cur.geo, h));
            atomicAdd(&out[fo == op ? 2 : (fo < op ? 3 : 4)], 1ull);
        })) atomicAdd(&out[0], 1ull);
}
void debug_entered(sylph_ctx* ctx, const Occs& o, const Filters& F, uint64_t slots, uint32_t grid) {
    const int j = F.n - 1;
    const char* dump = getenv("SYLPH_HIP_A10_DUMP");
    if (dump && j == 0) {       // (the records are still as a10_part_kernel left them: the flag kernel has not run)
        std::vector<OccRec> h(o.n);
        ctx->d2h(h.data(), o.recs, o.n * sizeof(OccRec));
        std::vector<uint64_t> hh(o.n);
        ctx->d2h(hh.data(), o.hash, (size_t)o.n * 8);
        if (FILE* f = fopen(dump, "wb")) { fwrite(hh.data(), 8, o.n, f); fwrite(h.data(), sizeof(OccRec), o.n, f); fclose(f); }
        std::vector<Ent> t(slots);
        ctx->d2h(t.data(), F.f[0].tab, slots * sizeof(Ent));
        if (FILE* f = fopen((std::string(dump) + ".table").c_str(), "wb")) { fwrite(t.data(), sizeof(Ent), slots, f); fclose(f); }
    }
    if (!getenv("SYLPH_HIP_A10_TRACE")) return;
    DevBuf dbg(ctx);
    dbg.reserve(64);
    SY_HIP(hipMemsetAsync(dbg.p, 0, 64, ctx->stream));
    hipLaunchKernelGGL(a10_debug_kernel, dim3(grid), dim3(WALK_TPB), 0, ctx->stream, o, F, dbg.as<unsigned long long>());
    unsigned long long hdbg[5];
    ctx->d2h(hdbg, dbg.p, 40);
    fprintf(stderr, "[sylph_hip] a10 phase %d: %llu occurrences take part, %llu operations, %llu inserting, %llu later than their class's first, %llu EARLIER than it\n",
            j, hdbg[0], hdbg[1], hdbg[2], hdbg[3], hdbg[4]);
}
void debug_cut(int j, uint64_t cap, FilterGeom geo, uint64_t cut, Cut at) {
    if (!getenv("SYLPH_HIP_A10_TRACE")) return;
    fprintf(stderr, "[sylph_hip] a10 phase %d: capacity %llu, %d fingerprint bits, %llu buckets; the next filter opens at record %llu, seed %llu, marker %llu (tile %u, %llu inserting operations before the tile)\n",
            j, (unsigned long long)cap, bit_length(geo.fp_mask), (unsigned long long)geo.nb_mask + 1, (unsigned long long)(cut >> 21),
            (unsigned long long)((cut >> 1) & RID_RANK_MAX), (unsigned long long)(cut & 1), at.tile, (unsigned long long)at.before);
}
#else
inline void debug_entered(sylph_ctx*, const Occs&, const Filters&, uint64_t, uint32_t) {}
inline void debug_cut(int, uint64_t, FilterGeom, uint64_t, Cut) {}
#endif

// ---- the partitioned pass (round 5): one filter, no device-wide atomics -------------------------------------------------------
// While the sample stays inside filter 0, "first operation of its class" needs no table: the operations are GROUPED by class (DESIGN.md §1,
// round 5).  One 8-byte word per operation (a10_plan.h op_word) goes through the coarse level of the replay's partition (partition.h) into
// ~8,000-operation ranges of equal class-hash width; the workgroups of a range find the words that share their upper half with another
// word, and only those fetch their record and set RID_A10_BIT where they are not the earliest of their class.  Skipped mate-2 occurrences
// (sketch.rs:852) take part although the walk never sees them: their items are those of the mate-1 occurrence of the same k-mer in the
// same pair, which precedes them.  The pass cannot tell by itself that one filter was enough: it leaves {workgroups too full, operations
// found} in two device words for the caller's tail block (a10_verdict).
struct OpsIn { const uint64_t* hash; const OccRec* recs; const uint32_t* blk_count; uint32_t n_dense, n_blk, slot_cap; };
__device__ __forceinline__ ulonglong2 op_words(FilterGeom d, const OccRec& r, bool valid, uint32_t slot) {
    if (!valid || !(r.rid & RID_MARKER_BIT)) return make_ulonglong2(INVALID_HASH, INVALID_HASH);
    return make_ulonglong2(op_word(d, r.hash, r.m0, 2u * slot), op_word(d, r.hash, r.m1, 2u * slot + 1u));
}
// ops[2 * slot + w] for every occurrence in the slots of the session's one batch, a partition TILE of the slots (blk_per_tile blocks of the
// seeding kernel) per workgroup, counting the words per class range on the way: hist[c * n_tiles + t] is what part_hist_kernel would find in
// a pass of its own over the 64 MB of words (round 6; eight groups of 32 lanes walk eight blocks at a time, as partition.h's for_tile_entries)
__global__ __launch_bounds__(PART_TPB) void a10_ops_tile_kernel(OpsIn in, FilterGeom d, uint32_t blk_per_tile, BucketMap bm, uint32_t n_tiles, ulonglong2* __restrict__ ops,
                                                                uint32_t* __restrict__ hist, uint32_t* __restrict__ tail) {
    __shared__ uint32_t s_h[MAX_COARSE];
    if (blockIdx.x == 0 && threadIdx.x < 2) tail[threadIdx.x] = 0;
    const uint32_t t = xcd_tile(n_tiles), C = bm.B;
    if (t >= n_tiles) return;
    for (uint32_t c = threadIdx.x; c < C; c += PART_TPB) s_h[c] = 0;
    __syncthreads();
    const uint32_t grp = threadIdx.x >> 5, l = threadIdx.x & 31;
    for (uint32_t bl = grp; bl < blk_per_tile; bl += PART_TPB / 32) {
        const uint32_t b = t * blk_per_tile + bl;
        if (b >= in.n_blk) break;
        const uint32_t cnt = min(in.blk_count[b], in.slot_cap), g0 = b * in.slot_cap;
        for (uint32_t i = l; i < cnt; i += 32) {
            const ulonglong2 w = op_words(d, in.recs[g0 + i], true, g0 + i);
            ops[g0 + i] = w;
            if (w.x != INVALID_HASH) {
                atomicAdd(&s_h[bucket_of_key((uint32_t)(w.x >> 32), bm)], 1u);
                atomicAdd(&s_h[bucket_of_key((uint32_t)(w.y >> 32), bm)], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < C; c += PART_TPB) hist[(size_t)c * n_tiles + t] = s_h[c];
}
// ... and for the dense arrays (the partition counts the words itself)
__global__ __launch_bounds__(256) void a10_ops_dense_kernel(OpsIn in, FilterGeom d, ulonglong2* __restrict__ ops, uint32_t* __restrict__ tail) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < 2) tail[i] = 0;
    if (i >= in.n_dense) return;
    ops[i] = op_words(d, in.recs[i], in.hash[i] != INVALID_HASH, i);
}

// ---- one partition level (round 6) ------------------------------------------------------------------------------------------
// The words stay where part_scatter left them, grouped by range, and the ones that share their upper half with another are found WITHOUT
// sorting them, by the steps below (the arithmetic and a sequential model of the steps: a10_plan.h, tests/a10_plan_capi.cpp).
// `split` workgroups share a range, each keeping the words whose slot falls into its 2^17 slots — twice the reads, from L2, for half the
// LDS: beside the next samples' seeding kernels the footprint decides, not the kernel's time alone (profiles/r06_ab_a10.txt).
#define SY_LDS __attribute__((address_space(3)))
struct RangeLds {
    SY_LDS uint32_t* bits;                      // [RNG_SLOTS / 32] one bit per slot of the workgroup's part
    SY_LDS unsigned long long *t_key, *t_min;   // [RNG_TAB] class keys (~0: free) | [RNG_TAB] earliest place of the class         (over bits)
    SY_LDS uint32_t *sec, *up, *list;           // [RNG_CAND] second arrivals' residues; [RNG_TAB] upper-half set (RNG_FREE: free); [RNG_CAND] candidates' operation ids
    SY_LDS uint32_t* n;                         // second arrivals, candidates
};
__device__ __forceinline__ RangeLds range_lds() {
    __shared__ __attribute__((aligned(16))) uint32_t s_bits[RNG_SLOTS / 32];
    __shared__ uint32_t s_sec[RNG_CAND], s_up[RNG_TAB], s_list[RNG_CAND], s_n[2];
    using W = SY_LDS uint32_t*; using D = SY_LDS unsigned long long*;
    return RangeLds{(W)s_bits, (D)s_bits, (D)s_bits + RNG_TAB, (W)s_sec, (W)s_up, (W)s_list, (W)s_n};      // (a10_plan.h: the class table fits over the bits)
}
// the words [lo, hi) of a range, as the workgroup `part` of the range's geo.split sees them during slice p of P
struct RangePart { const uint64_t* words; uint32_t lo, hi, lo_key, part; RangeGeom geo; uint32_t P, p; };

// appends v to list[0 .. RNG_CAND) behind *counter: one returning LDS atomic for the few lanes that take (3-7 % of them: a ballot +
// prefix count per visit, for every lane, was a third of the kernel's 45 VALU + 48 SALU instructions per word visited)
__device__ __forceinline__ void append(bool take, uint32_t v, SY_LDS uint32_t* list, SY_LDS uint32_t* counter) {
    if (take) {
        const uint32_t at = atomicAdd((uint32_t*)counter, 1u);
        if (at < RNG_CAND) list[at] = v;
    }
}
// body(valid, word) for every word of the range, U loads in flight per lane
template <class F>
__device__ __forceinline__ void for_words(const RangePart& r, F&& body) {
    constexpr uint32_t U = 4;
    const uint32_t tid = threadIdx.x;
    for (uint32_t e0 = r.lo; e0 < r.hi; e0 += U * RNG_TPB) {
        uint64_t w[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) { const uint32_t e = e0 + u * RNG_TPB + tid; w[u] = e < r.hi ? r.words[e] : 0ull; }
#pragma unroll
        for (uint32_t u = 0; u < U; u++) body(e0 + u * RNG_TPB + tid < r.hi, w[u]);
    }
}
// slot of a word in this workgroup's table, or RNG_FREE: another workgroup's (or another slice's) word
__device__ __forceinline__ uint32_t my_slot(const RangePart& r, uint32_t res) {
    const RangeSlot s = range_slot(res, r.geo);
    if (s.part != r.part) return RNG_FREE;
    return (r.P == 1 || slice_of(s.local, r.P) == r.p) ? s.local : RNG_FREE;
}
// every word sets its slot's bit; one that finds it set is a SECOND ARRIVAL (every duplicate but one of each group, and by chance 1.5 % of
// the rest), listed in s.sec -> their number
__device__ __forceinline__ uint32_t mark_arrivals(const RangeLds& s, const RangePart& r) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < RNG_SLOTS / 32; i += RNG_TPB) s.bits[i] = 0;
    for (uint32_t i = tid; i < RNG_TAB; i += RNG_TPB) s.up[i] = RNG_FREE;
    if (tid < 2) s.n[tid] = 0;
    __syncthreads();
    for_words(r, [&](bool valid, uint64_t w) {
        bool second = false;
        const uint32_t res = range_residue(w, r.lo_key);
        if (valid) {
            const uint32_t l = my_slot(r, res);
            if (l != RNG_FREE) {
                const uint32_t bit = 1u << (l & 31u);
                second = atomicOr((uint32_t*)&s.bits[l >> 5], bit) & bit;
            }
        }
        append(second, res, s.sec, &s.n[0]);
    });
    __syncthreads();
    return s.n[0];
}
// their upper halves go into a small open-addressing set
__device__ __forceinline__ void build_upper_set(const RangeLds& s, uint32_t n_sec) {
    for (uint32_t i = threadIdx.x; i < n_sec; i += RNG_TPB) {
        const uint32_t res = s.sec[i];
        uint32_t at = up_home(res);
        for (;;) {
            const uint32_t old = atomicCAS((uint32_t*)&s.up[at], RNG_FREE, res);
            if (old == RNG_FREE || old == res) break;
            at = tab_next(at);
        }
    }
    __syncthreads();
}
// every word asks the set for its upper half: the ones found (true duplicates, the filter's cross-item collisions, chance arrivals: ~7 %)
// are the candidates, listed in s.list -> their number
__device__ __forceinline__ uint32_t list_candidates(const RangeLds& s, const RangePart& r) {
    for_words(r, [&](bool valid, uint64_t w) {
        bool cand = false;
        if (valid) {
            const uint32_t res = range_residue(w, r.lo_key);
            if (my_slot(r, res) != RNG_FREE) {
                uint32_t at = up_home(res);
                for (;;) {
                    const uint32_t v = s.up[at];
                    if (v == res) { cand = true; break; }
                    if (v == RNG_FREE) break;
                    at = tab_next(at);
                }
            }
        }
        append(cand, (uint32_t)w, s.list, &s.n[1]);
    });
    __syncthreads();
    return s.n[1];
}
constexpr int RNG_Q = RNG_CAND / RNG_TPB;      // candidates fetch their record and meet in the table of {class key, earliest place in the walk}
struct Cands { uint64_t key[RNG_Q]; uint32_t opid[RNG_Q], at[RNG_Q]; };
__device__ __forceinline__ void resolve_classes(const RangeLds& s, FilterGeom d, const OccRec* __restrict__ recs, uint32_t nc, Cands& k) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < RNG_TAB; i += RNG_TPB) { s.t_key[i] = ~0ull; s.t_min[i] = ~0ull; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < RNG_Q; q++) {
        const uint32_t i = tid + q * RNG_TPB;
        k.key[q] = 0; k.opid[q] = 0; k.at[q] = 0;
        if (i < nc) {
            k.opid[q] = s.list[i];
            const OccRec r = recs[k.opid[q] >> 1];
            const uint64_t g = reduced_key(d, item_hash(r.hash, (k.opid[q] & 1u) ? r.m1 : r.m0));      // < 2^63: never the ~0 of a free entry
            k.key[q] = op_key(r.rid, k.opid[q] & 1u);
            k.at[q] = class_home(g);
            for (;;) {
                const unsigned long long old = atomicCAS((unsigned long long*)&s.t_key[k.at[q]], ~0ull, (unsigned long long)g);
                if (old == ~0ull || old == g) break;
                k.at[q] = tab_next(k.at[q]);
            }
            atomicMin((unsigned long long*)&s.t_min[k.at[q]], (unsigned long long)k.key[q]);
        }
    }
    __syncthreads();
}
// (both operations of an occurrence may be contained, from two workgroups: the OR commutes; this kernel reads the rid's record and rank only)
__device__ __forceinline__ void set_marks(const RangeLds& s, OccRec* __restrict__ recs, uint32_t nc, const Cands& k) {
#pragma unroll
    for (int q = 0; q < RNG_Q; q++)
        if (threadIdx.x + q * RNG_TPB < nc && s.t_min[k.at[q]] < k.key[q])
            atomicOr(reinterpret_cast<uint32_t*>(&recs[k.opid[q] >> 1].rid) + 1, (uint32_t)(RID_A10_BIT >> 32));
    __syncthreads();
}
#undef SY_LDS

__global__ __launch_bounds__(RNG_TPB) void a10_range_kernel(const uint64_t* __restrict__ words, const uint32_t* __restrict__ cbase, uint32_t B, RangeGeom geo, FilterGeom d,
                                                            OccRec* __restrict__ recs, uint32_t* __restrict__ tail) {
    const RangeLds s = range_lds();
    const RangeBlock blk = range_of_block(blockIdx.x, geo.split);
    if (blockIdx.x == 0 && threadIdx.x == 0) tail[1] = cbase[B];      // operations found
    if (blk.c >= B) return;                                           // (padding of the grid)
    RangePart r{words, cbase[blk.c], cbase[blk.c + 1], range_lo_key(blk.c, B), blk.part, geo, 1u, 0u};
    if (r.hi == r.lo) return;
    while (r.p < r.P) {
        const uint32_t n_sec = mark_arrivals(s, r);
        uint32_t n_over = n_sec * 2u;                                 // (what the candidates' list would have to take, at least)
        bool over = n_sec > RNG_CAND;
        if (!over) {
            build_upper_set(s, n_sec);
            n_over = list_candidates(s, r);
            over = n_over > RNG_CAND;
        }
        if (over) {      // narrower slices, from the top (marks set so far are set again: the OR is idempotent) — or the verdict
            r.P = next_slices(r.P, n_over);
            if (!r.P) { if (threadIdx.x == 0) atomicAdd(&tail[0], 1u); return; }
            r.p = 0;
            __syncthreads();
            continue;
        }
        Cands k;
        resolve_classes(s, d, recs, n_over, k);
        set_marks(s, recs, n_over, k);
        r.p++;
    }
}

FilterGeom filter_geometry_of(const sylph_sketch* sk, int j) {
    FilterGeom g;
    const uint64_t refused = filter_geometry(sk->dedup_capacity, sk->dedup_fpr, j, &g);
    SY_REQUIRE(!refused, "filter of %llu buckets", (unsigned long long)refused);
    return g;
}

}  // namespace

// The partitioned pass over the session's occurrences where they lie (slots of its one batch, or the dense arrays).
static void a10_mark_partitioned(sylph_sketch* sk) {
    sylph_ctx* ctx = sk->ctx;
    const Occurrences occ = sk->occurrences();
    const bool slotted = occ.slotted();
    HostPhase ph(ctx, "finish: a10 filter marks (partitioned)");
    sk->a10_tail.reserve(16);
    uint32_t* tail = sk->a10_tail.as<uint32_t>();
    DevBuf b_ops(ctx), b_pairs(ctx), b_hist(ctx);
    b_ops.reserve(occ.n_slots * 16);
    b_pairs.reserve(occ.n_slots * 16);
    const FilterGeom f0 = filter_geometry_of(sk, 0);
    const BucketMap bm = class_map(occ.n_expect, RNG_WORDS);       // equal ranges of the words' upper 32 bits, ~RNG_WORDS operations each
    const uint32_t B = bm.B;
    OpsIn oin{};
    PartIn in{};
    in.key_sh = bm.sh;
    in.carry = 1;
    uint32_t n_tiles;
    if (slotted) {
        const uint32_t* blk_count = slot_meta_of(sk, sk->pend.n_blk).blk_count;
        oin.recs = sk->slot_rec.as<OccRec>(); oin.blk_count = blk_count; oin.n_blk = sk->pend.n_blk; oin.slot_cap = sk->pend.slot_cap;
        in.slotted = 2; in.blk_count = blk_count; in.n_blk = sk->pend.n_blk; in.slot_cap = sk->pend.slot_cap; in.blk_per_tile = OPS_BLK_PER_TILE;
        n_tiles = (in.n_blk + OPS_BLK_PER_TILE - 1) / OPS_BLK_PER_TILE;
    } else {
        oin.hash = sk->hash.as<uint64_t>(); oin.recs = sk->recs.as<OccRec>(); oin.n_dense = (uint32_t)sk->n_occ;
        in.slotted = 0; in.n_dense = (uint32_t)(2 * sk->n_occ);
        in.tile_entries = (uint32_t)std::max<uint64_t>(4096, (2 * sk->n_occ + 65535) / 65536);
        n_tiles = (uint32_t)((2 * sk->n_occ + in.tile_entries - 1) / in.tile_entries);
    }
    in.hash = b_ops.as<uint64_t>();
    b_hist.reserve(part_hist_words(PartGeom{0, B}, n_tiles) * 4);
    ScopedKernelTimer t(ctx, "a10");
    if (slotted)      // (from slots, the operation words' kernel also counts them per (range, tile))
        hipLaunchKernelGGL(a10_ops_tile_kernel, dim3(((n_tiles + 7) / 8) * 8), dim3(PART_TPB), 0, ctx->stream, oin, f0, in.blk_per_tile, bm, n_tiles, b_ops.as<ulonglong2>(),
                           b_hist.as<uint32_t>(), tail);
    else hipLaunchKernelGGL(a10_ops_dense_kernel, dim3((uint32_t)((sk->n_occ + 255) / 256)), dim3(256), 0, ctx->stream, oin, f0, b_ops.as<ulonglong2>(), tail);
    launch_partition_coarse(ctx, in, bm, n_tiles, b_hist.as<uint32_t>(), b_pairs.as<uint2>(), slotted);      // words grouped by range where the scatter leaves them
    static const int env_split = [] { const char* e = getenv("SYLPH_HIP_A10_RANGE_SPLIT"); return e ? std::max(1, std::min((int)MAX_SPLIT, atoi(e))) : 2; }();
    static const int env_pad = [] { const char* e = getenv("SYLPH_HIP_A10_RANGE_LDS_PAD"); return e ? atoi(e) : 0; }();     // (A/B: LDS footprint)
    const RangeGeom geo = range_geometry(B, (uint32_t)env_split);
    hipLaunchKernelGGL(a10_range_kernel, dim3(range_grid(B, geo.split)), dim3(RNG_TPB), (size_t)env_pad, ctx->stream, b_pairs.as<uint64_t>(),
                       part_cbase(b_hist.as<uint32_t>(), B, n_tiles), B, geo, f0, const_cast<OccRec*>(oin.recs), tail);
    SY_HIP(hipGetLastError());
    sk->a10_marks = FilterMarks::Unread;
    if (ctx->profile) ctx->stats["a10_part"].launches++;              // (tests ask sylph_ctx_kernel_stats which pass ran)
    // (the buffers go back to the pool here; stream order keeps them alive for the kernels queued above)
}

// Marks (RID_A10_BIT) every occurrence of a paired session for which sketch.rs:747 / :754 would have found its (k-mer, markers)
// in the filter.  Works on the dense file-order arrays: occurrences still in their slots are compacted first.
static void a10_mark_walk(sylph_sketch* sk) {
    sylph_ctx* ctx = sk->ctx;
    flush_pending_slots(sk);
    sk->a10_marks = FilterMarks::Settled;
    const uint64_t n = sk->n_occ;
    if (!n) return;
    SY_REQUIRE(n < (1ull << 32), "more than 2^32-1 seed occurrences in one sample");
    HostPhase ph(ctx, "finish: a10 filter marks");
    DevBuf b_part(ctx), b_run(ctx), b_tiles(ctx);
    b_part.reserve(n);
    Occs o{sk->hash.as<uint64_t>(), sk->recs.as<OccRec>(), (uint32_t)n, b_part.as<uint8_t>()};
    const uint32_t grid = (uint32_t)((n + WALK_TPB - 1) / WALK_TPB), n_tiles = (uint32_t)((n + TILE_OCC - 1) / TILE_OCC);
    {
        ScopedKernelTimer t(ctx, "a10");
        hipLaunchKernelGGL(a10_part_kernel, dim3(grid), dim3(WALK_TPB), 0, ctx->stream, o, b_part.as<uint8_t>());
        SY_HIP(hipGetLastError());
    }
    const uint64_t n_ops = 2 * n;                 // an upper bound of the operations (occurrences that take part x 2)
    uint64_t ops_before = 0;                      // ... and of those before the current phase: every closed filter took its capacity
    std::vector<std::unique_ptr<DevBuf>> tables;
    Filters F{};
    F.begin = 0;
    for (int j = 0;; j++) {
        SY_REQUIRE(j < MAX_FILTERS, "the approximate dedup would need more than %d filters: raise dedup_capacity", MAX_FILTERS);
        const uint64_t cap = sk->dedup_capacity << j;
        // the phase's table: every operation behind the cut may enter it
        const uint64_t remaining = n_ops - std::min(n_ops, ops_before);
        const TableGeom tg = table_geometry(remaining);
        tables.emplace_back(new DevBuf(ctx));
        tables.back()->reserve(tg.slots * sizeof(Ent));
        F.f[j] = Filter{tables.back()->as<Ent>(), tg.tab_shift, (uint32_t)(tg.slots - 1), filter_geometry_of(sk, j), NO_OP};
        F.n = j + 1;
        F.end = NO_OP;
        ScopedKernelTimer t(ctx, "a10");
        SY_HIP(hipMemsetAsync(tables.back()->p, 0, tg.slots * sizeof(Ent), ctx->stream));
        hipLaunchKernelGGL(a10_enter_kernel, dim3(grid), dim3(WALK_TPB), 0, ctx->stream, o, F);
        debug_entered(ctx, o, F, tg.slots, grid);
        bool last = remaining <= cap;            // not even every remaining operation inserting would fill the filter
        if (!last) {                             // count per tile, cut search on the host, the operation inside the tile
            b_tiles.reserve(((size_t)n_tiles + 2) * 4 + 16);
            hipLaunchKernelGGL(a10_count_kernel, dim3(n_tiles), dim3(WALK_TPB), 0, ctx->stream, o, F, b_tiles.as<uint32_t>());
            SY_HIP(hipGetLastError());
            std::vector<uint32_t> h_tiles(n_tiles);
            ctx->d2h(h_tiles.data(), b_tiles.p, (size_t)n_tiles * 4);
            const Cut at = cut_tile(h_tiles.data(), n_tiles, cap);
            last = at.tile == n_tiles;
            if (!last) {
                uint64_t* d_cut = reinterpret_cast<uint64_t*>(b_tiles.as<uint32_t>() + ((n_tiles + 1) & ~1u));
                SY_HIP(hipMemsetAsync(d_cut, 0xFF, 8, ctx->stream));
                const uint32_t run_cap = (uint32_t)std::min<uint64_t>(2 * n, 1u << 22);     // operations of ONE record the cut can be looked for in
                b_run.reserve((size_t)run_cap * 8);
                hipLaunchKernelGGL(a10_find_kernel, dim3(1), dim3(WALK_TPB), 0, ctx->stream, o, F, at.tile, (uint32_t)(cap - at.before), b_run.as<unsigned long long>(), run_cap, d_cut);
                SY_HIP(hipGetLastError());
                uint64_t cut = 0;
                ctx->read_back(&cut, d_cut, 8);
                SY_REQUIRE(cut != NO_OP && cut > F.begin, "internal: the operation that opens filter %d was not found", j + 1);
                debug_cut(j, cap, F.f[j].geo, cut, at);
                F.f[j].cut = F.end = cut;
                ops_before += cap;
            }
        }
        hipLaunchKernelGGL(a10_flag_kernel, dim3(grid), dim3(WALK_TPB), 0, ctx->stream, o, F);
        SY_HIP(hipGetLastError());
        if (last) break;
        F.begin = F.end;
    }
    // (the tables go back to the pool here; stream order keeps them alive for the kernels queued above)
}

// Which pass (a10_plan.h fits): the partitioned one where the first filter takes every operation, the phase walk for samples that make it grow.
void a10_mark(sylph_sketch* sk) {
    if (!sk->filter_dedup() || sk->a10_marks != FilterMarks::None) return;
    SY_REQUIRE(sk->dedup_capacity >= 1 && sk->dedup_capacity < (1ull << 31), "dedup_capacity out of range");
    const Occurrences occ = sk->occurrences();
    if (occ.n_slots == 0) { sk->a10_marks = FilterMarks::Settled; return; }
    if (sk->a10_force != 1 && fits(occ.n_slots, occ.n_expect_filter, occ.n_plain, sk->dedup_capacity)) a10_mark_partitioned(sk);
    else a10_mark_walk(sk);
}

// The verdict words of the partitioned pass, read by the caller with its own tail or on their own: false = the marks are no good (a10_plan.h
// verdict_good) and stay unaccepted: the finish loop sends the sample through the walk (a10_remark_walk).  Good marks are accepted here.
bool a10_verdict(sylph_sketch* sk, const uint32_t words[2]) {
    if (sk->a10_marks != FilterMarks::Unread) return true;
    if (!verdict_good(words[0], words[1], sk->dedup_capacity)) return false;
    sk->a10_marks = FilterMarks::Settled;
    return true;
}

// ... and the phase walk marks the records again — on the dense arrays: whoever partitioned the slots starts over.
void a10_remark_walk(sylph_sketch* sk) {
    if (sk->ctx->profile) sk->ctx->stats["a10_redo"].launches++;       // (tests ask sylph_ctx_kernel_stats whether this road was taken)
    a10_mark_walk(sk);
}

}  // namespace sylph
