// replay_generic.hip — the device-wide K3: replay of dup_removal_lsh_full_exact (sketch.rs:690-731) as data-parallel segment kernels
// over a stable radix sort of the occurrences by hash -> (k-mer, count) table in ascending k-mer order.  The correctness fallback of
// the dedup tail: finish = generic, c < 2, and every bucket that outgrows LDS (replay_lds.hip).
//
// Replay formulation.  For one k-mer, let its occurrences in file order be i = 0..n-1, each with
// an optional marker pair (m0_i, m1_i) (pair_kmer_single sketch.rs:625 / pair_kmer :659).  Every occurrence that
// reaches the marker test inserts both of its markers, whether it is then counted or dropped (:709-722), so
//     dropped_i  <=>  has_marker_i  AND  i is not the first processed occurrence (count > 0, :711,:718)
//                     AND ( m0_i == m1_i  OR  {m0_i, m1_i} meets {m0_j, m1_j} for some processed j < i with a marker )
// which needs no sequential state.  The single-end cut-off (`count < 4`, :706,:937) only makes a suffix of the
// occurrences unconditional, handled by one short walk per k-mer.  Mate-2 occurrences whose hash also occurs in
// mate 1 of the same pair are removed first (sketch.rs:852).
#include <algorithm>
#include <cstddef>

#include "common.h"
#include "device_common.h"
#include "sketch_session.h"

namespace sylph {
namespace {

// number of valid occurrences = first index holding INVALID_HASH in the hash-sorted array (one lane, log n loads)
__global__ void count_valid_kernel(const uint64_t* __restrict__ hs, uint32_t n, uint32_t* __restrict__ out) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (hs[mid] < INVALID_HASH) lo = mid + 1; else hi = mid;
    }
    *out = lo;
}

__global__ void iota_kernel(uint32_t* v, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}

// gather payload into hash-sorted order and mark segment heads
__global__ __launch_bounds__(256) void gather_heads_kernel(const uint64_t* __restrict__ hs, const uint32_t* __restrict__ perm, const OccRec* __restrict__ recs,
                                                           uint32_t n, uint64_t* __restrict__ rid_s, uint64_t* __restrict__ m0_s, uint64_t* __restrict__ m1_s,
                                                           uint32_t* __restrict__ head, uint32_t* __restrict__ headidx) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = perm[i];
    const OccRec r = recs[p];
    rid_s[i] = r.rid;
    m0_s[i] = r.m0;
    m1_s[i] = r.m1;
    const bool hd = (i == 0) || (hs[i] != hs[i - 1]);
    head[i] = hd ? 1u : 0u;
    headidx[i] = hd ? i : 0u;
}

// K3a: mate-2 skip rule (sketch.rs:852): a mate-2 occurrence is not processed at all if the same hash was
// produced by mate 1 of the same pair.  Occurrences are in file order inside a segment, so the pair's mate-1
// occurrences sit immediately before its mate-2 occurrences.
__global__ __launch_bounds__(256) void skip_kernel(const uint64_t* __restrict__ rid_s, const uint32_t* __restrict__ seg_start, uint32_t n,
                                                   uint8_t* __restrict__ skip, unsigned int* __restrict__ n_skipped) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t rec = i < n ? (rid_s[i] & RID_MASK) : 0;
    uint8_t s = 0;
    if (rec & 1) {
        const uint32_t s0 = seg_start[i];
        for (uint32_t j = i; j > s0;) {
            j--;
            const uint64_t rj = rid_s[j] & RID_MASK;
            if ((rj >> 1) != (rec >> 1)) break;
            if ((rj & 1) == 0) { s = 1; break; }
        }
    }
    if (i < n) skip[i] = s;
    wave_count_add(n_skipped, s != 0);
}

// K3b: dropped_i as defined in the file header, computed by SORTING instead of scanning: an occurrence is dropped iff it is
// not the first processed occurrence of its k-mer and (m0 == m1, or one of its two markers was already inserted by an earlier
// processed occurrence of the same k-mer).  "Already inserted" = the (k-mer segment, marker value) pair has an entry with a
// smaller occurrence index.  Every processed occurrence with a marker contributes two entries e = 2 i + w (w: m0 / m1);
// entries are ordered by (segment, value, e) with two stable radix sorts (by value, then by segment) and every entry whose
// predecessor carries the same (segment, value) marks its occurrence as a hit.  O(n log n) whatever the coverage: the earlier
// formulation scanned all previous occurrences of the k-mer (quadratic for a k-mer with thousands of distinct reads).
__global__ __launch_bounds__(256) void marker_entries_kernel(const uint64_t* __restrict__ rid_s, const uint64_t* __restrict__ m0_s, const uint64_t* __restrict__ m1_s,
                                                             const uint8_t* __restrict__ skip, uint32_t n, uint64_t* __restrict__ key, uint32_t* __restrict__ ent) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * n) return;
    const uint32_t i = e >> 1;
    key[e] = (e & 1) ? m1_s[i] : m0_s[i];
    ent[e] = e;
}
// segment key of an entry: the index of the first occurrence of its k-mer, or n (behind every real segment) for entries of
// occurrences that insert no marker (skipped mate 2, sketch.rs:852; records without marker, :627,:661)
__global__ __launch_bounds__(256) void marker_segkey_kernel(const uint32_t* __restrict__ ent, const uint64_t* __restrict__ rid_s, const uint32_t* __restrict__ seg_start,
                                                            const uint8_t* __restrict__ skip, uint32_t n, uint32_t* __restrict__ segkey) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= 2 * n) return;
    const uint32_t i = ent[p] >> 1;
    const bool inserts = (rid_s[i] & RID_MARKER_BIT) && !(skip && skip[i]);
    segkey[p] = inserts ? seg_start[i] : n;
}
__global__ __launch_bounds__(256) void marker_hits_kernel(const uint32_t* __restrict__ ent, const uint32_t* __restrict__ segkey, const uint64_t* __restrict__ m0_s,
                                                          const uint64_t* __restrict__ m1_s, uint32_t n, uint8_t* __restrict__ hit) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0 || p >= 2 * n) return;
    const uint32_t sk = segkey[p];
    if (sk == n || segkey[p - 1] != sk) return;
    const uint32_t e = ent[p], f = ent[p - 1];
    const uint64_t v = (e & 1) ? m1_s[e >> 1] : m0_s[e >> 1], w = (f & 1) ? m1_s[f >> 1] : m0_s[f >> 1];
    if (v == w) hit[e >> 1] = 1;   // (f >> 1 == e >> 1 only when m0 == m1, which drops the occurrence anyway)
}
// DEDUP_FILTER: hit = the bit a10_mark left in the occurrence's record
__global__ __launch_bounds__(256) void filter_hits_kernel(const uint64_t* __restrict__ rid_s, uint32_t n, uint8_t* __restrict__ hit) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) hit[i] = (rid_s[i] & RID_A10_BIT) ? 1 : 0;
}
// flags[i]: bit0 = skip, bit1 = would-be-dropped.  Eproc = exclusive count of processed (non-skipped) occurrences.
__global__ __launch_bounds__(256) void dup_flags_kernel(const uint64_t* __restrict__ rid_s, const uint64_t* __restrict__ m0_s, const uint64_t* __restrict__ m1_s,
                                                        const uint32_t* __restrict__ seg_start, const uint8_t* __restrict__ skip, const uint32_t* __restrict__ Eproc,
                                                        const uint8_t* __restrict__ hit, uint32_t n, int filter, uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t fl = skip ? skip[i] : 0;
    if (!fl && (rid_s[i] & RID_MARKER_BIT)) {
        const uint32_t s0 = seg_start[i];
        bool any_prev = skip ? (Eproc[i] != Eproc[s0]) : (i != s0);
        if (filter && hit[i]) {
            // `*c > 0` (sketch.rs:749, :756) in the order of the WALK: a record's seeds go through the dedup in emission order (rank bits
            // of the rid), the sorted segment lists them by position — the first of the walk is the lowest rank among the segment's
            // leading occurrences of the head's record (replay_lds.hip walk_first)
            const uint64_t rec0 = rid_s[s0] & RID_MASK, ri = rid_s[i];
            any_prev = true;
            if ((ri & RID_MASK) == rec0) {
                any_prev = false;
                const uint64_t rank_i = (ri >> RID_RANK_SHIFT) & RID_RANK_MAX;
                for (uint32_t q = s0; q < n && seg_start[q] == s0 && (rid_s[q] & RID_MASK) == rec0; q++)
                    if (q != i && ((rid_s[q] >> RID_RANK_SHIFT) & RID_RANK_MAX) < rank_i) { any_prev = true; break; }
            }
        }
        // (filter mode: equal markers are the filter's business too — its second test finds what the first inserted)
        if (any_prev && (hit[i] || (!filter && m0_s[i] == m1_s[i]))) fl |= 2;
    }
    flags[i] = fl;
}
__global__ __launch_bounds__(256) void processed_kernel(const uint8_t* __restrict__ skip, uint32_t n, uint32_t* __restrict__ u) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) u[i] = (i < n && !skip[i]) ? 1u : 0u;
}

// K3c.  With u_i = 1 if occurrence i would be counted were there no cut-off (processed and not dropped) and
// P_i = number of such occurrences before i inside its k-mer (a segmented exclusive prefix sum), the reference's
// walk (sketch.rs:701-730) reduces to:  counted_i = (cutoff && P_i >= cutoff) ? 1 : u_i   (once the count has
// reached MAX_DEDUP_COUNT nothing is ever dropped again, :706), removed_i = processed_i && !counted_i.
__global__ __launch_bounds__(256) void would_count_kernel(const uint8_t* __restrict__ flags, uint32_t n, int no_dedup,
                                                          uint32_t* __restrict__ u) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) { u[i] = 0; return; }   // sentinel so the exclusive scan has n+1 entries
    const uint8_t fl = flags[i];
    u[i] = (fl & 1) ? 0u : ((no_dedup || !(fl & 2)) ? 1u : 0u);
}

__global__ __launch_bounds__(256) void counted_kernel(const uint8_t* __restrict__ flags, const uint32_t* __restrict__ Eu, const uint32_t* __restrict__ seg_start,
                                                      uint32_t n, int no_dedup, uint32_t cutoff, uint32_t* __restrict__ counted) {
    // removed occurrences = processed - counted, taken from the scan total on the host side (no atomics here)
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const uint8_t fl = flags[i];
        uint32_t c = 0;
        if (!(fl & 1)) {
            const uint32_t P = Eu[i] - Eu[seg_start[i]];
            const bool u = no_dedup || !(fl & 2);
            c = (cutoff && P >= cutoff) ? 1u : (u ? 1u : 0u);
        }
        counted[i] = c;
    } else if (i == n) {
        counted[i] = 0;
    }
}

// start[s] = index of the first occurrence of k-mer s (start[n_seg] = n)
__global__ __launch_bounds__(256) void seg_starts_kernel(const uint32_t* __restrict__ head, const uint32_t* __restrict__ seg_id,
                                                         uint32_t n, uint32_t n_seg, uint32_t* __restrict__ start) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && head[i]) start[seg_id[i]] = i;
    if (i == 0) start[n_seg] = n;
}

__global__ __launch_bounds__(256) void emit_table_kernel(const uint64_t* __restrict__ hs, const uint32_t* __restrict__ start, const uint32_t* __restrict__ Ec,
                                                         uint32_t n_seg, uint64_t* __restrict__ out_k, uint32_t* __restrict__ out_c) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    const uint32_t a = start[s], b = start[s + 1];
    out_k[s] = hs[a];
    out_c[s] = Ec[b] - Ec[a];
}

// The steps of the device-wide replay, in the order generic_replay runs them, and the buffers they hand on.  (Buffers come from the ctx
// pool, not from ctx->scratch: the bucket path calls this for the occurrences of its overflowing buckets while its own scratch arrays
// are still live.)
struct GenericReplay {
    sylph_ctx* ctx;
    hipStream_t s;
    const bool paired, no_dedup, filter;
    uint32_t nv = 0;                       // valid occurrences: the front of the hash-sorted order
    size_t nv1 = 0, ne = 0;                // nv + 1 (the scanned arrays carry a sentinel); 2 nv (marker entries: two per occurrence)
    DevBuf b_idx, b_hs, b_perm, b_cnt;     // sort_by_hash: 0 .. n_all - 1 | sorted hashes | sort permutation; the counter words
    DevBuf b_rid, b_m0, b_m1, b_u32, b_fl; // per valid occurrence, hash-sorted order: rid | m0 | m1 | the six u32 arrays | skip, flags
    DevBuf b_key, b_key2, b_ent, b_hit;    // K3b, from marker_buffers to drop_marker_buffers: marker values (in | sorted) | entries | hit_i
    static constexpr int CNT_VALID = 0, CNT_SKIPPED = 4;   // u32 words of b_cnt: count_valid_kernel's answer, skip_kernel's count
    const uint64_t* hs;
    uint64_t *rid, *m0, *m1;
    // b_u32: six arrays of nv1 words.  Four serve twice, under a second name from the step on that kills the first:
    uint32_t* head;                        // 1 at the first occurrence of a k-mer (a segment head), else 0
    uint32_t *headidx, *Eu;                // i at a head, else 0: dead once segments() has its running maximum | from count() on: exclusive sum of u
    uint32_t *seg_start, *start;           // first occurrence of the occurrence's k-mer: dead behind count() | in emit(): first occurrence of k-mer s, start[n_seg] = nv
    uint32_t* seg_id;                      // number of the occurrence's k-mer: exclusive sum of head
    uint32_t *u, *counted;                 // processed_i (pairs, flag_duplicates), then would-be-counted_i: dead behind its sum Eu | from count() on
    uint32_t* Ec;                          // exclusive sum of u while that is processed (Eproc), then of counted
    uint8_t *skip, *flags, *hit;
    const uint8_t* skip_arg = nullptr;     // skip once mate_skip has run, else nullptr: what the later kernels are handed
    unsigned int* d_skipped() const { return b_cnt.as<unsigned int>() + CNT_SKIPPED; }

    GenericReplay(sylph_ctx* c, bool paired_, int dedup)
        : ctx(c), s(c->stream), paired(paired_), no_dedup(dedup == DEDUP_NONE), filter(dedup == DEDUP_FILTER), b_idx(c), b_hs(c), b_perm(c),
          b_cnt(c), b_rid(c), b_m0(c), b_m1(c), b_u32(c), b_fl(c), b_key(c), b_key2(c), b_ent(c), b_hit(c) {
        b_cnt.reserve(64);
    }
    // stable sort by hash; invalid occurrences carry ~0 and end up behind the nv valid ones
    void sort_by_hash(const uint64_t* d_hash, uint32_t n_all) {
        HostPhase ph(ctx, "finish: sort by hash");
        b_idx.reserve((size_t)n_all * 4); b_hs.reserve((size_t)n_all * 8); b_perm.reserve((size_t)n_all * 4);
        hipLaunchKernelGGL(iota_kernel, dim3(grid_for64(n_all)), dim3(256), 0, s, b_idx.as<uint32_t>(), n_all);
        sort_pairs_u64_u32(ctx, d_hash, b_hs.as<uint64_t>(), b_idx.as<uint32_t>(), b_perm.as<uint32_t>(), n_all, 0, 64);
        uint32_t* d_nv = b_cnt.as<uint32_t>() + CNT_VALID;
        hipLaunchKernelGGL(count_valid_kernel, dim3(1), dim3(1), 0, s, b_hs.as<uint64_t>(), n_all, d_nv);
        ctx->read_back(&nv, d_nv, 4);
    }
    void carve() {
        nv1 = (size_t)nv + 1;
        b_rid.reserve((size_t)nv * 8); b_m0.reserve((size_t)nv * 8); b_m1.reserve((size_t)nv * 8);
        b_u32.reserve(nv1 * 4 * 6);          // head | headidx -> Eu | seg_start -> start | seg_id | u -> counted | Ec
        b_fl.reserve((size_t)nv * 2);        // skip | flags
        hs = b_hs.as<uint64_t>(); rid = b_rid.as<uint64_t>(); m0 = b_m0.as<uint64_t>(); m1 = b_m1.as<uint64_t>();
        head = b_u32.as<uint32_t>(); Eu = headidx = head + nv1; start = seg_start = headidx + nv1;
        seg_id = seg_start + nv1; counted = u = seg_id + nv1; Ec = u + nv1;
        skip = b_fl.as<uint8_t>(); flags = skip + nv;
    }
    // the records' payload in hash-sorted order; head, headidx
    void gather_heads(const OccRec* d_recs) {
        ScopedKernelTimer t(ctx, "replay");
        hipLaunchKernelGGL(gather_heads_kernel, dim3(grid_for64(nv)), dim3(256), 0, s, hs, b_perm.as<uint32_t>(), d_recs, nv, rid, m0, m1, head, headidx);
    }
    // seg_start, seg_id (headidx dies); the mate-skip counter starts at 0
    void segments() {
        inclusive_max_u32(ctx, headidx, seg_start, nv);
        exclusive_sum_u32(ctx, head, seg_id, nv);
        SY_HIP(hipMemsetAsync(d_skipped(), 0, 4, s));
    }
    // K3a (pairs): mate 2 whose hash mate 1 produced
    void mate_skip() {
        hipLaunchKernelGGL(skip_kernel, dim3(grid_for64(nv)), dim3(256), 0, s, rid, seg_start, nv, skip, d_skipped());
        skip_arg = skip;
    }
    // (both arms of the marker test reserve all four; the filter's uses `hit` only)
    void marker_buffers() {
        ne = (size_t)nv * 2;
        b_key.reserve(ne * 8); b_key2.reserve(ne * 8);
        b_ent.reserve(ne * 4 * 4);           // ent_in -> ent_out | ent_mid | sk_in | sk_out
        b_hit.reserve((size_t)nv + 4);
        hit = b_hit.as<uint8_t>();
        SY_HIP(hipMemsetAsync(hit, 0, nv, s));
    }
    void drop_marker_buffers() { b_hit.release(); b_ent.release(); b_key2.release(); b_key.release(); }
    // K3b, exact set: hit_i = one of i's markers was inserted by an earlier processed occurrence of its k-mer, by two stable sorts
    void marker_hits_exact() {
        // entries e = 2 i + w as generated | sorted by value | their segment keys | those sorted
        uint32_t *ent_in = b_ent.as<uint32_t>(), *ent_mid = ent_in + ne, *sk_in = ent_mid + ne, *sk_out = sk_in + ne;
        uint32_t* ent_out = ent_in;          // the entries sorted by (segment, value): ent_in is dead behind the first sort
        hipLaunchKernelGGL(marker_entries_kernel, dim3(grid_for64(ne)), dim3(256), 0, s, rid, m0, m1, skip_arg, nv, b_key.as<uint64_t>(), ent_in);
        sort_pairs_u64_u32(ctx, b_key.as<uint64_t>(), b_key2.as<uint64_t>(), ent_in, ent_mid, ne, 0, 64);
        hipLaunchKernelGGL(marker_segkey_kernel, dim3(grid_for64(ne)), dim3(256), 0, s, ent_mid, rid, seg_start, skip_arg, nv, sk_in);
        sort_pairs_u32_u32(ctx, sk_in, sk_out, ent_mid, ent_out, ne, 0, std::max(1, bit_length(nv)));
        hipLaunchKernelGGL(marker_hits_kernel, dim3(grid_for64(ne)), dim3(256), 0, s, ent_out, sk_out, m0, m1, nv, hit);
    }
    // K3b, sketch.rs:733-769: the marker test is the filter's answer (a10.hip), no sorting of marker entries
    void marker_hits_filter() { hipLaunchKernelGGL(filter_hits_kernel, dim3(grid_for64(nv)), dim3(256), 0, s, rid, nv, hit); }
    // flags: bit 0 = skip, bit 1 = would be dropped (u and Ec are free until would_count: they carry processed and its sum for the pairs)
    void flag_duplicates() {
        const uint32_t* Eproc = nullptr;
        if (skip_arg) {
            hipLaunchKernelGGL(processed_kernel, dim3(grid_for64(nv1)), dim3(256), 0, s, skip_arg, nv, u);
            exclusive_sum_u32(ctx, u, Ec, nv1);
            Eproc = Ec;
        }
        hipLaunchKernelGGL(dup_flags_kernel, dim3(grid_for64(nv)), dim3(256), 0, s, rid, m0, m1, seg_start, skip_arg, Eproc, hit, nv, filter ? 1 : 0, flags);
    }
    void no_flags() { SY_HIP(hipMemsetAsync(flags, 0, nv, s)); }
    // K3c: u
    void would_count() { hipLaunchKernelGGL(would_count_kernel, dim3(grid_for64(nv1)), dim3(256), 0, s, flags, nv, no_dedup ? 1 : 0, u); }
    // K3c: Eu (= headidx), counted (= u), Ec
    void count() {
        exclusive_sum_u32(ctx, u, Eu, nv1);
        {
            ScopedKernelTimer t(ctx, "replay");
            hipLaunchKernelGGL(counted_kernel, dim3(grid_for64(nv1)), dim3(256), 0, s, flags, Eu, seg_start, nv, no_dedup ? 1 : 0,
                               paired ? 0u : 4u /* MAX_DEDUP_COUNT, constants.rs:14 */, counted);
        }
        exclusive_sum_u32(ctx, counted, Ec, nv1);
    }
    // the table's size and the removed count from the tail words (the replay's one synchronising read-back), then the table
    void emit(DevBuf& out_k, DevBuf& out_c, uint64_t& n_out, uint64_t& removed_out) {
        struct Tail { uint32_t last_seg_id, last_head, n_counted, n_skipped; } tail;
        uint8_t* pin = (uint8_t*)ctx->pinned;
        SY_HIP(hipMemcpyAsync(pin + offsetof(Tail, last_seg_id), seg_id + (nv - 1), 4, hipMemcpyDeviceToHost, s));
        SY_HIP(hipMemcpyAsync(pin + offsetof(Tail, last_head), head + (nv - 1), 4, hipMemcpyDeviceToHost, s));
        SY_HIP(hipMemcpyAsync(pin + offsetof(Tail, n_counted), Ec + nv, 4, hipMemcpyDeviceToHost, s));
        SY_HIP(hipMemcpyAsync(pin + offsetof(Tail, n_skipped), d_skipped(), 4, hipMemcpyDeviceToHost, s));
        SY_HIP(hipStreamSynchronize(s));
        memcpy(&tail, pin, sizeof tail);
        const uint32_t n_seg = tail.last_seg_id + tail.last_head;
        out_k.reserve((size_t)n_seg * 8);
        out_c.reserve((size_t)n_seg * 4);
        ScopedKernelTimer t(ctx, "replay");
        hipLaunchKernelGGL(seg_starts_kernel, dim3(grid_for64(nv)), dim3(256), 0, s, head, seg_id, nv, n_seg, start);
        hipLaunchKernelGGL(emit_table_kernel, dim3(grid_for64(n_seg)), dim3(256), 0, s, hs, start, Ec, n_seg, out_k.as<uint64_t>(), out_c.as<uint32_t>());
        SY_HIP(hipGetLastError());
        n_out = n_seg;
        removed_out = (unsigned long long)nv - tail.n_skipped - tail.n_counted;   // processed - counted
    }
};

}  // namespace

// Device-wide replay of dup_removal_lsh_full_exact over `n_all` occurrences (hash = sort key, INVALID_HASH entries ignored;
// recs in file order): stable radix sort by hash, then per-occurrence kernels and scans (see the file header).  Writes the
// (k-mer, count) table in ascending k-mer order.  Used for whole samples (finish = generic, c < 2) and, by the bucket path,
// for the occurrences of buckets that do not fit in LDS.
void generic_replay(sylph_ctx* ctx, const uint64_t* d_hash, const OccRec* d_recs, uint32_t n_all, bool paired, int dedup,
                    DevBuf& out_k, DevBuf& out_c, uint64_t& n_out, uint64_t& removed_out) {
    n_out = 0;
    removed_out = 0;
    GenericReplay r(ctx, paired, dedup);
    if (n_all) r.sort_by_hash(d_hash, n_all);
    if (!r.nv) return;
    HostPhase ph_replay(ctx, "finish: replay");
    r.carve();
    r.gather_heads(d_recs);
    r.segments();
    {
        ScopedKernelTimer t(ctx, "replay");
        if (paired) r.mate_skip();                  // mate 2 whose hash mate 1 produced: not processed at all (sketch.rs:852)
        if (!r.no_dedup || paired) {
            // (with --no-dedup only the skip flags matter, :852 applies regardless; the marker flags are ignored by
            //  would_count_kernel, but computing them keeps one code path)
            r.marker_buffers();
            if (r.filter) r.marker_hits_filter(); else r.marker_hits_exact();
            r.flag_duplicates();                    // dropped_i of the header
            r.drop_marker_buffers();
        } else
            r.no_flags();
        r.would_count();
    }
    r.count();                                      // the cut-off: counted_i from u_i and P_i
    r.emit(out_k, out_c, n_out, removed_out);
}

}  // namespace sylph
