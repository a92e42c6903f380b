// replay_bucket.h — what one workgroup of the in-LDS replay does with one bucket (replay_lds.hip has the kernels around it and the host
// side): the arguments and the LDS of a replay workgroup, the steps the bodies share, and the three bodies — replay_bucket (any bucket a
// configuration holds), replay_bucket_lane (the common bucket, one occurrence per lane) and count_bucket (marker-less samples).
#pragma once
#include "sketch_session.h"
#include "partition.h"

namespace sylph {
namespace {

// Three configurations of the same kernel template (replay_plan.h: CAP_SMALL / CAP_MID / CAP_LARGE; the first carries a second, leaner
// body for buckets of up to LANE_CAP).  Buckets of up to CAP_SMALL occurrences (all of them, for ordinary samples) run with 10 KiB of
// LDS per workgroup -> 16 workgroups = 32 wavefronts per CU, which is what hides the latency of this barrier- and gather-heavy kernel
// (with a single 512-slot configuration occupancy was 14 wavefronts and the kernel 1.4x slower).  Larger buckets, and buckets that
// hold a deep k-mer (SEG_LIMIT), are queued for the CAP_MID / CAP_LARGE configurations, which replace the scan over a k-mer's earlier
// occurrences by a hash table in LDS and are launched only when something was queued; only beyond CAP_LARGE does a bucket take the
// device-wide path.
#ifndef SYLPH_REPLAY_TPB
#define SYLPH_REPLAY_TPB 128
#endif
constexpr int RTPB_SMALL = SYLPH_REPLAY_TPB;
constexpr int RTPB_MID = 256;        // hashed marker test, ~31 KiB of LDS: 5 workgroups per CU
constexpr int RTPB_LARGE = 256;      // hashed marker test, ~59 KiB of LDS: 2 workgroups per CU
constexpr uint32_t SINGLE_CUTOFF = 4;   // MAX_DEDUP_COUNT, constants.rs:14 (single-end; pairs have none)

// What a replay / count workgroup needs besides its bucket: filled once by finish_bucketed and passed to the kernels by value.
struct ReplayArgs {
    const OccRec* recs;          // replay: the occurrence records, gathered through perm
    const uint64_t* hash;        // count (marker-less samples): the hashes — sorted by bucket already when perm is null
    const uint32_t* perm;        // occurrence indices grouped by bucket
    const uint32_t* boff;        // boff[b] = first position of bucket b
    const uint32_t* p_nv;        // number of valid occurrences (= boff[B])
    int paired, dedup;           // dedup: a DEDUP_* mode
    uint32_t cutoff;             // 4 for single-end (sketch.rs:937), 0 for pairs
    BucketMap bm;
    uint64_t* tmp_k;             // rows of bucket b go to tmp_k / tmp_c [boff[b] ..), n_distinct[b] of them
    uint32_t* tmp_c;
    uint32_t* n_distinct;
    uint32_t* removed_b;
    uint32_t* overflow;          // FinishTail::overflow
    uint32_t* mid_list;          // [0] = buckets queued for the CAP_MID configuration, [1..] = their ids; the same for CAP_LARGE ...
    uint32_t* large_list;
    uint32_t* ovf_list;          // ... and for the host, which sends those buckets' occurrences through the device-wide path
    int dbg_stage;
};

// The LDS of one replay workgroup.  The kernel owns it and hands it to the body that runs the bucket: the lane body works in the
// first LANE_CAP entries of the 256-slot configuration's arrays, so the two bodies of one kernel cost the LDS of one.
template <int CAP, int RTPB>
struct ReplayLds {
    uint64_t hash[CAP], rid[CAP], m0[CAP], m1[CAP];
    __attribute__((aligned(8))) uint16_t seg[CAP];   // first sorted position of the k-mer each sorted position belongs to
    uint8_t fl[CAP];                                 // bit0 skip, bit1 would-be-dropped
    __attribute__((aligned(8))) uint16_t ab[2 * (CAP + 2)];   // exclusive counts <= CAP (s_a | s_b); before them: the marker tags
    uint32_t wave[RTPB / 64];
};

// 15-bit tag of a dedup marker, never 0 (bit 0 set): what the scan over a k-mer's earlier occurrences compares first
__device__ __forceinline__ uint32_t marker_tag(uint64_t m) { return (uint32_t)((m * 0x9E3779B97F4A7C15ull) >> 49) | 1u; }

// ---- the steps the bodies share: each works on the workgroup's LDS arrays and one sorted position --------------------------------
// Bucket b's stretch of the permutation: `n` occurrences from `first` on.  False: inconsistent bounds (defensive) — a general body
// counts such a bucket in `overflow`, and the host redoes the sample by the device-wide path.
__device__ __forceinline__ bool bucket_bounds(const ReplayArgs& ra, uint32_t b, uint32_t& first, uint32_t& n) {
    const uint32_t last = ra.boff[b + 1];
    first = ra.boff[b];
    n = last - first;
    return first <= last && last <= *ra.p_nv;
}
// One lane appends bucket b to a list ([0] = number of buckets queued, [1..] = their ids): mid_list / large_list for the next
// configurations, ovf_list for the host, which sends the occurrences of such buckets through the device-wide path.
__device__ __forceinline__ void queue_bucket(uint32_t* list, uint32_t b) { list[1 + atomicAdd(&list[0], 1u)] = b; }

// The starts of the sub-ranges from their counts (s_cnt[t] = start of sub-range t, s_cnt[SUBS] = n), and the hand-off of a bucket with a
// deep k-mer.  A k-mer SEG_LIMIT deep fills its sub-range that far (equal hashes share a sub-range): such a bucket is for the hashed
// marker test of the 512-slot configuration — passed on now, before the placement, the ranking (as long as the k-mer is deep, per
// occurrence) and the segment scans are spent on it here.  (A sub-range that full without a deep k-mer does not happen with ~0.5
// occurrences per sub-range; the next configuration is right for any bucket it can hold.)  True, for every lane: handed on.
template <int SUBS, int TPB>
__device__ __forceinline__ bool sub_range_starts_or_hand_off(uint32_t* s_cnt, uint32_t* s_wave, bool dedup, uint32_t* mid_list, uint32_t b) {
    const bool deep = scan_counters<SUBS, TPB>(s_cnt, s_cnt, s_wave) >= SEG_LIMIT;
    if (!__syncthreads_or(deep && dedup)) return false;
    if (threadIdx.x == 0) queue_bucket(mid_list, b);
    return true;
}
// Sorted position of an occurrence = start of its sub-range [lo, hi) + members with a smaller one-word key (rkey: residue of the hash
// << rank_bits | index); `head` = start + members with a smaller HASH — the sorted position of the k-mer's first occurrence, its
// segment head (equal hashes share a sub-range; key < hkey <=> smaller hash: the index sits below rank_bits) — so that no scan has to
// find the heads afterwards.
__device__ __forceinline__ uint32_t rank_and_head(const uint64_t* s_key, uint32_t lo, uint32_t hi, uint64_t rkey, int rank_bits, uint32_t& head) {
    const uint64_t hkey = rkey & ~((1ull << rank_bits) - 1ull);
    uint32_t smaller = 0, below = 0;
    for (uint32_t p = lo; p < hi; p++) {
        const uint64_t kp = s_key[p];
        smaller += kp < rkey ? 1u : 0u;
        below += kp < hkey ? 1u : 0u;
    }
    head = lo + below;
    return lo + smaller;
}
// Mate-2 skip (sketch.rs:852): the occurrence at sorted position j, of the k-mer whose segment starts at `seg`, is a mate 2 whose
// mate 1 holds the k-mer too (the mates of a pair are neighbours in file order, hence in the segment).
__device__ __forceinline__ bool mate2_skipped(const uint64_t* s_rid, uint32_t seg, uint32_t j) {
    const uint64_t rec = s_rid[j] & RID_MASK;
    if (rec & 1) {
        for (uint32_t q = j; q > seg;) {
            q--;
            const uint64_t rq = s_rid[q] & RID_MASK;
            if ((rq >> 1) != (rec >> 1)) break;
            if ((rq & 1) == 0) return true;
        }
    }
    return false;
}
// DEDUP_FILTER: `*c > 0` (sketch.rs:749, :756) = an occurrence of the k-mer went through the dedup before this one.  The walk hands
// over a record's seeds in EMISSION order (the rank bits of the rid; lane-interleaved for the AVX2 routine), the segment lists them
// by position: the first of the walk is the lowest rank among the segment's leading occurrences of the head's record — the head
// itself unless the read repeats the k-mer (a tandem repeat inside one read).  (None of those is a skipped mate 2: the mate-1
// occurrence that would make it one belongs to an earlier record.)
__device__ __forceinline__ bool walk_first(const uint64_t* s_rid, const uint16_t* s_seg, uint32_t n, uint32_t j) {
    const uint32_t s0 = s_seg[j];
    const uint64_t rec0 = s_rid[s0] & RID_MASK, rj = s_rid[j];
    if ((rj & RID_MASK) != rec0) return false;
    const uint64_t rank_j = (rj >> RID_RANK_SHIFT) & RID_RANK_MAX;
    for (uint32_t q = s0; q < n && (uint32_t)s_seg[q] == s0 && (s_rid[q] & RID_MASK) == rec0; q++)
        if (q != j && ((s_rid[q] >> RID_RANK_SHIFT) & RID_RANK_MAX) < rank_j) return false;
    return true;
}
// The tag word of an occurrence that puts its markers into the set: two 15-bit tags, never 0 (an occurrence that puts nothing into
// it — skipped mate 2, no markers — has the word 0).
__device__ __forceinline__ uint32_t marker_tags(uint64_t m0, uint64_t m1) { return marker_tag(m0) | (marker_tag(m1) << 16); }
// The marker test of the small configuration: does an earlier occurrence of the k-mer (sorted positions [seg, j)) hold marker a or b?
// The scan reads ONE 32-bit word per earlier occurrence — its tag word — and looks at the 16 bytes of markers only where a tag matches
// (a real duplicate, or 4 x 2^-15 by chance); flag byte + record id + both markers (25 bytes of LDS, four 64-bit compares) per earlier
// occurrence made this loop a third of the kernel for a community with 30x genomes in it.  ("A processed occurrence precedes j" is
// "j is not the head": the head of a segment is never a skipped mate 2.)
__device__ __forceinline__ bool tag_scan_hit(const uint32_t* s_tag, const uint64_t* s_m0, const uint64_t* s_m1, uint32_t seg, uint32_t j,
                                             uint64_t a, uint64_t b) {
    const uint32_t ta = marker_tag(a) * 0x00010001u, tb = marker_tag(b) * 0x00010001u;
    for (uint32_t q = seg; q < j; q++) {
        const uint32_t w = s_tag[q], za = w ^ ta, zb = w ^ tb;
        if ((((za - 0x00010001u) & ~za) | ((zb - 0x00010001u) & ~zb)) & 0x80008000u) {     // a zero halfword in either
            const uint64_t x = s_m0[q], y = s_m1[q];
            if (w && (x == a || y == a || x == b || y == b)) return true;
        }
    }
    return false;
}
// End of the segment that starts at sorted position j = the next head or n: a walk (segments of the small configuration are shorter
// than SEG_LIMIT).
__device__ __forceinline__ uint32_t segment_end(const uint16_t* s_seg, uint32_t n, uint32_t j) {
    uint32_t e = j + 1;
    while (e < n && s_seg[e] == j) e++;
    return e;
}

// One workgroup = one bucket.  SINGLE_CUTOFF = 4 for single-end (sketch.rs:937), 0 for pairs.
//
// Ordering inside the bucket: the partition hands over the bucket's occurrences in no particular order, but the index an
// occurrence is gathered by (position in the dense arrays / slot number) grows with the file order: a first rank loop over the
// indices gives every occurrence its ARRIVAL number (its place by (record, position) inside the bucket); what is left is a
// sort by (hash, arrival).  Each lane keeps its (up to ITEMS) records in registers, publishes one 64-bit key per record in
// LDS and finds the record's sorted position by counting smaller keys — every lane reads the same LDS word per step (a
// broadcast, no bank conflicts), the loop has no barriers and no dependent LDS round trips, and it is O(n^2 / lanes) with
// n ~ 200.  Keys are unique: the bucket's hashes lie in one narrow range, so key = (hash - lowest hash of the bucket) << 10 |
// arrival number whenever that difference fits in 54 bits (bm.composite, decided by the host; else — tiny samples — the
// two-part comparison is spelled out).  Records are then written straight to their sorted slots.
// Handles buckets with min_n < n <= CAP; larger ones bump `overflow` (when count_overflow) and are left to the caller.
template <int CAP, int RTPB>
__device__ __forceinline__ void replay_bucket(const uint32_t b, const ReplayArgs& ra, ReplayLds<CAP, RTPB>& lds) {
    const OccRec* __restrict__ recs = ra.recs;
    const uint32_t* __restrict__ perm = ra.perm;
    uint64_t* __restrict__ tmp_k = ra.tmp_k;
    uint32_t* __restrict__ tmp_c = ra.tmp_c;
    uint32_t* __restrict__ n_distinct = ra.n_distinct;
    uint32_t* __restrict__ mid_list = ra.mid_list;
    const int paired = ra.paired, dbg_stage = ra.dbg_stage;
    const uint32_t cutoff = ra.cutoff;
    const BucketMap& bm = ra.bm;
    constexpr int ITEMS = CAP / RTPB;     // records per lane
    constexpr int CFG = cfg_of_cap(CAP);  // the configuration's entry of bm.sub_mult / sub_width / rank_bits
    // The medium / large configurations are HASHED: their marker test is a hash table in LDS, their sub-ranges are cut a second time by
    // index where they hold one deep k-mer, and they find the segment heads by a scan.  The small one scans a k-mer's earlier
    // occurrences, hands a bucket with a deep k-mer on, and has its rank loops yield the segment heads.
    constexpr bool HASHED = CAP != CAP_SMALL;
    // DEDUP_FILTER (the reference's default for pairs, a10.hip): everything as in the exact mode except the marker test itself,
    // which is the bit a10_mark left in the occurrence's record.
    const bool filter = ra.dedup == DEDUP_FILTER;
    const int no_dedup = filter ? 0 : ra.dedup;
    uint64_t* const s_hash = lds.hash, * const s_rid = lds.rid, * const s_m0 = lds.m0, * const s_m1 = lds.m1;
    uint16_t* const s_seg = lds.seg;
    uint8_t* const s_fl = lds.fl;
    uint16_t* const s_ab = lds.ab;
    uint16_t* const s_a = s_ab;
    uint16_t* const s_b = s_ab + (CAP + 2);
    uint32_t* const s_wave = lds.wave;
    const uint32_t tid = threadIdx.x;
    uint32_t first, n;
    if (!bucket_bounds(ra, b, first, n)) { if (tid == 0) atomicAdd(ra.overflow, 1u); return; }
    if (n == 0) return;                   // (n_distinct was zeroed by the host)
    // too large for this configuration: for the first one that holds it, or for the host
    if (n > CAP) {
        if (tid == 0)
            queue_bucket((CAP < CAP_MID && n <= (uint32_t)CAP_MID) ? mid_list : (CAP < CAP_LARGE && n <= (uint32_t)CAP_LARGE) ? ra.large_list : ra.ovf_list, b);
        return;
    }
    // ---- gather (through the partition permutation, one 32 B sector per occurrence) + sort by (hash, file order) -------
    uint64_t* s_key = s_m0;               // keys live in s_m0 until the sorted records are written
    const bool composite = bm.composite != 0;
    const uint64_t lo_hash = composite ? bucket_lo_hash(b, bm.mult, bm.sh) : 0ull;
    OccRec r[ITEMS];
    uint32_t pidx[ITEMS], rank[ITEMS];
    uint32_t seg0[ITEMS];                 // small configuration: the segment heads, from the rank loops
#pragma unroll
    for (int q = 0; q < ITEMS; q++) seg0[q] = 0;
    uint32_t* const s_pidx = reinterpret_cast<uint32_t*>(s_rid);   // (s_rid is free until the sorted records are written)
    const int levels = (int)((n + RTPB - 1) / RTPB);   // lanes of level q hold a record iff q < levels (wave-uniform)
    // every load of the bucket before the first wait: a lane past the end loads the bucket's last entry again (one line for the
    // whole wavefront), so there is no branch around the loads and the gather is two load latencies, not one per record
#pragma unroll
    for (int q = 0; q < ITEMS; q++) pidx[q] = perm[first + min(tid + q * RTPB, n - 1u)];
#pragma unroll
    for (int q = 0; q < ITEMS; q++) r[q] = recs[pidx[q]];
#pragma unroll
    for (int q = 0; q < ITEMS; q++) {
        rank[q] = 0;
        if (tid + q * RTPB >= n) pidx[q] = 0xFFFFFFFFu;
    }
    if (composite) {
        // Sub-bin sort, linear in the bucket: the bucket's hashes are uniform over its narrow range, so CAP equal sub-ranges hold
        // about half an occurrence each.  Count per sub-range (LDS atomics), scan, drop every (hash, index) into its sub-range
        // (any order), then each occurrence ranks itself among the few members of its own sub-range: sorted position =
        // start of the sub-range + members with a smaller (hash, index).  The occurrences of one k-mer share a sub-range: for
        // them that loop is as long as the k-mer is deep, like the marker test below.  (Rounds 1-2 ranked every occurrence
        // against the whole bucket, n^2 comparisons; with the partition no longer stable a second such loop over the indices
        // would have been needed on top.)
        uint32_t* const s_cnt = reinterpret_cast<uint32_t*>(s_m1);   // CAP + 1 counters (s_m1 is free until the sorted records are written)
        const uint32_t sub_mult = bm.sub_mult[CFG];
        uint32_t sub[ITEMS];
        const int rank_bits = bm.rank_bits[CFG];
        // hashed configurations (deep buckets): lowest and highest hash of every sub-range (s_hash / s_rid are free until the
        // sorted records are written) — a sub-range whose two are equal holds ONE k-mer, see the second level below
        unsigned long long* const s_min = reinterpret_cast<unsigned long long*>(s_hash);
        unsigned long long* const s_max = reinterpret_cast<unsigned long long*>(s_rid);
        for (uint32_t t = tid; t <= (uint32_t)CAP; t += RTPB) s_cnt[t] = 0;
        // (the placement's counters too: s_seg is not written before the segments)
        for (uint32_t t = tid; t < (uint32_t)CAP / 2; t += RTPB) reinterpret_cast<uint32_t*>(s_seg)[t] = 0;
        if constexpr (HASHED)
            for (uint32_t t = tid; t < (uint32_t)CAP; t += RTPB) { s_min[t] = ~0ull; s_max[t] = 0ull; }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < ITEMS; q++) {
            const uint32_t i = tid + q * RTPB;
            sub[q] = 0;
            if (i < n) {
                sub[q] = sub_range_of((uint32_t)((r[q].hash - lo_hash) >> bm.sh), sub_mult, CAP);          // (the distance is < bm.range_hs)
                atomicAdd(&s_cnt[sub[q]], 1u);
                if constexpr (HASHED) {
                    atomicMin(&s_min[sub[q]], (unsigned long long)r[q].hash);
                    atomicMax(&s_max[sub[q]], (unsigned long long)r[q].hash);
                }
            }
        }
        __syncthreads();
        // s_cnt[t] = start of sub-range t, s_cnt[CAP] = n
        if constexpr (HASHED) {
            scan_counters<CAP, RTPB>(s_cnt, s_cnt, s_wave);
            __syncthreads();
        } else if (sub_range_starts_or_hand_off<CAP, RTPB>(s_cnt, s_wave, !no_dedup, mid_list, b))
            return;
        // Second level (hashed configurations): the occurrences of a DEEP k-mer all sit in one sub-range, and ranking them among
        // each other by index is quadratic in the depth.  A sub-range that holds one k-mer only (lowest hash = highest hash) and
        // at least DEEP_SUB occurrences is therefore cut once more, by INDEX: cnt equal index ranges own one place each of the
        // sub-range's cnt places (the occurrences of a k-mer are spread over the file like the reads are, so the ranges hold
        // about one each; whatever they hold is ranked inside its range, so any spread is sorted correctly).  Bin of an
        // occurrence = first place of its sub-range (+ its index range): bins are places, they order like (hash, index).
        uint32_t bin[ITEMS];
        const uint32_t* starts = s_cnt;
#pragma unroll
        for (int q = 0; q < ITEMS; q++) bin[q] = sub[q];
        if constexpr (HASHED) {
            if (rank_bits) {
                constexpr uint32_t DEEP_SUB = 32;
                uint32_t* const s_c2 = reinterpret_cast<uint32_t*>(s_m0);       // CAP + 1 counters (s_key is not written before the placement)
                uint32_t* const s_s2 = reinterpret_cast<uint32_t*>(s_hash);     // their scan (s_min is done with by then)
                for (uint32_t t = tid; t <= (uint32_t)CAP; t += RTPB) s_c2[t] = 0;
                __syncthreads();
#pragma unroll
                for (int q = 0; q < ITEMS; q++) {
                    const uint32_t i = tid + q * RTPB;
                    if (i < n) {
                        const uint32_t lo = s_cnt[sub[q]], cnt = s_cnt[sub[q] + 1] - lo;
                        const bool pure = cnt >= DEEP_SUB && s_min[sub[q]] == s_max[sub[q]];
                        bin[q] = lo + (pure ? min(cnt - 1u, (uint32_t)(((uint64_t)pidx[q] * cnt) >> rank_bits)) : 0u);
                        atomicAdd(&s_c2[bin[q]], 1u);
                    }
                }
                __syncthreads();
                scan_counters<CAP, RTPB>(s_c2, s_s2, s_wave);
                __syncthreads();
                starts = s_s2;
            }
        }
        // place (cursor = a second counter array would cost LDS: take places from the END of each sub-range instead, counting the
        // start words' neighbours down is not possible either — so the places come from s_seg, which is free until the segments)
        uint16_t* const s_fill = s_seg;                               // members placed so far per sub-range (<= CAP: 16 bits do)
        // ranking key of an occurrence inside its sub-range: (hash - a lower bound of the sub-range's hashes, index) in one word
        // when the host found room for both (rank_bits > 0), else the hash with the indices in a second array
        uint64_t rkey[ITEMS];
#pragma unroll
        for (int q = 0; q < ITEMS; q++) {
            const uint32_t i = tid + q * RTPB;
            rkey[q] = 0;
            if (i < n) {
                const uint32_t place = starts[bin[q]] + take_place(s_fill, bin[q]);
                if (rank_bits) {
                    const uint64_t res = (r[q].hash - lo_hash) - ((uint64_t)(sub[q] * bm.sub_width[CFG]) << bm.sh);
                    rkey[q] = (res << rank_bits) | pidx[q];
                    s_key[place] = rkey[q];
                } else {
                    s_key[place] = r[q].hash;
                    s_pidx[place] = pidx[q];
                }
            }
        }
        __syncthreads();
        if (dbg_stage == 1) { if (tid == 0) n_distinct[b] = 0; return; }
        if (rank_bits) {
#pragma unroll
            for (int q = 0; q < ITEMS; q++) {
                const uint32_t i = tid + q * RTPB;
                if (i < n) {
                    const uint32_t lo = starts[bin[q]], hi = starts[bin[q] + 1];
                    if constexpr (HASHED) {
                        uint32_t smaller = 0;
                        for (uint32_t p = lo; p < hi; p++) smaller += s_key[p] < rkey[q] ? 1u : 0u;
                        rank[q] = lo + smaller;
                    } else
                        rank[q] = rank_and_head(s_key, lo, hi, rkey[q], rank_bits, seg0[q]);
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < ITEMS; q++) {
                const uint32_t i = tid + q * RTPB;
                if (i < n) {
                    const uint32_t lo = starts[bin[q]], hi = starts[bin[q] + 1];
                    uint32_t smaller = 0, below = 0;
                    for (uint32_t p = lo; p < hi; p++) {
                        const uint64_t kp = s_key[p];
                        smaller += (kp < r[q].hash || (kp == r[q].hash && s_pidx[p] < pidx[q])) ? 1u : 0u;
                        if constexpr (!HASHED) below += kp < r[q].hash ? 1u : 0u;
                    }
                    rank[q] = lo + smaller;
                    seg0[q] = lo + below;
                }
            }
        }
    } else {
        // tiny samples (the bucket's hash range does not fit the key): every occurrence against every other, as in rounds 1-2
        uint16_t* const s_arr = s_a;                                  // (free until the counts)
        uint32_t arrival[ITEMS];
#pragma unroll
        for (int q = 0; q < ITEMS; q++) {
            const uint32_t i = tid + q * RTPB;
            arrival[q] = 0;
            if (i < n) s_pidx[i] = pidx[q];
        }
        __syncthreads();
        // arrival number = how many of the bucket's occurrences come earlier in the file (their indices are distinct)
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t pj = s_pidx[j];
#pragma unroll
            for (int q = 0; q < ITEMS; q++)
                if (q < levels) arrival[q] += (pj < pidx[q]) ? 1u : 0u;
        }
#pragma unroll
        for (int q = 0; q < ITEMS; q++) {
            const uint32_t i = tid + q * RTPB;
            if (i < n) { s_key[i] = r[q].hash; s_arr[i] = (uint16_t)arrival[q]; }
        }
        __syncthreads();
        if (dbg_stage == 1) { if (tid == 0) n_distinct[b] = 0; return; }
        for (uint32_t j = 0; j < n; j++) {
            const uint64_t kj = s_key[j];
#pragma unroll
            for (int q = 0; q < ITEMS; q++)
                if (q < levels && tid + q * RTPB < n) {
                    rank[q] += ((kj < r[q].hash) || (kj == r[q].hash && (uint32_t)s_arr[j] < arrival[q])) ? 1u : 0u;
                    if constexpr (!HASHED) seg0[q] += kj < r[q].hash ? 1u : 0u;
                }
        }
    }
    __syncthreads();                      // every lane is done with s_key (= s_m0), s_pidx (= s_rid), the counters (= s_m1, s_seg, s_a)
#pragma unroll
    for (int q = 0; q < ITEMS; q++) {
        const uint32_t i = tid + q * RTPB;
        if (i < n) {
            const uint32_t d = rank[q];
            s_hash[d] = r[q].hash; s_rid[d] = r[q].rid; s_m0[d] = r[q].m0; s_m1[d] = r[q].m1;
            if constexpr (!HASHED) s_seg[d] = (uint16_t)seg0[q];
        }
    }
    __syncthreads();
    if (dbg_stage == 2) { if (tid == 0) n_distinct[b] = 0; return; }
    // ---- segments ---------------------------------------------------------------------------------------------
    // lane owns `items` contiguous sorted positions; s_seg = running "last head seen" (segmented max-scan)
    const uint32_t items = (n + RTPB - 1) / RTPB;
    const uint32_t j0 = tid * items;
    uint32_t heads = 0;
    uint8_t headbits = 0;
    if constexpr (!HASHED) {
        // s_seg came with the sorted records: a head is a position that is its own segment's start
        for (uint32_t t = 0; t < items; t++) {
            const uint32_t j = j0 + t;
            if (j >= n) break;
            if ((uint32_t)s_seg[j] == j) { heads++; headbits |= (uint8_t)(1u << t); }
        }
    } else {
        uint32_t last_head = 0;
        bool has_head = false;
        for (uint32_t t = 0; t < items; t++) {
            const uint32_t j = j0 + t;
            if (j >= n) break;
            const bool hd = (j == 0) || (s_hash[j] != s_hash[j - 1]);
            if (hd) { heads++; last_head = j; has_head = true; headbits |= (uint8_t)(1u << t); }
        }
        // inclusive max-scan of last_head over lanes (a lane without a head inherits from the left)
        uint32_t carry = has_head ? last_head + 1 : 0;   // +1 so that 0 means "none"
        {
            const uint32_t lane = tid & 63, wave = tid >> 6;
            uint32_t x = carry;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(x, d);
                if (lane >= (uint32_t)d) x = max(x, y);
            }
            __syncthreads();
            if (lane == 63) s_wave[wave] = x;
            __syncthreads();
            uint32_t left = 0;
            for (uint32_t w = 0; w < wave; w++) left = max(left, s_wave[w]);
            const uint32_t prev = max(left, __shfl_up(x, 1));   // inclusive result of the lane to the left
            carry = (lane == 0) ? left : prev;
        }
        {
            uint32_t cur = carry;   // last head (+1) before this lane's first position
            for (uint32_t t = 0; t < items; t++) {
                const uint32_t j = j0 + t;
                if (j >= n) break;
                if (headbits & (1u << t)) cur = j + 1;
                s_seg[j] = (uint16_t)(cur - 1);
            }
        }
        __syncthreads();
    }
    constexpr uint32_t MARKER_TAB = 4 * CAP;    // slots of the marker table: 2 x (2 entries per occurrence)
    if constexpr (!HASHED) {
        // a long k-mer segment of occurrences that carry markers: not for the quadratic marker test below (reads above 400 bases
        // carry none — the test does not run for them, however deep the k-mer)
        // (a composite bucket got here only if no sub-range held SEG_LIMIT occurrences — every k-mer is shallower)
        if (!no_dedup && !composite) {
            __shared__ uint32_t s_longest;
            if (tid == 0) s_longest = 0;
            __syncthreads();
            uint32_t mine = 0;
            for (uint32_t t = 0; t < items; t++) {
                const uint32_t j = j0 + t;
                if (j >= n) break;
                if (s_rid[j] & RID_MARKER_BIT) mine = max(mine, j - (uint32_t)s_seg[j] + 1);
            }
            if (mine >= SEG_LIMIT) atomicMax(&s_longest, mine);
            __syncthreads();
            if (s_longest >= SEG_LIMIT) {
                if (tid == 0) queue_bucket(mid_list, b);
                return;
            }
        }
    }
    uint32_t* const s_tag = reinterpret_cast<uint32_t*>(s_ab);           // CAP words: fits the 2 x (CAP + 2) halfwords of s_a | s_b, which are written later
    // ---- mate-2 skip (sketch.rs:852) and duplicate flags ----------------------------------------------------------
    for (uint32_t t = 0; t < items; t++) {
        const uint32_t j = j0 + t;
        if (j >= n) break;
        const uint8_t fl = (paired && mate2_skipped(s_rid, s_seg[j], j)) ? 1 : 0;
        s_fl[j] = fl;
        if constexpr (!HASHED) s_tag[j] = (!fl && (s_rid[j] & RID_MARKER_BIT)) ? marker_tags(s_m0[j], s_m1[j]) : 0u;
    }
    __syncthreads();
    uint32_t my_u = 0;
    uint8_t ubits = 0;
    // The duplicate flag of every position of the lane: the filter's answer (sketch.rs:747-760, `*c > 0` = not the first of the k-mer in
    // the walk), or the exact set's — an earlier occurrence of the k-mer holds one of the two markers (marker_hit: the configuration's
    // test), or the two are equal — for every occurrence but the first of its k-mer: the head of a segment is never a skipped mate 2
    // (the mate-1 occurrence that would make it one precedes it in the segment), so "a processed occurrence precedes j" is simply
    // "j is not the head".
    auto flag_duplicates = [&](auto&& marker_hit) {
        for (uint32_t t = 0; t < items; t++) {
            const uint32_t j = j0 + t;
            if (j >= n) break;
            uint8_t fl = s_fl[j];
            if (!fl && !no_dedup && (s_rid[j] & RID_MARKER_BIT)) {
                if (filter) {
                    if ((s_rid[j] & RID_A10_BIT) && !walk_first(s_rid, s_seg, n, j)) fl |= 2;
                } else if (j != (uint32_t)s_seg[j]) {
                    const uint64_t a = s_m0[j], bb = s_m1[j];
                    if (marker_hit(j, a, bb) || a == bb) fl |= 2;
                }
            }
            const bool u = !(fl & 1) && (no_dedup || !(fl & 2));
            if (u) { my_u++; ubits |= (uint8_t)(1u << t); }
            s_fl[j] = fl;   // NB: later lanes only read bit0 of earlier positions, which does not change here
        }
    };
    if constexpr (HASHED) {
        // Marker test through a hash table in LDS.  Every processed occurrence with markers enters both of them under the key
        // (k-mer segment, marker value); a slot belongs to the first entry that claims it (owner entry in the high half of the
        // word, never changes) and keeps the smallest sorted position among the entries with its key in the low half.  An
        // occurrence is a duplicate when one of its two keys was entered from an earlier position (sketch.rs:709-722: markers
        // go into the set whether the occurrence is then counted or dropped).
        __shared__ uint32_t s_tab[MARKER_TAB];
        __shared__ uint16_t s_slot[2 * CAP];
        static_assert((MARKER_TAB & (MARKER_TAB - 1)) == 0 && 2 * CAP <= 0xFFFF, "marker table geometry");
        for (uint32_t t = tid; t < MARKER_TAB; t += RTPB) s_tab[t] = 0xFFFFFFFFu;
        __syncthreads();
        auto marker_of = [&](uint32_t e) { return (e & 1u) ? s_m1[e >> 1] : s_m0[e >> 1]; };
        if (!no_dedup && !filter) {
            for (uint32_t t = 0; t < items; t++) {
                const uint32_t j = j0 + t;
                if (j >= n) break;
                if ((s_fl[j] & 1) || !(s_rid[j] & RID_MARKER_BIT)) continue;
                const uint32_t seg = s_seg[j];
                for (uint32_t w = 0; w < 2; w++) {
                    const uint32_t e = 2 * j + w;
                    const uint64_t v = marker_of(e);
                    uint32_t h = (uint32_t)(((v ^ (v >> 31) ^ ((uint64_t)seg << 17)) * 0x9E3779B97F4A7C15ull) >> 40) & (MARKER_TAB - 1);
                    for (;;) {
                        const uint32_t old = atomicCAS(&s_tab[h], 0xFFFFFFFFu, (e << 16) | j);
                        const uint32_t o = old == 0xFFFFFFFFu ? e : old >> 16;
                        if (marker_of(o) == v && s_seg[o >> 1] == seg) {
                            if (old != 0xFFFFFFFFu) atomicMin(&s_tab[h], (o << 16) | j);
                            s_slot[e] = (uint16_t)h;
                            break;
                        }
                        h = (h + 1) & (MARKER_TAB - 1);
                    }
                }
            }
        }
        __syncthreads();
        flag_duplicates([&](uint32_t j, uint64_t, uint64_t) { return (s_tab[s_slot[2 * j]] & 0xFFFFu) < j || (s_tab[s_slot[2 * j + 1]] & 0xFFFFu) < j; });
    } else
        flag_duplicates([&](uint32_t j, uint64_t a, uint64_t bb) { return tag_scan_hit(s_tag, s_m0, s_m1, s_seg[j], j, a, bb); });
    if (dbg_stage == 3) { if (tid == 0) n_distinct[b] = 0; return; }
    // ---- P_i = would-be-counted occurrences before i in its k-mer; counted_i (cut-off rule, sketch.rs:706) ------
    // two block scans in total: (would-count, heads) packed 16+16 bits here, (counted, removed) below; sums <= CAP
    uint32_t base_h = 0, total_heads = 0, total_removed = 0;
    if (CAP <= 512 && cutoff == 0) {
        // pairs (no cut-off): counted = would-count, so ONE block scan of (would-count, heads, removed) packed 10+10+10 bits (sums <= CAP
        // <= 512) gives both the distinct indices and Ec; the per-k-mer prefix P is not needed
        uint32_t my_removed = 0;
        for (uint32_t t = 0; t < items; t++) {
            const uint32_t j = j0 + t;
            if (j >= n) break;
            if (!(s_fl[j] & 1) && !((ubits >> t) & 1)) my_removed++;
        }
        uint32_t tot = 0;
        const uint32_t base = block_excl_sum<RTPB>(my_u | (heads << 10) | (my_removed << 20), s_wave, &tot);
        base_h = (base >> 10) & 0x3FFu;
        total_heads = (tot >> 10) & 0x3FFu;
        total_removed = tot >> 20;
        uint32_t run = base & 0x3FFu;
        for (uint32_t t = 0; t < items; t++) {
            const uint32_t j = j0 + t;
            if (j >= n) break;
            s_b[j] = (uint16_t)run;             // Ec[j] = Eu[j]
            if (ubits & (1u << t)) run++;
        }
        if (j0 < n && j0 + items >= n) s_b[n] = (uint16_t)run;
        __syncthreads();
    } else {
    uint32_t tot_uh = 0;
    const uint32_t base_uh = block_excl_sum<RTPB>(my_u | (heads << 16), s_wave, &tot_uh);
    const uint32_t base_u = base_uh & 0xFFFFu;
    base_h = base_uh >> 16;
    total_heads = tot_uh >> 16;
    {
        uint32_t run = base_u;
        for (uint32_t t = 0; t < items; t++) {
            const uint32_t j = j0 + t;
            if (j >= n) break;
            s_a[j] = (uint16_t)run;             // Eu[j]
            if (ubits & (1u << t)) run++;
        }
    }
    __syncthreads();
    uint32_t my_c = 0, my_removed = 0;
    uint8_t cbits = 0;
    for (uint32_t t = 0; t < items; t++) {
        const uint32_t j = j0 + t;
        if (j >= n) break;
        const uint8_t fl = s_fl[j];
        if (fl & 1) continue;
        const uint32_t P = (uint32_t)s_a[j] - (uint32_t)s_a[s_seg[j]];
        const bool u = (ubits >> t) & 1;
        const bool c = (cutoff && P >= cutoff) ? true : u;
        if (c) { my_c++; cbits |= (uint8_t)(1u << t); } else my_removed++;
    }
    uint32_t tot_cr = 0;
    const uint32_t base_c = block_excl_sum<RTPB>(my_c | (my_removed << 16), s_wave, &tot_cr) & 0xFFFFu;
    total_removed = tot_cr >> 16;
    {
        uint32_t rc = base_c;
        for (uint32_t t = 0; t < items; t++) {
            const uint32_t j = j0 + t;
            if (j >= n) break;
            s_b[j] = (uint16_t)rc;              // Ec[j]
            if (cbits & (1u << t)) rc++;
        }
        if (j0 < n && j0 + items >= n) s_b[n] = (uint16_t)rc;   // Ec[n], written by the lane that owns the last position
    }
    __syncthreads();
    }
    // heads emit (k-mer, count); the distinct index of a head = number of heads before it
    if constexpr (HASHED) {
        // segment end = position of the next head: the heads publish their positions by distinct index (s_a is free by now)
        uint16_t* const s_headpos = s_a;
        {
            uint32_t rh = base_h;
            for (uint32_t t = 0; t < items; t++) {
                const uint32_t j = j0 + t;
                if (j >= n) break;
                if (headbits & (1u << t)) s_headpos[rh++] = (uint16_t)j;
            }
            if (tid == 0) s_headpos[total_heads] = (uint16_t)n;
        }
        __syncthreads();
        uint32_t rh = base_h;
        for (uint32_t t = 0; t < items; t++) {
            const uint32_t j = j0 + t;
            if (j >= n) break;
            if (headbits & (1u << t)) {
                const uint32_t e = s_headpos[rh + 1];
                tmp_k[first + rh] = s_hash[j];
                tmp_c[first + rh] = (uint32_t)s_b[e] - (uint32_t)s_b[j];
                rh++;
            }
        }
    } else {
        uint32_t rh = base_h;
        const uint32_t out0 = first;
        for (uint32_t t = 0; t < items; t++) {
            const uint32_t j = j0 + t;
            if (j >= n) break;
            if (headbits & (1u << t)) {
                const uint32_t e = segment_end(s_seg, n, j);
                tmp_k[out0 + rh] = s_hash[j];
                tmp_c[out0 + rh] = (uint32_t)s_b[e] - (uint32_t)s_b[j];
                rh++;
            }
        }
    }
    // (per-bucket removed counts are summed by a separate kernel: one atomic per workgroup on a single word runs at ~88
    //  atomics/us on this chip and was bounding the whole kernel at ~0.2 ms for 2e4 buckets)
    if (tid == 0) { n_distinct[b] = total_heads; ra.removed_b[b] = total_removed; }
}

// The common bucket — at most LANE_CAP occurrences, composite keys with a one-word ranking key (rank_bits > 0) — with ONE occurrence
// per lane: the steps of replay_bucket<256, 128> in the same order, the shared ones through the same functions (gather with both loads
// in flight, sub-range count, counter scan, hand-off of a bucket with a deep k-mer, placement, the rank loop that also yields the segment
// head, sorted write, mate-2 rule, tags, marker test, one packed block scan for pairs / two for single-end, rows), but a lane's sorted
// position is its thread number:
// no levels, no loops over a lane's positions, flags in registers, and what replay_bucket decides at run time — pairs or the
// single-end cut-off, exact set / filter / no dedup — is a template parameter, so that the arms a sample cannot take are not in the
// instance at all.  Writes what replay_bucket writes (tmp_k / tmp_c / n_distinct / removed_b: the sort is the same total order by
// (hash, index), only found through 128 sub-ranges instead of 256).
template <bool PAIRED, int DEDUP>
__device__ __forceinline__ void replay_bucket_lane(const uint32_t b, const uint32_t first, const uint32_t n, const ReplayArgs& ra,
                                                   ReplayLds<CAP_SMALL, LANE_CAP>& lds) {
    const OccRec* __restrict__ recs = ra.recs;
    const uint32_t* __restrict__ perm = ra.perm;
    uint64_t* __restrict__ tmp_k = ra.tmp_k;
    uint32_t* __restrict__ tmp_c = ra.tmp_c;
    const BucketMap& bm = ra.bm;
    constexpr bool filter = DEDUP == DEDUP_FILTER, no_dedup = DEDUP == DEDUP_NONE;
    uint64_t* const s_hash = lds.hash, * const s_rid = lds.rid, * const s_m0 = lds.m0, * const s_m1 = lds.m1;
    uint16_t* const s_seg = lds.seg;
    uint16_t* const s_a = lds.ab;
    uint16_t* const s_b = lds.ab + (CAP_SMALL + 2);
    uint32_t* const s_wave = lds.wave;
    const uint32_t tid = threadIdx.x;
    const bool live = tid < n;
    // ---- gather + sort by (hash, file order) ---------------------------------------------------------------------------
    // (a lane past the end loads the bucket's last entry again: no branch around the loads, two load latencies in all)
    const uint32_t pidx = perm[first + min(tid, n - 1u)];
    const OccRec r = recs[pidx];
    const uint64_t lo_hash = bucket_lo_key(b, bm.mult, bm.inv_mult) << bm.sh;      // = bucket_lo_hash(b, bm.mult, bm.sh)
    const int rank_bits = bm.rank_bits[LANE_CFG];
    uint64_t* const s_key = s_m0;                                  // keys live in s_m0 until the sorted records are written
    uint32_t* const s_cnt = reinterpret_cast<uint32_t*>(s_m1);     // LANE_CAP + 1 counters
    uint16_t* const s_fill = s_seg;                                // members placed so far per sub-range
    s_cnt[tid] = 0;
    if (tid == 0) s_cnt[LANE_CAP] = 0;
    if (tid < LANE_CAP / 2) reinterpret_cast<uint32_t*>(s_seg)[tid] = 0;
    __syncthreads();
    uint32_t sub = 0;
    if (live) {
        sub = sub_range_of((uint32_t)((r.hash - lo_hash) >> bm.sh), bm.sub_mult[LANE_CFG], LANE_CAP);
        atomicAdd(&s_cnt[sub], 1u);
    }
    __syncthreads();
    // s_cnt[t] = start of sub-range t, s_cnt[LANE_CAP] = n
    if (sub_range_starts_or_hand_off<LANE_CAP, LANE_CAP>(s_cnt, s_wave, !no_dedup, ra.mid_list, b)) return;
    uint64_t rkey = 0;
    if (live) {
        const uint32_t place = s_cnt[sub] + take_place(s_fill, sub);
        const uint64_t res = (r.hash - lo_hash) - ((uint64_t)(sub * bm.sub_width[LANE_CFG]) << bm.sh);
        rkey = (res << rank_bits) | pidx;
        s_key[place] = rkey;
    }
    __syncthreads();
    uint32_t rank = 0, seg0 = 0;
    if (live) rank = rank_and_head(s_key, s_cnt[sub], s_cnt[sub + 1], rkey, rank_bits, seg0);
    __syncthreads();                      // every lane is done with s_key (= s_m0) and the counters (= s_m1, s_seg)
    if (live) {
        s_hash[rank] = r.hash; s_rid[rank] = r.rid; s_m0[rank] = r.m0; s_m1[rank] = r.m1;
        s_seg[rank] = (uint16_t)seg0;
    }
    __syncthreads();
    // ---- sorted position j = tid: head, mate-2 skip (sketch.rs:852), tag -------------------------------------------------
    const uint32_t j = tid;
    const uint32_t seg = live ? (uint32_t)s_seg[j] : 0u;
    const bool head = live && seg == j;
    const uint64_t rid = live ? s_rid[j] : 0ull;
    uint32_t* const s_tag = reinterpret_cast<uint32_t*>(lds.ab);   // (s_a | s_b are written after the marker test)
    bool skip = false;                    // a mate 2 whose mate 1 holds the k-mer too
    if (live) {
        if constexpr (PAIRED) skip = mate2_skipped(s_rid, seg, j);
        if constexpr (!filter && !no_dedup) s_tag[j] = (!skip && (rid & RID_MARKER_BIT)) ? marker_tags(s_m0[j], s_m1[j]) : 0u;
    }
    if constexpr (!filter && !no_dedup) __syncthreads();
    // ---- duplicate flag -------------------------------------------------------------------------------------------------
    bool dup = false;                     // would be dropped
    if (live && !skip && (rid & RID_MARKER_BIT)) {
        if constexpr (filter) {
            // the filter's answer (the bit a10_mark left in the record), unless this is the first of the k-mer in the walk
            dup = (rid & RID_A10_BIT) && !walk_first(s_rid, s_seg, n, j);
        } else if constexpr (!no_dedup) {
            const uint64_t a = s_m0[j], bb = s_m1[j];
            const bool hit = tag_scan_hit(s_tag, s_m0, s_m1, seg, j, a, bb);
            dup = j != seg && (hit || a == bb);
        }
    }
    const bool u = live && !skip && (no_dedup || !dup);            // would count
    // ---- counts (cut-off rule, sketch.rs:706) and rows --------------------------------------------------------------------
    uint32_t base_h, total_heads, total_removed;
    if constexpr (PAIRED) {
        // no cut-off: counted = would-count, ONE block scan of (would-count, heads, removed) packed 10+10+10 bits
        const bool removed = live && !skip && !u;
        uint32_t tot = 0;
        const uint32_t base = block_excl_sum<LANE_CAP>((u ? 1u : 0u) | (head ? 1u << 10 : 0u) | (removed ? 1u << 20 : 0u), s_wave, &tot);
        base_h = (base >> 10) & 0x3FFu;
        total_heads = (tot >> 10) & 0x3FFu;
        total_removed = tot >> 20;
        if (live) {
            s_b[j] = (uint16_t)(base & 0x3FFu);                    // Ec[j] = Eu[j]
            if (j + 1 == n) s_b[n] = (uint16_t)((base & 0x3FFu) + (u ? 1u : 0u));
        }
        __syncthreads();
    } else {
        // P = would-be-counted occurrences before j in its k-mer: counted from the cut-off on whatever the markers say
        uint32_t tot_uh = 0;
        const uint32_t base_uh = block_excl_sum<LANE_CAP>((u ? 1u : 0u) | (head ? 1u << 16 : 0u), s_wave, &tot_uh);
        base_h = base_uh >> 16;
        total_heads = tot_uh >> 16;
        if (live) s_a[j] = (uint16_t)(base_uh & 0xFFFFu);          // Eu[j]
        __syncthreads();
        bool c = false;
        if (live && !skip) c = ((uint32_t)s_a[j] - (uint32_t)s_a[seg] >= SINGLE_CUTOFF) ? true : u;
        const bool removed = live && !skip && !c;
        uint32_t tot_cr = 0;
        const uint32_t base_c = block_excl_sum<LANE_CAP>((c ? 1u : 0u) | (removed ? 1u << 16 : 0u), s_wave, &tot_cr) & 0xFFFFu;
        total_removed = tot_cr >> 16;
        if (live) {
            s_b[j] = (uint16_t)base_c;                             // Ec[j]
            if (j + 1 == n) s_b[n] = (uint16_t)(base_c + (c ? 1u : 0u));
        }
        __syncthreads();
    }
    if (head) {
        const uint32_t e = segment_end(s_seg, n, j);
        tmp_k[first + base_h] = s_hash[j];
        tmp_c[first + base_h] = (uint32_t)s_b[e] - (uint32_t)s_b[j];
    }
    if (tid == 0) { ra.n_distinct[b] = total_heads; ra.removed_b[b] = total_removed; }
}

// Marker-less samples (single-end; long reads or --no-dedup: sylph_sketch::n_plain): nothing is ever dropped, the table is the
// histogram of the hashes.  Same bucket, same sub-range sort as replay_bucket, on 8-byte hashes gathered through the permutation
// instead of 32-byte records (the gather is what bounds the replay: 65 B fetched per occurrence there); no records exist at all.
// Buckets above CAP go to the next configuration's list (large_list), above that to ovf_list — the host writes the records of
// the sample then (OccRec{hash, 0, 0, 0}) and sends those buckets the usual way.
template <int CAP, int RTPB>
__device__ __forceinline__ void count_bucket(const uint32_t b, const ReplayArgs& ra) {
    const uint64_t* __restrict__ hash = ra.hash;
    const uint32_t* __restrict__ perm = ra.perm;
    uint64_t* __restrict__ tmp_k = ra.tmp_k;
    uint32_t* __restrict__ tmp_c = ra.tmp_c;
    const BucketMap& bm = ra.bm;
    constexpr int ITEMS = CAP / RTPB;
    constexpr int CFG = cfg_of_cap(CAP);
    __shared__ uint64_t s_key[CAP], s_sorted[CAP];
    __shared__ uint32_t s_cnt[CAP + 1], s_mult[CAP];
    __shared__ __attribute__((aligned(8))) uint16_t s_fill[CAP];
    __shared__ uint32_t s_wave[RTPB / 64];
    const uint32_t tid = threadIdx.x;
    uint32_t first, n;
    if (!bucket_bounds(ra, b, first, n)) { if (tid == 0) atomicAdd(ra.overflow, 1u); return; }
    if (n == 0) return;
    if (n > (uint32_t)CAP) {
        if (tid == 0) queue_bucket((CAP < CAP_LARGE && n <= (uint32_t)CAP_LARGE) ? ra.large_list : ra.ovf_list, b);
        return;
    }
    const uint64_t lo_hash = bucket_lo_hash(b, bm.mult, bm.sh);      // (bm.composite: checked by the host)
    const uint32_t sub_mult = bm.sub_mult[CFG];
    uint64_t h[ITEMS];
    uint32_t sub[ITEMS], place[ITEMS];
#pragma unroll
    for (int q = 0; q < ITEMS; q++) {
        const uint32_t i = tid + q * RTPB;
        h[q] = i < n ? (perm ? hash[perm[first + i]] : hash[first + i]) : 0ull;      // perm == nullptr: `hash` is sorted by bucket already
    }
    for (uint32_t t = tid; t <= (uint32_t)CAP; t += RTPB) s_cnt[t] = 0;
    for (uint32_t t = tid; t < (uint32_t)CAP; t += RTPB) s_fill[t] = 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < ITEMS; q++) {
        const uint32_t i = tid + q * RTPB;
        sub[q] = 0;
        if (i < n) {
            sub[q] = sub_range_of((uint32_t)((h[q] - lo_hash) >> bm.sh), sub_mult, CAP);
            atomicAdd(&s_cnt[sub[q]], 1u);
        }
    }
    __syncthreads();
    scan_counters<CAP, RTPB>(s_cnt, s_cnt, s_wave);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < ITEMS; q++) {
        const uint32_t i = tid + q * RTPB;
        place[q] = 0;
        if (i < n) {
            place[q] = s_cnt[sub[q]] + take_place(s_fill, sub[q]);
            s_key[place[q]] = h[q];
        }
    }
    __syncthreads();
    // sorted position = start of the sub-range + smaller hashes in it + equal hashes placed before; the first of its equals
    // carries the k-mer's multiplicity
#pragma unroll
    for (int q = 0; q < ITEMS; q++) {
        const uint32_t i = tid + q * RTPB;
        if (i < n) {
            const uint32_t lo = s_cnt[sub[q]], hi = s_cnt[sub[q] + 1];
            uint32_t less = 0, eq = 0, eq_before = 0;
            for (uint32_t p = lo; p < hi; p++) {
                const uint64_t kp = s_key[p];
                less += kp < h[q] ? 1u : 0u;
                const uint32_t same = kp == h[q] ? 1u : 0u;
                eq += same;
                eq_before += (same && p < place[q]) ? 1u : 0u;
            }
            const uint32_t r = lo + less + eq_before;
            s_sorted[r] = h[q];
            s_mult[r] = eq_before == 0 ? eq : 0u;
        }
    }
    __syncthreads();
    const uint32_t items = (n + RTPB - 1) / RTPB, j0 = tid * items;
    uint32_t heads = 0;
    for (uint32_t t = 0; t < items; t++) {
        const uint32_t j = j0 + t;
        if (j >= n) break;
        heads += s_mult[j] ? 1u : 0u;
    }
    uint32_t total_heads = 0;
    uint32_t rh = block_excl_sum<RTPB>(heads, s_wave, &total_heads);
    for (uint32_t t = 0; t < items; t++) {
        const uint32_t j = j0 + t;
        if (j >= n) break;
        const uint32_t m = s_mult[j];
        if (m) { tmp_k[first + rh] = s_sorted[j]; tmp_c[first + rh] = m; rh++; }
    }
    if (tid == 0) { ra.n_distinct[b] = total_heads; ra.removed_b[b] = 0; }
}

}  // namespace
}  // namespace sylph
