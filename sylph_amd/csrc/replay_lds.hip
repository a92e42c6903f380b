// replay_lds.hip — finish() of a read-sketch session without device-wide sorts: bucket partition + in-LDS replay.
//
// FracMinHash survivors are uniformly distributed below the threshold (mm_hash64 is a bijection of canonical
// k-mers), so the top bits of the hash split the sample's occurrences into B buckets of nearly equal size (~96: nearly all of them
// at most 128, one occurrence per lane of the replay workgroup — replay_bucket_lane).
// The PARTITION (round 3: hand-written, four small kernels, no library sort, no memset dispatches) only moves 8-byte
// (bucket, occurrence index) pairs, in two levels: tiles of occurrences are histogrammed over <= 512 coarse hash ranges, a
// scan turns the (range x tile) counts into offsets, the pairs are scattered range by range, and one workgroup per coarse
// range finishes with a counting sort by bucket in LDS, which also yields the bucket offsets.  Neither level keeps the file
// order inside a bucket (ranks come from LDS atomics): the occurrence index IS the file order, and the replay workgroup
// re-establishes it for its ~128 occurrences with one rank loop.  The 32 B occurrence records never move: the replay gathers
// them through the permutation — from the session's dense arrays, or straight from the per-block slots the seeding kernel
// left them in when the sample came in one batch (no compaction pass at all).
// One workgroup then owns one bucket entirely in LDS: counting-rank sort by (hash, file order) -> k-mer segments in file
// order -> mate-2 skip, duplicate flags, cut-off and counts (the same data-parallel formulation of
// dup_removal_lsh_full_exact as sketch.hip, see its header) -> distinct (k-mer, count) pairs.  Buckets are ordered
// by hash, so concatenating their outputs gives the table in ascending k-mer order.
// A bucket beyond 1024 occurrences (a k-mer more than ~1000 deep) goes through the device-wide path of sketch.hip, as a
// small sample of its own.
#include "common.h"
#include "device_common.h"
#include "sketch_session.h"
#include "partition.h"

namespace sylph {
namespace {

// Three configurations of the same kernel template (the first carries a second, leaner body for buckets of up to 128: LANE_CAP).  Buckets of up to CAP_SMALL occurrences (all of them, for ordinary
// samples) run with 10 KiB of LDS per workgroup -> 16 workgroups = 32 wavefronts per CU, which is what hides the latency of
// this barrier- and gather-heavy kernel (with a single 512-slot configuration occupancy was 14 wavefronts and the kernel 1.4x
// slower).  Larger buckets, and buckets that hold a deep k-mer (SEG_LIMIT), are queued for the CAP_MID / CAP_LARGE
// configurations, which replace the scan over a k-mer's earlier occurrences by a hash table in LDS and are launched only
// when something was queued; only beyond CAP_LARGE does a bucket take the device-wide path.
#ifndef SYLPH_REPLAY_TPB
#define SYLPH_REPLAY_TPB 128
#endif
constexpr int CAP_SMALL = 256, RTPB_SMALL = SYLPH_REPLAY_TPB;
constexpr int CAP_MID = 512, RTPB_MID = 256;       // hashed marker test, ~31 KiB of LDS: 5 workgroups per CU
constexpr int CAP_LARGE = 1024, RTPB_LARGE = 256;   // hashed marker test, ~59 KiB of LDS: 2 workgroups per CU
constexpr int IDX_BITS = 10;         // arrival index inside a bucket (< CAP_LARGE)
// The marker test of the small configuration looks at every earlier occurrence of the k-mer: quadratic in a k-mer's coverage.
// A bucket holding a k-mer with SEG_LIMIT or more occurrences (a genome at ~100x and above) is handed to the medium / large
// configuration, whose marker test is a hash table in LDS: linear in the bucket size.
constexpr uint32_t SEG_LIMIT = 96;
constexpr uint32_t SINGLE_CUTOFF = 4;   // MAX_DEDUP_COUNT, constants.rs:14 (single-end; pairs have none)
// The one-occurrence-per-lane body (replay_bucket_lane): buckets of up to LANE_CAP occurrences, LANE_CAP threads, LANE_CAP
// sub-ranges — the fourth entry of BucketMap::sub_mult / sub_width / rank_bits.
constexpr int LANE_CAP = 128, LANE_CFG = 3;


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

// What the host reads back at the end of a pass: written by table_compact_kernel (`overflow`: by the replay), copied in one piece.
struct FinishTail {
    unsigned long long removed;  // duplicates dropped
    uint32_t overflow;           // buckets with inconsistent bounds (defensive)
    uint32_t n_seg;              // rows of the table
    uint32_t n_ovf, n_mid, n_large;   // heads of the three lists
    uint32_t verdict[2];         // deferred seeding verdict (reads.hip ReadsState: long_record, overflowing blocks)
    uint32_t a10_words[2];       // verdict of the filter dedup's partitioned pass (a10.hip)
    uint32_t n_found;            // occurrences the partition found: what a deferred batch's slots really hold
};
static_assert(sizeof(FinishTail) == 48, "tail block");

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
    const uint32_t* __restrict__ boff = ra.boff;
    uint64_t* __restrict__ tmp_k = ra.tmp_k;
    uint32_t* __restrict__ tmp_c = ra.tmp_c;
    uint32_t* __restrict__ n_distinct = ra.n_distinct;
    uint32_t* __restrict__ mid_list = ra.mid_list;
    const int paired = ra.paired, dbg_stage = ra.dbg_stage;
    const uint32_t cutoff = ra.cutoff;
    const BucketMap& bm = ra.bm;
    constexpr int ITEMS = CAP / RTPB;     // records per lane
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
    const uint32_t nv = *ra.p_nv;
    const uint32_t first = boff[b], last = boff[b + 1];
    const uint32_t n = last - first;
    if (last > nv || first > last) { if (tid == 0) atomicAdd(ra.overflow, 1u); return; }   // defensive: inconsistent bounds
    if (n == 0) return;                   // (n_distinct was zeroed by the host)
    // too large for this configuration: queue it for the large one (large_list: [0] = count, [1..] = buckets), or for the
    // host, which sends the occurrences of such buckets through the device-wide path (ovf_list, same layout)
    if (n > CAP) {
        if (tid == 0) {
            uint32_t* list = (CAP < CAP_MID && n <= (uint32_t)CAP_MID) ? mid_list : (CAP < CAP_LARGE && n <= (uint32_t)CAP_LARGE) ? ra.large_list : ra.ovf_list;
            list[1 + atomicAdd(&list[0], 1u)] = b;
        }
        return;
    }
    // ---- gather (through the partition permutation, one 32 B sector per occurrence) + sort by (hash, file order) -------
    uint64_t* s_key = s_m0;               // keys live in s_m0 until the sorted records are written
    const bool composite = bm.composite != 0;
    const uint64_t lo_hash = composite ? bucket_lo_hash(b, bm.mult, bm.sh) : 0ull;
    OccRec r[ITEMS];
    uint32_t pidx[ITEMS], rank[ITEMS];
    // 256 slots: the rank loops below also count the members with a smaller HASH — the sorted position of the k-mer's first
    // occurrence, i.e. its segment head (equal hashes share a sub-range) — so that no scan has to find the heads afterwards
    constexpr bool SEG_DIRECT = CAP == CAP_SMALL;
    uint32_t seg0[ITEMS];
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
        const uint32_t sub_mult = bm.sub_mult[CAP == CAP_SMALL ? 0 : CAP == CAP_MID ? 1 : 2];
        uint32_t sub[ITEMS];
        constexpr int CFG = CAP == CAP_SMALL ? 0 : CAP == CAP_MID ? 1 : 2;
        const int rank_bits = bm.rank_bits[CFG];
        // hashed configurations (deep buckets): lowest and highest hash of every sub-range (s_hash / s_rid are free until the
        // sorted records are written) — a sub-range whose two are equal holds ONE k-mer, see the second level below
        constexpr bool TWO_LEVEL = CAP != CAP_SMALL;
        unsigned long long* const s_min = reinterpret_cast<unsigned long long*>(s_hash);
        unsigned long long* const s_max = reinterpret_cast<unsigned long long*>(s_rid);
        for (uint32_t t = tid; t <= (uint32_t)CAP; t += RTPB) s_cnt[t] = 0;
        // (the placement's counters too: s_seg is not written before the segments)
        for (uint32_t t = tid; t < (uint32_t)CAP / 2; t += RTPB) reinterpret_cast<uint32_t*>(s_seg)[t] = 0;
        if constexpr (TWO_LEVEL)
            for (uint32_t t = tid; t < (uint32_t)CAP; t += RTPB) { s_min[t] = ~0ull; s_max[t] = 0ull; }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < ITEMS; q++) {
            const uint32_t i = tid + q * RTPB;
            sub[q] = 0;
            if (i < n) {
                sub[q] = sub_range_of((uint32_t)((r[q].hash - lo_hash) >> bm.sh), sub_mult, CAP);          // (the distance is < bm.range_hs)
                atomicAdd(&s_cnt[sub[q]], 1u);
                if constexpr (TWO_LEVEL) {
                    atomicMin(&s_min[sub[q]], (unsigned long long)r[q].hash);
                    atomicMax(&s_max[sub[q]], (unsigned long long)r[q].hash);
                }
            }
        }
        __syncthreads();
        {   // s_cnt[t] = start of sub-range t, s_cnt[CAP] = n
            const bool deep = scan_counters<CAP, RTPB>(s_cnt, s_cnt, s_wave) >= SEG_LIMIT;
            // A k-mer SEG_LIMIT deep fills its sub-range that far (equal hashes share a sub-range): such a bucket is for the
            // hashed marker test of the next configuration — pass it on now, before the placement, the ranking (as long as the k-mer
            // is deep, per occurrence) and the segment scans are spent on it here.  (A sub-range that full without a deep k-mer
            // does not happen with ~0.5 occurrences per sub-range; the next configuration is right for any bucket it can hold.)
            if constexpr (CAP == CAP_SMALL) {
                if (__syncthreads_or(deep && !no_dedup)) {
                    if (tid == 0) mid_list[1 + atomicAdd(&mid_list[0], 1u)] = b;
                    return;
                }
            } else
                __syncthreads();
        }
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
        if constexpr (TWO_LEVEL) {
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
                    uint32_t smaller = 0;
                    if constexpr (SEG_DIRECT) {
                        // (key < hkey <=> smaller hash: the index sits below rank_bits)
                        const uint64_t hkey = rkey[q] & ~((1ull << rank_bits) - 1ull);
                        uint32_t below = 0;
                        for (uint32_t p = lo; p < hi; p++) {
                            const uint64_t kp = s_key[p];
                            smaller += kp < rkey[q] ? 1u : 0u;
                            below += kp < hkey ? 1u : 0u;
                        }
                        seg0[q] = lo + below;
                    } else {
                        for (uint32_t p = lo; p < hi; p++) smaller += s_key[p] < rkey[q] ? 1u : 0u;
                    }
                    rank[q] = lo + smaller;
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
                        if constexpr (SEG_DIRECT) below += kp < r[q].hash ? 1u : 0u;
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
                    if constexpr (SEG_DIRECT) seg0[q] += kj < r[q].hash ? 1u : 0u;
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
            if constexpr (SEG_DIRECT) s_seg[d] = (uint16_t)seg0[q];
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
    if constexpr (SEG_DIRECT) {
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
    constexpr bool HASHED = CAP != CAP_SMALL;
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
                if (tid == 0) mid_list[1 + atomicAdd(&mid_list[0], 1u)] = b;
                return;
            }
        }
    }
    // DEDUP_FILTER: `*c > 0` (sketch.rs:749, :756) = an occurrence of the k-mer went through the dedup before this one.  The walk hands
    // over a record's seeds in EMISSION order (the rank bits of the rid; lane-interleaved for the AVX2 routine), the segment lists them
    // by position: the first of the walk is the lowest rank among the segment's leading occurrences of the head's record — the head
    // itself unless the read repeats the k-mer (a tandem repeat inside one read).  (None of those is a skipped mate 2: the mate-1
    // occurrence that would make it one belongs to an earlier record.)
    auto walk_first = [&](uint32_t j) {
        const uint32_t s0 = s_seg[j];
        const uint64_t rec0 = s_rid[s0] & RID_MASK, rj = s_rid[j];
        if ((rj & RID_MASK) != rec0) return false;
        const uint64_t rank_j = (rj >> RID_RANK_SHIFT) & RID_RANK_MAX;
        for (uint32_t q = s0; q < n && (uint32_t)s_seg[q] == s0 && (s_rid[q] & RID_MASK) == rec0; q++)
            if (q != j && ((s_rid[q] >> RID_RANK_SHIFT) & RID_RANK_MAX) < rank_j) return false;
        return true;
    };
    uint32_t* const s_tag = reinterpret_cast<uint32_t*>(s_ab);           // CAP words: fits the 2 x (CAP + 2) halfwords of s_a | s_b, which are written later
    // ---- mate-2 skip (sketch.rs:852) and duplicate flags ----------------------------------------------------------
    for (uint32_t t = 0; t < items; t++) {
        const uint32_t j = j0 + t;
        if (j >= n) break;
        uint8_t fl = 0;
        if (paired) {
            const uint64_t rec = s_rid[j] & RID_MASK;
            if (rec & 1) {
                const uint32_t s0 = s_seg[j];
                for (uint32_t q = j; q > s0;) {
                    q--;
                    const uint64_t rq = s_rid[q] & RID_MASK;
                    if ((rq >> 1) != (rec >> 1)) break;
                    if ((rq & 1) == 0) { fl = 1; break; }
                }
            }
        }
        s_fl[j] = fl;
        if constexpr (CAP == CAP_SMALL)
            s_tag[j] = (!fl && (s_rid[j] & RID_MARKER_BIT)) ? (marker_tag(s_m0[j]) | (marker_tag(s_m1[j]) << 16)) : 0u;
    }
    __syncthreads();
    uint32_t my_u = 0;
    uint8_t ubits = 0;
    if constexpr (HASHED) {
        // Marker test through a hash table in LDS.  Every processed occurrence with markers enters both of them under the key
        // (k-mer segment, marker value); a slot belongs to the first entry that claims it (owner entry in the high half of the
        // word, never changes) and keeps the smallest sorted position among the entries with its key in the low half.  An
        // occurrence is a duplicate when one of its two keys was entered from an earlier position (sketch.rs:709-722: markers
        // go into the set whether the occurrence is then counted or dropped), or when its two markers are equal — and it is
        // not the first of its k-mer: the head of a segment is never a skipped mate 2 (the mate-1 occurrence that would make
        // it one precedes it in the segment), so "a processed occurrence precedes j" is simply "j is not the head".
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
        for (uint32_t t = 0; t < items; t++) {
            const uint32_t j = j0 + t;
            if (j >= n) break;
            uint8_t fl = s_fl[j];
            if (!fl && !no_dedup && (s_rid[j] & RID_MARKER_BIT) && (filter || j != (uint32_t)s_seg[j])) {
                if (filter) {      // sketch.rs:747-760: the filter's answers, `*c > 0` = not the first of the k-mer in the walk
                    if ((s_rid[j] & RID_A10_BIT) && !walk_first(j)) fl |= 2;
                } else {
                    const bool hit = (s_tab[s_slot[2 * j]] & 0xFFFFu) < j || (s_tab[s_slot[2 * j + 1]] & 0xFFFFu) < j;
                    if (hit || s_m0[j] == s_m1[j]) fl |= 2;
                }
            }
            const bool u = !(fl & 1) && (no_dedup || !(fl & 2));
            if (u) { my_u++; ubits |= (uint8_t)(1u << t); }
            s_fl[j] = fl;
        }
    } else {
        for (uint32_t t = 0; t < items; t++) {
            const uint32_t j = j0 + t;
            if (j >= n) break;
            uint8_t fl = s_fl[j];
            if (filter) {
                if (!fl && (s_rid[j] & RID_MARKER_BIT) && (s_rid[j] & RID_A10_BIT) && !walk_first(j)) fl |= 2;
            } else if (!fl && !no_dedup && (s_rid[j] & RID_MARKER_BIT)) {
                const uint64_t a = s_m0[j], bb = s_m1[j];
                bool hit = false;
                // Round 5: the scan over the k-mer's earlier occurrences reads ONE 32-bit word per occurrence — two 15-bit tags of its
                // markers, 0 for an occurrence that put nothing into the set (skipped mate 2, no markers) — and looks at the 16 bytes of
                // markers only where a tag matches (a real duplicate, or 4 x 2^-15 by chance).  Before: flag byte + record id + both
                // markers (25 bytes of LDS, four 64-bit compares) per earlier occurrence: the loop was a third of this kernel for a
                // community with 30x genomes in it.  ("A processed occurrence precedes j" is "j is not the head": the head of a
                // segment is never a skipped mate 2.)
                const uint32_t ta = marker_tag(a) * 0x00010001u, tb = marker_tag(bb) * 0x00010001u;
                for (uint32_t q = s_seg[j]; q < j; q++) {
                    const uint32_t w = s_tag[q], za = w ^ ta, zb = w ^ tb;
                    if ((((za - 0x00010001u) & ~za) | ((zb - 0x00010001u) & ~zb)) & 0x80008000u) {     // a zero halfword in either
                        const uint64_t x = s_m0[q], y = s_m1[q];
                        if (w && (x == a || y == a || x == bb || y == bb)) { hit = true; break; }
                    }
                }
                if (j != (uint32_t)s_seg[j] && (hit || a == bb)) fl |= 2;
            }
            const bool u = !(fl & 1) && (no_dedup || !(fl & 2));
            if (u) { my_u++; ubits |= (uint8_t)(1u << t); }
            s_fl[j] = fl;   // NB: later lanes only read bit0 of earlier positions, which does not change here
        }
    }
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
                // segment end = next head or n: walk (segments here are shorter than SEG_LIMIT)
                uint32_t e = j + 1;
                while (e < n && s_seg[e] == j) e++;
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
// per lane: the same steps in the same order as replay_bucket<256, 128> (gather with both loads in flight, sub-range count, counter
// scan, hand-off of a bucket with a deep k-mer, placement, the rank loop that also yields the segment head, sorted write, mate-2 rule,
// tags, marker test, one packed block scan for pairs / two for single-end, rows), but a lane's sorted position is its thread number:
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
    {   // s_cnt[t] = start of sub-range t, s_cnt[LANE_CAP] = n; a k-mer SEG_LIMIT deep fills its sub-range that far: the bucket is
        // for the hashed marker test of the 512-slot configuration (as in replay_bucket, at the same point)
        const bool deep = scan_counters<LANE_CAP, LANE_CAP>(s_cnt, s_cnt, s_wave) >= SEG_LIMIT;
        if constexpr (!no_dedup) {
            if (__syncthreads_or(deep)) {
                if (tid == 0) ra.mid_list[1 + atomicAdd(&ra.mid_list[0], 1u)] = b;
                return;
            }
        } else
            __syncthreads();
    }
    uint64_t rkey = 0;
    if (live) {
        const uint32_t place = s_cnt[sub] + take_place(s_fill, sub);
        const uint64_t res = (r.hash - lo_hash) - ((uint64_t)(sub * bm.sub_width[LANE_CFG]) << bm.sh);
        rkey = (res << rank_bits) | pidx;
        s_key[place] = rkey;
    }
    __syncthreads();
    uint32_t rank = 0, seg0 = 0;
    if (live) {
        // sorted position = start of the sub-range + members with a smaller key; segment head = start + members with a smaller
        // HASH (key < hkey <=> smaller hash: the index sits below rank_bits)
        const uint32_t lo = s_cnt[sub], hi = s_cnt[sub + 1];
        const uint64_t hkey = rkey & ~((1ull << rank_bits) - 1ull);
        uint32_t smaller = 0, below = 0;
        for (uint32_t p = lo; p < hi; p++) {
            const uint64_t kp = s_key[p];
            smaller += kp < rkey ? 1u : 0u;
            below += kp < hkey ? 1u : 0u;
        }
        rank = lo + smaller;
        seg0 = lo + below;
    }
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
        if constexpr (PAIRED) {
            const uint64_t rec = rid & RID_MASK;
            if (rec & 1) {
                for (uint32_t q = j; q > seg;) {
                    q--;
                    const uint64_t rq = s_rid[q] & RID_MASK;
                    if ((rq >> 1) != (rec >> 1)) break;
                    if ((rq & 1) == 0) { skip = true; break; }
                }
            }
        }
        if constexpr (!filter && !no_dedup)
            s_tag[j] = (!skip && (rid & RID_MARKER_BIT)) ? (marker_tag(s_m0[j]) | (marker_tag(s_m1[j]) << 16)) : 0u;
    }
    if constexpr (!filter && !no_dedup) __syncthreads();
    // ---- duplicate flag -------------------------------------------------------------------------------------------------
    bool dup = false;                     // would be dropped
    if (live && !skip && (rid & RID_MARKER_BIT)) {
        if constexpr (filter) {
            // the filter's answer (the bit a10_mark left in the record), unless this is the first of the k-mer in the walk: the lowest
            // emission rank among the segment's leading occurrences of the head's record (see replay_bucket)
            if (rid & RID_A10_BIT) {
                const uint64_t rec0 = s_rid[seg] & RID_MASK;
                bool walk_first = (rid & RID_MASK) == rec0;
                if (walk_first) {
                    const uint64_t rank_j = (rid >> RID_RANK_SHIFT) & RID_RANK_MAX;
                    for (uint32_t q = seg; q < n && (uint32_t)s_seg[q] == seg && (s_rid[q] & RID_MASK) == rec0; q++)
                        if (q != j && ((s_rid[q] >> RID_RANK_SHIFT) & RID_RANK_MAX) < rank_j) { walk_first = false; break; }
                }
                dup = !walk_first;
            }
        } else if constexpr (!no_dedup) {
            // the k-mer's earlier occurrences, one word of two 15-bit tags each; the markers themselves only where a tag matches
            const uint64_t a = s_m0[j], bb = s_m1[j];
            bool hit = false;
            const uint32_t ta = marker_tag(a) * 0x00010001u, tb = marker_tag(bb) * 0x00010001u;
            for (uint32_t q = seg; q < j; q++) {
                const uint32_t w = s_tag[q], za = w ^ ta, zb = w ^ tb;
                if ((((za - 0x00010001u) & ~za) | ((zb - 0x00010001u) & ~zb)) & 0x80008000u) {     // a zero halfword in either
                    const uint64_t x = s_m0[q], y = s_m1[q];
                    if (w && (x == a || y == a || x == bb || y == bb)) { hit = true; break; }
                }
            }
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
        // segment end = next head or n: walk (segments here are shorter than SEG_LIMIT)
        uint32_t e = j + 1;
        while (e < n && s_seg[e] == j) e++;
        tmp_k[first + base_h] = s_hash[j];
        tmp_c[first + base_h] = (uint32_t)s_b[e] - (uint32_t)s_b[j];
    }
    if (tid == 0) { ra.n_distinct[b] = total_heads; ra.removed_b[b] = total_removed; }
}

// LANE: which instance of the lane body the kernel carries beside replay_bucket — LANE_OFF (none: replay_bucket runs every bucket, as
// before round 10) or lane_mode(paired, dedup).  The choice per bucket is uniform over the workgroup: at most LANE_CAP occurrences,
// consistent bounds, composite keys with a one-word ranking key -> the lane body; everything else (129 ... 256 occurrences, larger
// ones queued, inconsistent bounds counted) -> replay_bucket, in the same launch and the same LDS.
constexpr int LANE_OFF = -1;
constexpr int lane_mode(bool paired, int dedup) { return (paired ? 1 : 0) | (dedup << 1); }
// (num_sgpr: two bodies in one kernel take 101 scalar registers when left alone, one more than 8 wavefronts per SIMD leave each — and
//  with the LDS admitting 15 workgroups per CU, 7.5 wavefronts per SIMD, the eighth counts; held to 100 nothing spills)
template <int CAP, int RTPB, int LANE = LANE_OFF>
__global__ __launch_bounds__(RTPB) __attribute__((amdgpu_num_sgpr(100))) void bucket_replay_kernel(ReplayArgs ra) {
    __shared__ ReplayLds<CAP, RTPB> lds;
    if constexpr (LANE != LANE_OFF) {
        static_assert(CAP == CAP_SMALL && RTPB == LANE_CAP, "the lane body shares the 256-slot configuration's workgroup");
        const uint32_t first = ra.boff[blockIdx.x], last = ra.boff[blockIdx.x + 1];
        if (first < last && last <= *ra.p_nv && last - first <= (uint32_t)LANE_CAP && ra.bm.composite && ra.bm.rank_bits[LANE_CFG]) {
            replay_bucket_lane<(LANE & 1) != 0, (LANE >> 1)>(blockIdx.x, first, last - first, ra, lds);
            return;
        }
    }
    replay_bucket<CAP, RTPB>(blockIdx.x, ra, lds);
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
    const uint32_t* __restrict__ boff = ra.boff;
    uint64_t* __restrict__ tmp_k = ra.tmp_k;
    uint32_t* __restrict__ tmp_c = ra.tmp_c;
    const BucketMap& bm = ra.bm;
    constexpr int ITEMS = CAP / RTPB;
    __shared__ uint64_t s_key[CAP], s_sorted[CAP];
    __shared__ uint32_t s_cnt[CAP + 1], s_mult[CAP];
    __shared__ __attribute__((aligned(8))) uint16_t s_fill[CAP];
    __shared__ uint32_t s_wave[RTPB / 64];
    const uint32_t tid = threadIdx.x;
    const uint32_t nv = *ra.p_nv;
    const uint32_t first = boff[b], last = boff[b + 1];
    const uint32_t n = last - first;
    if (last > nv || first > last) { if (tid == 0) atomicAdd(ra.overflow, 1u); return; }
    if (n == 0) return;
    if (n > (uint32_t)CAP) {
        if (tid == 0) {
            uint32_t* list = (CAP < CAP_LARGE && n <= (uint32_t)CAP_LARGE) ? ra.large_list : ra.ovf_list;
            list[1 + atomicAdd(&list[0], 1u)] = b;
        }
        return;
    }
    const uint64_t lo_hash = bucket_lo_hash(b, bm.mult, bm.sh);      // (bm.composite: checked by the host)
    const uint32_t sub_mult = bm.sub_mult[CAP == CAP_SMALL ? 0 : CAP == CAP_MID ? 1 : 2];
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
template <int CAP, int RTPB>
__global__ __launch_bounds__(RTPB) void bucket_count_kernel(ReplayArgs ra) {
    count_bucket<CAP, RTPB>(blockIdx.x, ra);
}
// the list-driven configurations: a fixed, small grid walks the (usually empty) list of buckets an earlier configuration queued
template <int CAP, int RTPB>
__global__ __launch_bounds__(RTPB) void bucket_count_list_kernel(ReplayArgs ra, const uint32_t* __restrict__ my_list) {
    const uint32_t n_listed = my_list[0];
    for (uint32_t i = blockIdx.x; i < n_listed; i += gridDim.x) {
        count_bucket<CAP, RTPB>(my_list[1 + i], ra);
        __syncthreads();
    }
}
template <int CAP, int RTPB>
__global__ __launch_bounds__(RTPB) void bucket_replay_list_kernel(ReplayArgs ra, const uint32_t* __restrict__ my_list) {
    const uint32_t n_listed = my_list[0];
    __shared__ ReplayLds<CAP, RTPB> lds;
    for (uint32_t i = blockIdx.x; i < n_listed; i += gridDim.x) {
        replay_bucket<CAP, RTPB>(my_list[1 + i], ra, lds);
        __syncthreads();   // the LDS arrays are reused by the next bucket
    }
}

// Table offsets in two levels, no library scan: workgroup w scans the 1024 buckets of its chunk — d_loc[b] = table rows of the
// chunk's buckets before b — and leaves the chunk's row total and removed total; the compaction kernel adds the chunk totals
// before w (at most 256 of them: B <= 2^18 on this path).
constexpr uint32_t SCAN_CHUNK = 1024;
__global__ __launch_bounds__(SCAN_CHUNK) void table_scan_kernel(const uint32_t* __restrict__ n_distinct, const uint32_t* __restrict__ removed_b,
                                                                uint32_t B, uint32_t ipt, uint32_t* __restrict__ d_loc,
                                                                uint32_t* __restrict__ chunk_rows, unsigned long long* __restrict__ chunk_removed) {
    // a workgroup scans a chunk of SCAN_CHUNK * ipt buckets, every lane `ipt` consecutive ones (ipt = 1 up to 2^18 buckets; a
    // long-read sample at c = 100 has 4e5: at most 256 chunks whatever B, so that the second level fits one workgroup's LDS)
    __shared__ uint32_t s_wave[SCAN_CHUNK / 64];
    __shared__ unsigned long long s_rem[SCAN_CHUNK / 64];
    const uint32_t b0 = (blockIdx.x * SCAN_CHUNK + threadIdx.x) * ipt, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t v = 0;
    unsigned long long rem = 0;
    for (uint32_t i = 0; i < ipt && b0 + i < B; i++) { v += n_distinct[b0 + i]; rem += removed_b[b0 + i]; }
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= (uint32_t)d) x += y;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) rem += __shfl_xor(rem, d);
    if (lane == 63) s_wave[wave] = x;
    if (lane == 0) s_rem[wave] = rem;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (uint32_t w = 0; w < SCAN_CHUNK / 64; w++) { const uint32_t t = s_wave[w]; if (w < wave) base += t; tot += t; }
    uint32_t run = base + x - v;
    for (uint32_t i = 0; i < ipt && b0 + i < B; i++) { d_loc[b0 + i] = run; run += n_distinct[b0 + i]; }
    if (threadIdx.x == 0) {
        unsigned long long r = 0;
        for (uint32_t w = 0; w < SCAN_CHUNK / 64; w++) r += s_rem[w];
        chunk_rows[blockIdx.x] = tot;
        chunk_removed[blockIdx.x] = r;
    }
}
// out[rows before bucket b + i] = tmp[boff[b] + i] for i < n_distinct[b]; a workgroup walks buckets with its four wavefronts
// (one bucket holds ~50 rows).  Also fills the tail block the host reads (FinishTail).
__global__ __launch_bounds__(256) void table_compact_kernel(const uint64_t* __restrict__ tmp_k, const uint32_t* __restrict__ tmp_c,
                                                            const uint32_t* __restrict__ boff, const uint32_t* __restrict__ d_loc,
                                                            const uint32_t* __restrict__ chunk_rows, const unsigned long long* __restrict__ chunk_removed,
                                                            const uint32_t* __restrict__ n_distinct, uint32_t B, uint32_t ipt,
                                                            uint64_t* __restrict__ out_k, uint32_t* __restrict__ out_c,
                                                            const uint32_t* __restrict__ ovf_list, const uint32_t* __restrict__ mid_list,
                                                            const uint32_t* __restrict__ large_list, int skip_if_listed,
                                                            FinishTail* __restrict__ tail, const uint32_t* __restrict__ verdict,
                                                            const uint32_t* __restrict__ a10_words, const uint32_t* __restrict__ p_nv) {
    __shared__ uint32_t s_base[257];
    __shared__ uint32_t s_wave[4];
    __shared__ unsigned long long s_rem[4];
    const uint32_t chunk = SCAN_CHUNK * ipt, n_chunks = (B + chunk - 1) / chunk;        // <= 256: one chunk total per lane
    {
        const uint32_t v = threadIdx.x < n_chunks ? chunk_rows[threadIdx.x] : 0u;
        uint32_t tot = 0;
        const uint32_t ex = block_excl_sum<256>(v, s_wave, &tot);
        if (threadIdx.x < n_chunks) s_base[threadIdx.x] = ex;
        if (threadIdx.x == 0) s_base[n_chunks] = tot;
        if (blockIdx.x == 0) {                                                       // the tail block, once
            unsigned long long rem = threadIdx.x < n_chunks ? chunk_removed[threadIdx.x] : 0ull;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) rem += __shfl_xor(rem, d);
            if ((threadIdx.x & 63) == 0) s_rem[threadIdx.x >> 6] = rem;
            __syncthreads();
            if (threadIdx.x == 0) {
                tail->removed = s_rem[0] + s_rem[1] + s_rem[2] + s_rem[3];
                tail->n_seg = tot; tail->n_ovf = ovf_list[0]; tail->n_mid = mid_list[0]; tail->n_large = large_list[0];
                // the deferred seeding verdict and the filter pass's verdict words ride in the same block: one copy
                tail->verdict[0] = verdict ? verdict[0] : 0u; tail->verdict[1] = verdict ? verdict[1] : 0u;
                tail->a10_words[0] = a10_words ? a10_words[0] : 0u; tail->a10_words[1] = a10_words ? a10_words[1] : 0u;
                tail->n_found = *p_nv;
            }
        }
    }
    __syncthreads();
    // buckets are still waiting for the list-driven configurations: the host will come back after running them (a long-read
    // table has tens of millions of rows: copying it twice would cost more than the configurations themselves)
    if (skip_if_listed && (mid_list[0] | large_list[0])) return;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t b = blockIdx.x * 4 + wave; b < B; b += gridDim.x * 4) {
        const uint32_t n = n_distinct[b], s0 = boff[b], d = s_base[b / chunk] + d_loc[b];
        for (uint32_t i = lane; i < n; i += 64) { out_k[d + i] = tmp_k[s0 + i]; out_c[d + i] = tmp_c[s0 + i]; }
    }
}
// ---- buckets beyond the large configuration: their occurrences go through the device-wide path as one small sample --------
// sub_off[i] = occurrences of the listed buckets before bucket i (single workgroup; the list is short); sub_off[m] = total
__global__ __launch_bounds__(1024) void ovf_offsets_kernel(const uint32_t* __restrict__ ovf_list, const uint32_t* __restrict__ boff,
                                                           uint32_t* __restrict__ sub_off) {
    __shared__ uint32_t s_part[1024];
    const uint32_t m = ovf_list[0], tid = threadIdx.x;
    const uint32_t per = (m + 1023) / 1024;
    uint32_t sum = 0;
    for (uint32_t i = tid * per; i < min(m, (tid + 1) * per); i++) { const uint32_t b = ovf_list[1 + i]; sum += boff[b + 1] - boff[b]; }
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (uint32_t t = 0; t < 1024; t++) { const uint32_t v = s_part[t]; s_part[t] = run; run += v; }
        sub_off[m] = run;
    }
    __syncthreads();
    uint32_t run = s_part[tid];
    for (uint32_t i = tid * per; i < min(m, (tid + 1) * per); i++) {
        const uint32_t b = ovf_list[1 + i];
        sub_off[i] = run;
        run += boff[b + 1] - boff[b];
    }
}

// the occurrence indices of listed bucket i -> sub_idx[sub_off[i] ..): sorted afterwards, they are the listed buckets'
// occurrences in FILE order (what the device-wide path expects of its input)
__global__ __launch_bounds__(256) void ovf_indices_kernel(const uint32_t* __restrict__ ovf_list, const uint32_t* __restrict__ sub_off,
                                                          const uint32_t* __restrict__ boff, const uint32_t* __restrict__ perm,
                                                          uint32_t* __restrict__ sub_idx) {
    const uint32_t b = ovf_list[1 + blockIdx.x], first = boff[b], n = boff[b + 1] - first, o = sub_off[blockIdx.x];
    for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) sub_idx[o + j] = perm[first + j];
}
__global__ __launch_bounds__(256) void ovf_gather_kernel(const uint32_t* __restrict__ sorted_idx, uint32_t n, const OccRec* __restrict__ recs,
                                                         uint64_t* __restrict__ sub_hash, OccRec* __restrict__ sub_recs) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const OccRec r = recs[sorted_idx[j]];
    sub_hash[j] = r.hash;
    sub_recs[j] = r;
}

// the (k-mer, count) rows the device-wide path produced for listed bucket i go to the bucket's slots of the temporary table
__global__ __launch_bounds__(256) void ovf_patch_kernel(const uint32_t* __restrict__ ovf_list, BucketMap bm,
                                                        const uint64_t* __restrict__ sub_k, const uint32_t* __restrict__ sub_c,
                                                        uint32_t n_sub_out, const uint32_t* __restrict__ boff,
                                                        uint64_t* __restrict__ tmp_k, uint32_t* __restrict__ tmp_c,
                                                        uint32_t* __restrict__ n_distinct) {
    const uint32_t b = ovf_list[1 + blockIdx.x];
    auto lower = [&](uint64_t key) {   // first row with k-mer >= key
        uint32_t lo = 0, hi = n_sub_out;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (sub_k[mid] < key) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    // rows of bucket b = rows with k-mer in [smallest hash of bucket b, smallest hash of bucket b + 1) (inverse of bucket_of)
    __shared__ uint32_t s_lo, s_hi;
    if (threadIdx.x == 0) {
        s_lo = lower(bucket_lo_hash(b, bm.mult, bm.sh));
        s_hi = (b + 1 < bm.B) ? lower(bucket_lo_hash(b + 1, bm.mult, bm.sh)) : n_sub_out;
    }
    __syncthreads();
    const uint32_t lo = s_lo, n = s_hi - s_lo, d = boff[b];
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) { tmp_k[d + i] = sub_k[lo + i]; tmp_c[d + i] = sub_c[lo + i]; }
    if (threadIdx.x == 0) n_distinct[b] = n;
}

// The 256-slot launch: the instance that carries the lane body for the sample's mode (pairs or single-end, exact set or filter —
// the modes a sample can come in by default or by one flag); any other combination, a build with another workgroup size and the
// stage cuts of SYLPH_REPLAY_STAGE (which the lane body does not have) take replay_bucket alone.
void launch_replay(sylph_ctx* ctx, uint32_t B, const ReplayArgs& ra, bool paired, bool stage_cut) {
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(B), dim3(RTPB_SMALL), 0, ctx->stream, ra); };
    if constexpr (RTPB_SMALL == LANE_CAP) {
        if (!stage_cut) {
            if (paired && ra.dedup == DEDUP_EXACT) return go(bucket_replay_kernel<CAP_SMALL, RTPB_SMALL, lane_mode(true, DEDUP_EXACT)>);
            if (paired && ra.dedup == DEDUP_FILTER) return go(bucket_replay_kernel<CAP_SMALL, RTPB_SMALL, lane_mode(true, DEDUP_FILTER)>);
            if (!paired && ra.dedup == DEDUP_EXACT) return go(bucket_replay_kernel<CAP_SMALL, RTPB_SMALL, lane_mode(false, DEDUP_EXACT)>);
        }
    }
    go(bucket_replay_kernel<CAP_SMALL, RTPB_SMALL>);
}
// Which body a launch_replay of this map sends a bucket of n occurrences to (the kernel's own test, for the road counters)
bool lane_road(const BucketMap& bm, uint32_t n, bool paired, int dedup, bool stage_cut) {
    const bool instance = RTPB_SMALL == LANE_CAP && !stage_cut && (dedup == DEDUP_EXACT || (paired && dedup == DEDUP_FILTER));
    return instance && n >= 1 && n <= (uint32_t)LANE_CAP && bm.composite && bm.rank_bits[LANE_CFG];
}

uint32_t grid_of(uint64_t n, uint32_t tpb = 256) { return (uint32_t)((n + tpb - 1) / tpb); }

}  // namespace

bool finish_bucketed(sylph_sketch* sk) {
    sylph_ctx* ctx = sk->ctx;
    const bool slotted = sk->pend.live;                // the sample's one batch, still in its slots (reads.hip)
    // deferred verdict (sketch_session.h PendingSlots): the number of occurrences is not known on the host — geometry from the
    // expectation, capacities from the upper bound, every count the kernels need from device memory, the verdict read with the tail
    const bool deferred = slotted && sk->pend.deferred;
    const uint32_t n_cap = slotted ? sk->pend.n : (uint32_t)sk->n_occ;      // what the arrays must hold
    const uint32_t n_all = deferred ? std::max<uint32_t>(1, sk->pend.n_expect) : n_cap;
    sk->n_out = 0;
    sk->dup_removed = 0;
    if (n_cap == 0) return true;
    if (sk->c < 2) return false;   // c = 1: valid hashes reach the top bit that marks invalid occurrences
    // bucket geometry: B = n / TARGET equal hash ranges (see BucketMap)
    const uint64_t thr = UINT64_MAX / (uint64_t)sk->c;
    const uint32_t TARGET = ctx->bucket_target;
    const uint32_t B = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, n_all / TARGET), 1u << 24);
    BucketMap bm;
    bm.sh = key_shift(sk->c);
    const uint64_t hs_max = thr >> bm.sh;                              // hashes are < thr
    bm.mult = (uint32_t)std::min<uint64_t>(0xFFFFFFFFull, ((uint64_t)B << 32) / (hs_max + 1));
    bm.B = B;
    bm.inv_mult = bm.mult > 1 ? (uint64_t)(((unsigned __int128)1 << 64) / bm.mult) : ~0ull;
    // widest bucket in hs units is ceil(2^32 / mult) + 1; the key needs (range << sh) to fit in 64 - IDX_BITS bits
    const uint64_t range_hs = (0x100000000ull + bm.mult - 1) / std::max<uint32_t>(1, bm.mult) + 1;
    bm.composite = bm.mult >= 1 && bit_length(range_hs) + bm.sh <= 64 - IDX_BITS;
    bm.range_hs = (uint32_t)std::min<uint64_t>(range_hs, 0xFFFFFFFFull);
    {
        const uint32_t caps[4] = {(uint32_t)CAP_SMALL, (uint32_t)CAP_MID, (uint32_t)CAP_LARGE, (uint32_t)LANE_CAP};   // ([LANE_CFG]: the lane body)
        for (int i = 0; i < 4; i++) bm.sub_mult[i] = range_hs > caps[i] ? (uint32_t)(((uint64_t)caps[i] << 32) / range_hs) : 0u;
        // one-word ranking keys: sub-range s of configuration i (sub = floor(hs * sub_mult / 2^32), sub_mult rounded down) holds
        // hs values from s * width on (width = floor(range_hs / caps[i]) <= 2^32 / sub_mult) and below (s + 1) * 2^32 / sub_mult;
        // the distance between the two grows with s: the last sub-range gives the span every residue stays below
        const uint64_t max_index = slotted ? (uint64_t)sk->pend.n_blk * sk->pend.slot_cap : (uint64_t)n_all;
        const int index_bits = bit_length(max_index | 1);
        for (int i = 0; i < 4; i++) {
            bm.sub_width[i] = bm.sub_mult[i] ? (uint32_t)(range_hs / caps[i]) : 1u;
            uint64_t span_hs = 1;
            if (bm.sub_mult[i]) {
                const uint64_t top = std::min<uint64_t>(range_hs, (((uint64_t)caps[i] << 32) + bm.sub_mult[i] - 1) / bm.sub_mult[i]);
                span_hs = top - (uint64_t)(caps[i] - 1) * bm.sub_width[i] + 1;
            }
            bm.rank_bits[i] = (bm.composite && bit_length(span_hs) + bm.sh + index_bits <= 64) ? index_bits : 0;
        }
    }
    // partition geometry: F = 2^fine_bits buckets per coarse range (about 512 ranges), tiles of occurrences
    const PartGeom geom = part_geometry(B);
    // marker-less sample (sketch_session.h): hashes only, counted without occurrence records; tiny samples whose bucket range does
    // not fit the sub-range arithmetic get their records written and take the usual kernels
    if (!slotted && sk->n_plain && !(sk->n_plain == sk->n_occ && bm.composite)) materialise_plain_records(sk);
    bool plain = !slotted && sk->n_plain != 0;
    // Run-time shape knobs.  SYLPH_HIP_PART_TILE_BLOCKS / SYLPH_HIP_PART_STAGE_PAIRS: seeding blocks per partition tile and pairs the scatter stages
    // in LDS for the slotted sample — round 6 had 16 / 4096 (36.7 KiB of LDS per scatter workgroup, which waits for room beside the seeding kernel).
    static const uint32_t tile_blocks = [] { const char* e = getenv("SYLPH_HIP_PART_TILE_BLOCKS"); return e ? (uint32_t)std::max(1, std::min(32, atoi(e))) : BLK_PER_TILE; }();
    // (2048 pairs: 16 KiB + the range counters, 20 KiB per workgroup; a tile holds ~3,000 occurrences, the rest goes out directly —
    //  pipelined exact set +0.4..0.9 % over 4096 on top of the lean replay, 1536 and 1024 within noise of it: profiles/r07_ab_tail.txt)
    static const uint32_t stage_pairs = [] { const char* e = getenv("SYLPH_HIP_PART_STAGE_PAIRS"); return e ? (uint32_t)std::max(256, std::min(8192, atoi(e))) : 2048u; }();
    PartIn in{};
    in.slotted = slotted ? 1 : 0;
    in.key_sh = bm.sh;
    uint32_t n_tiles;
    const OccRec* recs;
    if (slotted) {
        in.slot_key = sk->slot_key.as<uint32_t>();
        in.n_blk = sk->pend.n_blk;
        in.slot_cap = sk->pend.slot_cap;
        in.blk_count = sk->slot_meta.as<uint32_t>() + (sk->pend.n_blk + 1);   // (layout: reads.hip SlotMeta)
        in.blk_per_tile = tile_blocks;
        in.stage_pairs = stage_pairs;
        n_tiles = (in.n_blk + tile_blocks - 1) / tile_blocks;
        recs = sk->slot_rec.as<OccRec>();
    } else {
        in.hash = sk->hash.as<uint64_t>();
        in.n_dense = n_all;
        in.tile_entries = (uint32_t)std::max<uint64_t>(4096, ((uint64_t)n_all + 65535) / 65536);   // at most 65,536 tiles
        n_tiles = (uint32_t)(((uint64_t)n_all + in.tile_entries - 1) / in.tile_entries);
        recs = sk->recs.as<OccRec>();
    }
    DevBuf &b_hist = ctx->scratch[0], &b_pairs = ctx->scratch[1], &b_perm = ctx->scratch[2], &b_tmpk = ctx->scratch[3],
           &b_tmpc = ctx->scratch[4], &b_small = ctx->scratch[5], &b_bk = ctx->scratch[6];
    b_hist.reserve(part_hist_words(geom, n_tiles) * 4);
    b_pairs.reserve((size_t)n_cap * 8);                                 // (bucket, occurrence index) pairs grouped by coarse range
    if (!plain) b_perm.reserve((size_t)n_cap * 4);
    DevBuf& b_sorted = ctx->scratch[7];                                 // marker-less: the hashes sorted by bucket
    if (plain) b_sorted.reserve((size_t)n_cap * 8);
    uint64_t* sorted_hash = plain ? b_sorted.as<uint64_t>() : nullptr;
    in.carry = plain ? 1 : 0;
    b_tmpk.reserve((size_t)n_cap * 8);
    b_tmpc.reserve((size_t)n_cap * 4);
    b_small.reserve(64);                                                // FinishTail (part_hist_kernel clears 16 words)
    // boff | large_list | ovf_list | n_distinct | removed | d_off | mid_list (each B+2) | chunk_rows (264) | chunk_removed (264 u64)
    b_bk.reserve((size_t)(B + 2) * 4 * 7 + 264 * 4 + 264 * 8 + 16);
    uint32_t* hist = b_hist.as<uint32_t>();
    uint2* pairs = b_pairs.as<uint2>();
    uint32_t* boff = b_bk.as<uint32_t>();
    uint32_t* large_list = boff + (B + 2);      // [0] = number of buckets queued for the large configuration, [1..] = ids
    uint32_t* ovf_list = large_list + (B + 2);  // [0] = number of buckets beyond the large configuration, [1..] = ids
    uint32_t* n_distinct = ovf_list + (B + 2);
    uint32_t* removed_b = n_distinct + (B + 2);
    uint32_t* d_off = removed_b + (B + 2);
    uint32_t* mid_list = d_off + (B + 2);       // buckets for the medium configuration (n <= CAP_MID, or a long k-mer segment)
    uint32_t* chunk_rows = mid_list + (B + 2) + ((B & 1u) ? 1 : 0);       // (8-byte aligned: 7 * (B + 2) words is odd for odd B)
    unsigned long long* chunk_removed = reinterpret_cast<unsigned long long*>(chunk_rows + 264);
    FinishTail* d_tail = b_small.as<FinishTail>();
    const uint32_t* d_nv = boff + B;            // boff[B] = number of valid occurrences
    const uint32_t n_zero = (B + 2) * 2;                                            // n_distinct and removed (cleared by part_hist_kernel)
    // every launch below takes its sizes from device memory; the host synchronises ONCE, at the end (unless some buckets need
    // the list-driven configurations or the device-wide path)
    const int dbg = getenv("SYLPH_REPLAY_STAGE") ? atoi(getenv("SYLPH_REPLAY_STAGE")) : 0;
    const uint32_t cutoff = sk->paired ? 0u : SINGLE_CUTOFF;
    sk->out_k.reserve((size_t)n_cap * 8);          // upper bound: distinct k-mers <= occurrences
    sk->out_c.reserve((size_t)n_cap * 4);
    ReplayArgs ra{};
    if (plain) ra.hash = sorted_hash;
    else { ra.recs = recs; ra.perm = b_perm.as<uint32_t>(); }
    ra.boff = boff; ra.p_nv = d_nv;
    ra.paired = sk->paired; ra.dedup = sk->dedup_mode(); ra.cutoff = cutoff; ra.bm = bm;
    ra.tmp_k = b_tmpk.as<uint64_t>(); ra.tmp_c = b_tmpc.as<uint32_t>(); ra.n_distinct = n_distinct; ra.removed_b = removed_b;
    ra.overflow = &d_tail->overflow;               // (an address on the device: not read here)
    ra.mid_list = mid_list; ra.large_list = large_list; ra.ovf_list = ovf_list; ra.dbg_stage = dbg;
    {
        HostPhase ph(ctx, "finish(bucket): partition + LDS replay + compact");
        {
            ScopedKernelTimer t(ctx, "sort");   // the partition: what the library's radix sort of (bucket, index) pairs used to do
            launch_partition(ctx, in, bm, geom, n_tiles, n_all, hist, pairs, boff, b_perm.as<uint32_t>(), sorted_hash, n_distinct, n_zero,
                             b_small.as<uint32_t>(), large_list, ovf_list, mid_list);
        }
        {
            ScopedKernelTimer t(ctx, "replay");
            if (plain) hipLaunchKernelGGL((bucket_count_kernel<CAP_SMALL, RTPB_SMALL>), dim3(B), dim3(RTPB_SMALL), 0, ctx->stream, ra);
            else launch_replay(ctx, B, ra, sk->paired != 0, dbg != 0);
        }
    }
    // removed counts, table offsets, compaction, and everything the host needs to know in one block (FinishTail)
    auto close_table = [&](int skip_if_listed) {
        // two levels: chunks of 1024 x ipt buckets (at most 256 of them), then the compaction, which scans the chunk totals itself
        const uint32_t ipt = (B + (1u << 18) - 1) >> 18;
        ScopedKernelTimer t(ctx, "replay");
        hipLaunchKernelGGL(table_scan_kernel, dim3((B + SCAN_CHUNK * ipt - 1) / (SCAN_CHUNK * ipt)), dim3(SCAN_CHUNK), 0, ctx->stream, n_distinct,
                           removed_b, B, ipt, d_off, chunk_rows, chunk_removed);
        hipLaunchKernelGGL(table_compact_kernel, dim3(std::min<uint32_t>((B + 3) / 4, 1u << 15)), dim3(256), 0, ctx->stream,
                           b_tmpk.as<uint64_t>(), b_tmpc.as<uint32_t>(), boff, d_off, chunk_rows, chunk_removed, n_distinct, B, ipt,
                           sk->out_k.as<uint64_t>(), sk->out_c.as<uint32_t>(), ovf_list, mid_list, large_list, skip_if_listed,
                           d_tail, deferred ? sk->slot_meta.as<uint32_t>() + (size_t)(sk->pend.n_blk + 1) * 4 : (const uint32_t*)nullptr,
                           sk->a10_state == 1 ? sk->a10_tail.as<uint32_t>() : (const uint32_t*)nullptr, d_nv);
        SY_HIP(hipGetLastError());
    };
    FinishTail host{};
    auto read_tail = [&] {
        SY_HIP(hipMemcpyAsync(ctx->pinned, d_tail, sizeof host, hipMemcpyDeviceToHost, ctx->stream));
        SY_HIP(hipStreamSynchronize(ctx->stream));
        memcpy(&host, ctx->pinned, sizeof host);
        if (!ctx->pending.empty()) profile_collect(ctx);
    };
    close_table(1);
    read_tail();
    if (deferred) {
        if (host.verdict[0] || host.verdict[1]) {  // not a batch for the short-read kernel after all: the checked push, then from the top
            redo_deferred_batch(sk);
            a10_mark(sk);                          // (filter dedup: the marks went with the slots)
            return finish_bucketed(sk);
        }
        sk->pend.deferred = false;                 // the verdict is in: from here on an ordinary slotted sample ...
        sk->pend.n = host.n_found;                 // ... whose occurrence count is known (whoever flushes the slots to the dense arrays needs it)
    }
    // filter dedup: were the partitioned pass's marks good (a10.hip)?  If not the phase walk has marked the records again, dense: from the top
    if (!a10_verdict(sk, host.a10_words)) return finish_bucketed(sk);
    if (host.overflow) return false;             // inconsistent bounds (defensive): the generic path redoes the sample
    if (ctx->profile && !plain && (ctx->profile_only.empty() || ctx->profile_only.find(",replay,") != std::string::npos)) {
        // road counters (tests and tools ask sylph_ctx_kernel_stats how many buckets took which body): from the bucket offsets, on the
        // host — the kernel keeps no count.  Only where the replay family is timed at all: a region that times the seeding kernel
        // alone (bench.py's quoted rate) pays no read-back.
        std::vector<uint32_t> h_boff((size_t)B + 1);
        ctx->d2h(h_boff.data(), boff, ((size_t)B + 1) * 4);
        uint64_t n_lane = 0, n_general = 0;
        for (uint32_t i = 0; i < B; i++) {
            const uint32_t n_b = h_boff[i + 1] - h_boff[i];
            if (lane_road(bm, n_b, sk->paired != 0, ra.dedup, dbg != 0)) n_lane++;
            else if (n_b) n_general++;
        }
        ctx->stats["replay_lane"].launches += n_lane;
        ctx->stats["replay_general"].launches += n_general;
    }
    if (plain && host.n_ovf) {
        // k-mers more than a thousand deep in a marker-less sample: write the occurrence records after all and take the usual
        // kernels from the start (their overflow path works on records and on the index permutation)
        materialise_plain_records(sk);
        return finish_bucketed(sk);
    }
    if (host.n_mid || host.n_large) {
        // Buckets the 256-slot configuration passed on (more than 256 occurrences, or a k-mer 96+ deep: abundant genomes).  The
        // list-driven configurations are launched only now, with grids that match the lists: launched speculatively with every
        // sample they are two dispatches of large-LDS workgroups that find nothing to do, but cannot even START beside another
        // stream's seeding kernel (which leaves 10 KiB of LDS per CU) — in the pipelined bench they held the stream up for 0.3 ms.
        HostPhase ph(ctx, "finish(bucket): medium / large configurations");
        {
            ScopedKernelTimer t(ctx, "replay");
            if (plain) {
                if (host.n_large)
                    hipLaunchKernelGGL((bucket_count_list_kernel<CAP_LARGE, RTPB_LARGE>), dim3(std::min<uint32_t>(host.n_large, 1536u)),
                                       dim3(RTPB_LARGE), 0, ctx->stream, ra, large_list);
            } else {
                if (host.n_mid)
                    hipLaunchKernelGGL((bucket_replay_list_kernel<CAP_MID, RTPB_MID>), dim3(std::min<uint32_t>(host.n_mid, 1280u)),
                                       dim3(RTPB_MID), 0, ctx->stream, ra, mid_list);
                if (host.n_large)
                    hipLaunchKernelGGL((bucket_replay_list_kernel<CAP_LARGE, RTPB_LARGE>), dim3(std::min<uint32_t>(host.n_large, 512u)),
                                       dim3(RTPB_LARGE), 0, ctx->stream, ra, large_list);
            }
        }
        close_table(0);
        read_tail();
        if (host.overflow) return false;
    }
    unsigned long long removed_extra = 0;
    if (host.n_ovf) {
        // Some buckets exceed even the large configuration (k-mers with thousands of occurrences: low-complexity reads,
        // very abundant genomes).  Only THEIR occurrences go through the device-wide path, as one small sample; its rows
        // are patched into the buckets' slots and the table is compacted again.
        if (ctx->finish_mode == 2 || host.n_ovf > 4096) return false;
        HostPhase ph(ctx, "finish(bucket): overflowing buckets through the device-wide path");
        const uint32_t m = host.n_ovf;
        DevBuf b_so(ctx), b_si(ctx), b_sh(ctx), b_sr(ctx), sub_k(ctx), sub_c(ctx);
        b_so.reserve(((size_t)m + 1) * 4);
        hipLaunchKernelGGL(ovf_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, ovf_list, boff, b_so.as<uint32_t>());
        uint32_t n_sub = 0;
        ctx->read_back(&n_sub, b_so.as<uint32_t>() + m, 4);
        b_si.reserve((size_t)n_sub * 8);            // indices | sorted indices
        b_sh.reserve((size_t)n_sub * 8);
        b_sr.reserve((size_t)n_sub * sizeof(OccRec));
        uint32_t* sub_idx = b_si.as<uint32_t>();
        uint32_t* sub_sorted = sub_idx + n_sub;
        hipLaunchKernelGGL(ovf_indices_kernel, dim3(m), dim3(256), 0, ctx->stream, ovf_list, b_so.as<uint32_t>(), boff,
                           b_perm.as<uint32_t>(), sub_idx);
        sort_keys_u32(ctx, sub_idx, sub_sorted, n_sub, 0, 32);       // ascending index = file order
        {
            ScopedKernelTimer t(ctx, "replay_overflow");   // (family of its own so that tests can see this path was taken)
            hipLaunchKernelGGL(ovf_gather_kernel, dim3(grid_of(n_sub)), dim3(256), 0, ctx->stream, sub_sorted, n_sub, recs,
                               b_sh.as<uint64_t>(), b_sr.as<OccRec>());
        }
        uint64_t n_sub_out = 0, removed_sub = 0;
        generic_replay(ctx, b_sh.as<uint64_t>(), b_sr.as<OccRec>(), n_sub, sk->paired, sk->dedup_mode(), sub_k, sub_c, n_sub_out, removed_sub);
        removed_extra = removed_sub;
        {
            ScopedKernelTimer t(ctx, "replay");
            hipLaunchKernelGGL(ovf_patch_kernel, dim3(m), dim3(256), 0, ctx->stream, ovf_list, bm, sub_k.as<uint64_t>(),
                               sub_c.as<uint32_t>(), (uint32_t)n_sub_out, boff, b_tmpk.as<uint64_t>(), b_tmpc.as<uint32_t>(), n_distinct);
        }
        close_table(0);
        read_tail();
    }
    sk->n_out = host.n_seg;
    sk->dup_removed = host.removed + removed_extra;
    return true;
}

}  // namespace sylph
