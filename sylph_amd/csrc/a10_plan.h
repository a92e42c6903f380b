// a10_plan.h — the arithmetic of the filter dedup, free of HIP: a10.hip's kernels and host code call these functions for it and nothing else;
// tests/test_a10_plan.py compiles the same header with g++ (tests/a10_plan_capi.cpp) and runs a sequential model of the range pass over it.
#pragma once
#include <cmath>
#include <cstdint>

#include "replay_plan.h"

namespace sylph {
// the bits of an occurrence record's rid (their meaning: sketch_session.h, at OccRec) and the hash of an empty entry
constexpr uint64_t RID_MARKER_BIT = 1ull << 63;
constexpr uint64_t RID_A10_BIT = 1ull << 62;
constexpr int RID_RANK_SHIFT = 42;
constexpr uint64_t RID_RANK_MAX = (1ull << 20) - 1;
constexpr uint64_t RID_MASK = (1ull << RID_RANK_SHIFT) - 1;
constexpr uint64_t INVALID_HASH = ~0ull;

namespace a10_plan {
using namespace replay_plan;      // BucketMap, MAX_COARSE, min_u32, mulhi_u32, bits_of, bucket_lo_hash

constexpr uint64_t FX_K = 0x517cc1b727220a95ull;        // rustc-hash 1.x
constexpr uint64_t GOLD = 0x9E3779B97F4A7C15ull;
constexpr int MAX_FILTERS = 8;                           // capacities cap0 * (2^8 - 1): 2.5e9 items for the default cap0
constexpr uint64_t NO_OP = ~0ull;
constexpr uint32_t TILE_OCC = 1024, WALK_TPB = 256;      // occurrences per tile of the walk's inserting-operation count; its block size
constexpr uint32_t OPS_BLK_PER_TILE = 8;                 // seeding blocks per partition tile: two words per slot, half of BLK_PER_TILE
static_assert(TILE_OCC % WALK_TPB == 0, "a lane of the find kernel holds TILE_OCC / WALK_TPB consecutive occurrences");

// ---- hashes and keys ----------------------------------------------------------------------------------------------------------
SY_PLAN_HD uint64_t fx_add(uint64_t h, uint64_t w) { return (((h << 5) | (h >> 59)) ^ w) * FX_K; }
// FxHasher over the tuple (u64, [u32; 2]), mixed once more (the model's choice of 64 hash bits)
SY_PLAN_HD uint64_t item_hash(uint64_t km, uint64_t marker) { return fx_add(fx_add(fx_add(0, km), marker & 0xffffffffull), marker >> 32) * GOLD; }
struct FilterGeom { uint32_t fp_mask, nb_mask; };        // fingerprint bits of the filter; buckets - 1
// (fingerprint, smaller of the item's two buckets): what a cuckoo filter can still tell apart.  Below 2^63.
SY_PLAN_HD uint64_t reduced_key(FilterGeom d, uint64_t h) {
    uint32_t f = (uint32_t)(h >> 32) & d.fp_mask;
    if (!f) f = 1u;
    const uint32_t i1 = (uint32_t)h & d.nb_mask;
    const uint32_t i2 = (i1 ^ (uint32_t)(fx_add(0, f) >> 11)) & d.nb_mask;
    return ((uint64_t)f << 32) | min_u32(i1, i2);
}
// The place of an operation in the walk of sketch.rs:806-867, smaller = earlier: records in file order (mate 1, then mate 2), inside a
// record the order extract_markers emitted its seeds in (the rank the seeding kernels left in the rid), markers.0 before markers.1.
SY_PLAN_HD uint64_t op_key(uint64_t rid, uint32_t w) { return ((rid & RID_MASK) << 21) | (((rid >> RID_RANK_SHIFT) & RID_RANK_MAX) << 1) | w; }
// The word the partition moves for an operation: {upper 32 bits of the mixed class key | operation id = 2 x slot + marker}
SY_PLAN_HD uint64_t op_word(FilterGeom d, uint64_t km, uint64_t marker, uint32_t opid) {
    return ((reduced_key(d, item_hash(km, marker)) * GOLD) & 0xFFFFFFFF00000000ull) | opid;
}
// ---- filters, tables, which pass ------------------------------------------------------------------------------------------------
// Filter j of the scalable filter (as CuckooFilter::init / ScalableCuckoo::grow of the tests' CPU checker) -> 0, or the refused bucket count (> 2^31)
inline uint64_t filter_geometry(uint64_t capacity, double fpr0, int j, FilterGeom* out) {
    const uint64_t cap = capacity << j;
    const double fpr = fpr0 * std::pow(0.9, (double)j);
    int fp_bits = (int)std::ceil(std::log2(1.0 / fpr) + std::log2(8.0));
    fp_bits = fp_bits < 1 ? 1 : fp_bits > 31 ? 31 : fp_bits;
    uint64_t n_buckets = 1;
    while (n_buckets * 4 < cap) n_buckets <<= 1;
    *out = FilterGeom{(uint32_t)((1ull << fp_bits) - 1), (uint32_t)(n_buckets - 1)};
    return n_buckets <= (1ull << 31) ? 0 : n_buckets;
}
// The walk's table of a phase that `remaining` operations may enter: slot of a key = table_home(key, tab_shift), linear probing
struct TableGeom { uint64_t slots; uint32_t tab_shift; };
inline TableGeom table_geometry(uint64_t remaining) {
    uint64_t slots = 1024;
    while (slots < 2 * remaining) slots <<= 1;
    return TableGeom{slots, (uint32_t)(64 - (replay_plan::bits_of(slots) - 1))};
}
SY_PLAN_HD uint32_t table_home(uint64_t g, uint32_t tab_shift) { return (uint32_t)((g * GOLD) >> tab_shift); }
// the partitioned pass wherever the first filter is sure (count known) or expected (deferred batches: the verdict tells) to take every operation
SY_PLAN_HD bool fits(uint64_t n_slots, uint64_t n_expect_filter, uint64_t n_plain, uint64_t capacity) {
    return n_slots < (1ull << 31) && 2 * n_expect_filter <= capacity && n_plain == 0;
}
// ... and its two tail words {workgroups whose slices stayed too full, operations found}: are the marks good?
SY_PLAN_HD bool verdict_good(uint32_t too_full, uint32_t n_ops, uint64_t capacity) { return too_full == 0 && (uint64_t)n_ops <= capacity; }
// The walk's cut search: the tile that holds inserting operation number `cap` (0-based) and those before it; tile == n_tiles: none does
struct Cut { uint32_t tile; uint64_t before; };
inline Cut cut_tile(const uint32_t* tile_counts, uint32_t n_tiles, uint64_t cap) {
    uint64_t seen = 0;
    for (uint32_t q = 0; q < n_tiles; q++) {
        if (seen + tile_counts[q] > cap) return Cut{q, seen};
        seen += tile_counts[q];
    }
    return Cut{n_tiles, seen};
}
// ---- the partitioned pass: ranges, slots, slices, grid ------------------------------------------------------------------------
constexpr uint32_t RNG_TPB = 256;                                           // threads of a range workgroup
constexpr uint32_t RNG_SLOT_BITS = 17, RNG_SLOTS = 1u << RNG_SLOT_BITS;     // per workgroup, one bit each: 16 KB
constexpr uint32_t RNG_CAND = 512, RNG_TAB = 1024, RNG_TAB_BITS = 10;       // candidates per slice, table entries (both tables)
constexpr uint32_t RNG_WORDS = 8192;                                        // words per range aimed for
constexpr uint32_t RNG_FREE = 0xFFFFFFFFu;
constexpr uint32_t MAX_SPLIT = 8, XCDS = 8;                                 // workgroups that share a range; L2s the grid is dealt to
constexpr uint32_t MAX_SLICES = 4096, SLICE_STOP = 1024;                    // slices of a part; no further escalation from this many on
static_assert(RNG_TAB * 16 <= RNG_SLOTS / 8 && RNG_TAB == 1u << RNG_TAB_BITS, "the class table {key, earliest place} lies over the bit table");
static_assert(RNG_CAND % RNG_TPB == 0 && RNG_CAND <= RNG_TAB / 2, "every lane resolves RNG_CAND / RNG_TPB candidates; the tables stay half empty");
static_assert(((uint64_t)MAX_SPLIT << RNG_SLOT_BITS) <= 0xFFFFFFFFull, "the slot count of a range fits in 32 bits");

// B ranges of equal class-hash width, ~range_words operations each: key = upper half of an operation word, bucket = (key * B) >> 32.
// Not what make_bucket_map gives (sh = 32, mult = B): range_lo_key is the exact inverse of bucket_of_key for every B in 1..MAX_COARSE
// (tests/test_a10_plan.py), which `key - range_lo_key(c)` in the range kernel relies on.
SY_PLAN_HD uint64_t class_range(uint32_t B) { return (0x100000000ull + B - 1) / B + 1; }          // widest range in key units
inline BucketMap class_map(uint64_t n_expect, uint32_t range_words) {
    const uint64_t want = 2 * n_expect / range_words;
    BucketMap bm{};
    bm.B = (uint32_t)(want < 1 ? 1 : want > MAX_COARSE ? MAX_COARSE : want);
    bm.sh = 32;
    bm.mult = bm.B;                                                // (B << 32) / 2^32
    bm.composite = 1;
    bm.range_hs = (uint32_t)(class_range(bm.B) < 0xFFFFFFFFull ? class_range(bm.B) : 0xFFFFFFFFull);
    return bm;
}
SY_PLAN_HD uint32_t range_lo_key(uint32_t c, uint32_t B) { return (uint32_t)replay_plan::bucket_lo_hash(c, B, 0); }    // smallest upper half of range c
// distance of a word's upper half to its range's lowest (never RNG_FREE: the upper-half set keeps that for its free entries)
SY_PLAN_HD uint32_t range_residue(uint64_t word, uint32_t lo_key) { return min_u32((uint32_t)(word >> 32) - lo_key, RNG_FREE - 1u); }
// `split` workgroups share a range; the upper halves are uniform over it: residue x all_slots / width is a direct-mapped slot (slot_mult = 0: the residue itself)
struct RangeGeom { uint32_t split, all_slots, slot_mult; };
inline RangeGeom range_geometry(uint32_t B, uint32_t split) {
    const uint64_t all_slots = (uint64_t)split << RNG_SLOT_BITS, range = class_range(B);
    return RangeGeom{split, (uint32_t)all_slots, range > all_slots ? (uint32_t)((all_slots << 32) / range) : 0u};
}
struct RangeSlot { uint32_t part, local; };              // the workgroup of the range that holds the slot; the slot in its bit table
SY_PLAN_HD RangeSlot range_slot(uint32_t res, RangeGeom g) {
    const uint32_t s = min_u32(g.slot_mult ? mulhi_u32(res, g.slot_mult) : res, g.all_slots - 1u);
    return RangeSlot{s >> RNG_SLOT_BITS, s & (RNG_SLOTS - 1u)};
}
// A part too full for the lists is cut into P slices of equal slot width, resolved one after the other (equal classes share a slot)
SY_PLAN_HD uint32_t slice_of(uint32_t local, uint32_t P) { return (uint32_t)(((uint64_t)local * P) >> RNG_SLOT_BITS); }
// The next slice count after a pass over P slices found a list too full (n_over: twice the second arrivals, or the candidates): slices
// of about half the lists (the slots are uniform: 11 sigma of room); a slice that is still too full holds many copies of ONE item —
// eight times as many, again while there are fewer than SLICE_STOP (from 3: 24, 192, 1536), then 0: more copies of one item than the lists take, the walk takes the sample.
SY_PLAN_HD uint32_t next_slices(uint32_t P, uint32_t n_over) {
    if (P >= SLICE_STOP) return 0;
    // (half a list per slice; not (n_over + half - 1) / half: the sum may wrap)
    return P == 1 ? min_u32(n_over / (RNG_CAND / 2) + (n_over % (RNG_CAND / 2) ? 1u : 0u), MAX_SLICES) : min_u32(P * 8u, MAX_SLICES);
}
// Workgroups go round-robin to the XCDS L2s: the `split` workgroups of a range are XCDS apart in the grid — the same XCD, one right
// behind the other — so that the second one's reads of the range's words are L2 hits.  c >= B: padding to whole groups of XCDS ranges.
struct RangeBlock { uint32_t c, part; };
SY_PLAN_HD RangeBlock range_of_block(uint32_t block, uint32_t split) {
    return RangeBlock{(block / (XCDS * split)) * XCDS + (block & (XCDS - 1u)), (block / XCDS) % split};
}
SY_PLAN_HD uint32_t range_grid(uint32_t B, uint32_t split) { return ((B + XCDS - 1) / XCDS) * XCDS * split; }
// home slots of the two open-addressing LDS tables (linear probing, RNG_TAB entries): the upper-half set and the class table
SY_PLAN_HD uint32_t up_home(uint32_t res) { return (res * 0x9E3779B1u) >> (32 - RNG_TAB_BITS); }
SY_PLAN_HD uint32_t class_home(uint64_t g) { return (uint32_t)((g * GOLD) >> 40) & (RNG_TAB - 1u); }
SY_PLAN_HD uint32_t tab_next(uint32_t at) { return (at + 1u) & (RNG_TAB - 1u); }
}  // namespace a10_plan
}  // namespace sylph
