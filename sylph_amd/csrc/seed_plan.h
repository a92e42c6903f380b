// seed_plan.h — the geometry of the seeding kernels (reads.hip + reads_block.h: one lane per record; seeds.hip: one lane per 64
// positions), free of HIP: the constants and what their comments claim, how the host cuts a short-read batch into blocks, which
// records and which stream words belong to a block, where a k-mer's hit bit lies, how workgroups are dealt to the XCDs, and the
// layout of the block tables.  The kernels and their launchers include this header; tests/test_seed_plan.py compiles the same header
// with g++ (tests/seed_plan_capi.cpp) and checks every rule below at the two clamps of the block size and 64 sizes in between.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SY_SEED_HD __host__ __device__ __forceinline__
#else
#define SY_SEED_HD inline
#endif

namespace sylph {
namespace seed_plan {

// ---- the read kernel (K1r) --------------------------------------------------------------------------------------------------
constexpr int RTPB = 256;                          // lanes = records per pass
constexpr int RTPB_RAGGED = 512;                   // lanes (= records per pass) of the kernel's variant for ragged input
// A workgroup's block of aligned base coordinates is sized by the host so that it holds about RTPB records (rt = 256 x mean
// record length, a multiple of 16): with a fixed 16 KiB block only 109 of the 256 lanes had a 150 bp read to work on.
constexpr int RT_MIN = 4096, RT_MAX = 65536;
constexpr int RH = 400;                            // halo = longest record taken (pair_kmer_single's upper limit, sketch.rs:923)
constexpr int K_MIN = 21;                          // the smallest k: a record has at most RH - (K_MIN - 1) hashed k-mers
constexpr int NH_MAX = RH - (K_MIN - 1);           // RH - 20
constexpr int RPAD = 32;                           // lanes that idle behind the longest read of their wave read past the data
constexpr int MASKW = 12;                          // 12 * 32 = 384 >= RH - 20 k-mers per record
constexpr int OFFS_256 = 600;                      // record offsets staged in LDS (256-record blocks)
SY_SEED_HD constexpr int offs_staged(int tpb) { return tpb == RTPB ? OFFS_256 : 2 * tpb + 80; }
constexpr int OWNER_LANE_BITS = 10;                // the survivors' list: lane | k-mer index << 10

// ---- the position kernels (K1) ----------------------------------------------------------------------------------------------
constexpr int TPB = 256;
constexpr int WPT = 4;                        // packed dwords (16 bases each) per lane
constexpr int TILE_WORDS = TPB * WPT;         // 1024
constexpr int TILE_BASES = TILE_WORDS * 16;   // 16384
constexpr int HALO_WORDS = 2;                 // k-1 <= 31 bases beyond the tile
constexpr int STAGE_CAP = 1024;               // LDS survivor staging (12 KiB)
constexpr int FLUSH_AT = 512;
constexpr int LIST_CAP = 2048;                // survivors of a tile finished cooperatively (ordered-slots kernel); 16384 / c expected

SY_SEED_HD constexpr uint32_t half_groups(uint32_t nh) { return (nh + 7u) >> 3; }     // half-groups of 8 k-mers

// ---- which k-mers of a record the reference hashes, and in which order it emits them ------------------------------------------------
// Number of k-mer start positions of a length-L sequence that the reference hashes.
//   scalar  (seeding.rs:93,120):              L >= k ? L-k+1 : 0
//   avx2    (avx2_seeding.rs:37-44,95):       4*((L-k+1)/4), nothing if L < min_len (k+1 reads, 2k contigs :160)
SY_SEED_HD constexpr uint64_t n_hashed_kmers(uint64_t L, uint32_t k, int avx2_compat, int positions) {
    if (L < k) return 0;
    if (!avx2_compat) return L - k + 1;
    const uint64_t min_len = positions ? 2ull * k : (uint64_t)k + 1;
    if (L < min_len) return 0;
    return ((L - k + 1) / 4) * 4;
}
// The quarter of a record k-mer i lies in, i / len4 for i < 4 * len4 (len4 > 0): the quotient is 0..3, so three compares against len4,
// 2 len4 and 3 len4 count it where the division was a 32-bit integer division per survivor (tests/test_pass_state_plan.py: every
// nh <= NH_MAX, and a sample of large ones for the position kernel).
SY_SEED_HD constexpr uint32_t emission_lane(uint32_t i, uint32_t len4) {
    return (uint32_t)(i >= len4) + (uint32_t)(i >= 2u * len4) + (uint32_t)(i >= 3u * len4);   // (len4 <= 2^30: no product wraps)
}
// Place of the k-mer that starts at base i of a record with nh hashed k-mers in the order extract_markers emits the record's seeds
// (sketch.rs:53-69): position order for the scalar routine (seeding.rs:86-146); the 4-lane AVX2 routine (avx2_seeding.rs:33-148) walks
// four quarters of the record in lock step and pushes lane 0..3 of every step: (i mod len4, i div len4) with len4 = nh / 4 (there nh
// is a multiple of 4, n_hashed_kmers, and i < nh).
SY_SEED_HD constexpr uint64_t emission_rank(uint32_t i, uint32_t nh, int avx2_compat) {
    if (!avx2_compat || nh < 4) return i;
    const uint32_t len4 = nh >> 2, lane = emission_lane(i, len4);
    return (uint64_t)(i - lane * len4) * 4 + lane;
}

// slots of a block / tile that expects `expect` survivors, of at most `full`: 75 % and 48 above the expectation
SY_SEED_HD constexpr uint32_t slot_capacity(uint64_t full, uint64_t expect) {
    const uint64_t want = expect + expect * 3 / 4 + 48;
    return (uint32_t)(full < want ? full : want);
}

// ---- a block's stream ---------------------------------------------------------------------------------------------------------
// aligned coordinate of stream base 0 of block blk (a multiple of 16; negative for the first block)
SY_SEED_HD constexpr int64_t block_a0(uint32_t blk, uint32_t rt) { return (int64_t)blk * rt - RH; }
// block_a0 >= 0: every block but the first (rt >= RT_MIN > RH) — asked of the block's number, a 32-bit scalar
SY_SEED_HD constexpr bool block_starts_inside(uint32_t blk) { return blk != 0u; }
// stream words a block loads: its rt coordinates, RH on both sides (the end of its last record; mate 1 of a mate 2 that starts the
// block), and the words a 64-bit window behind the last base touches
SY_SEED_HD constexpr uint32_t stream_words(uint32_t rt) { return (rt + 2u * RH) / 16u + 3u; }
SY_SEED_HD constexpr uint32_t lds_words(uint32_t rt) { return stream_words(rt) + RPAD; }       // what lds_bytes pays for
// The words of a block's stream that lie inside the batch: word ci starts at coordinate a0 + 16 ci and is loaded where that is in
// [0, n_al) — the words [lo, hi) — and zero elsewhere (only the first and the last blocks of a batch have such words)
SY_SEED_HD void stream_word_range(int64_t a0, uint64_t n_al, uint32_t n_words, uint32_t& lo, uint32_t& hi) {
    const int64_t left = (int64_t)n_al - a0;                      // coordinates from the block's first to the end of the batch
    const uint64_t l = a0 < 0 ? (uint64_t)(-a0) / 16u : 0u, h = left > 0 ? ((uint64_t)left + 15u) / 16u : 0u;
    lo = (uint32_t)(l < n_words ? l : n_words);
    hi = (uint32_t)(h < n_words ? h : n_words);
}
// A record belongs to the block its aligned start coordinate (off + bias) falls into: block b begins with the first record r in
// [0, n_rec] whose coordinate is not below block_begin(b, rt) (off is non-decreasing)
SY_SEED_HD constexpr uint64_t block_begin(uint32_t blk, uint32_t rt) { return (uint64_t)blk * rt; }
SY_SEED_HD uint64_t first_record_of_block(const uint64_t* off, uint64_t n_rec, uint32_t bias, uint32_t blk, uint32_t rt) {
    const uint64_t target = block_begin(blk, rt);
    uint64_t lo = 0, hi = n_rec;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid] + bias < target) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// stream base of a record (or of a mate) that starts at `start`: in [RH, RH + rt) for the records of the block itself
SY_SEED_HD constexpr uint32_t record_rel(uint64_t start, uint32_t bias, int64_t a0) { return (uint32_t)((int64_t)(start + bias) - a0); }
// The same base in 32 bits: the block's constant rel_bias is formed once (a scalar), a record's base is ONE 32-bit add on the low
// word of its offset — what the truncation in record_rel leaves of the 64-bit sum and difference (tests/test_pass_state_plan.py).
SY_SEED_HD constexpr uint32_t rel_bias(uint32_t bias, int64_t a0) { return bias - (uint32_t)(uint64_t)a0; }
SY_SEED_HD constexpr uint32_t record_rel32(uint64_t start, uint32_t rb) { return (uint32_t)start + rb; }
// What a lane keeps of its record for the steps behind the hash loop: the stream bases of its two marker windows (sketch.rs:625-688) — a
// single read of 66..RH bases marks its start and its middle, a pair whose mates both have 33 bases marks the mates' starts.  bb = 0: no
// markers (a marked record's second window starts at least 33 bases into the stream).  Lengths are at most RH here: 32 bits.
struct MarkerBases { uint32_t ba, bb; };
SY_SEED_HD constexpr MarkerBases single_marker_bases(uint32_t rel, uint32_t L) {
    return (L >= 66u && L <= (uint32_t)RH) ? MarkerBases{rel, rel + L / 2u} : MarkerBases{0u, 0u};
}
SY_SEED_HD constexpr MarkerBases pair_marker_bases(uint32_t rel1, uint32_t rel2, uint32_t L1, uint32_t L2) {
    return (L1 >= 33u && L2 >= 33u) ? MarkerBases{rel1, rel2} : MarkerBases{0u, 0u};
}
// The hash loop of a lane with stream base rel in a wavefront whose longest record has nh_max k-mers: it holds the raw words w0, w0 + 1
// (w0 = rel >> 4), takes three lane-aligned words before the loop and one per whole group of 16, each fetching the raw word two ahead.
SY_SEED_HD constexpr uint32_t hash_hi_word(uint32_t rel, uint32_t nh_max) { return (rel >> 4) + 4u + (half_groups(nh_max) >> 1); }
// highest word of the 64-bit window of 32 bases at stream base b (win64: markers and the survivors' k-mers)
SY_SEED_HD constexpr uint32_t win64_hi_word(uint32_t b) { return (b >> 4) + 2u; }

// ---- hit masks ----------------------------------------------------------------------------------------------------------------
// k-mer i of a record <-> bit 31 - (i & 31) of word i >> 5 of the record's mask column
SY_SEED_HD constexpr uint32_t kmer_word(uint32_t i) { return i >> 5; }
SY_SEED_HD constexpr uint32_t kmer_bit(uint32_t i) { return 31u - (i & 31u); }
// a group of 16 k-mers is one 16-bit half of its word, even groups the upper half: the half's index behind the record's first word
// in a [MASKW][tpb] array of 32-bit words seen as halves
SY_SEED_HD constexpr uint32_t group_half(uint32_t g, uint32_t tpb) { return ((g >> 1) * tpb * 2u) + ((g & 1u) ^ 1u); }
SY_SEED_HD constexpr uint32_t mask_words(uint32_t nh) { return (nh + 31u) >> 5; }
// the bits of a record's last word that are its own: nh - 32 (mask_words - 1) = 1 .. 32 k-mers, from bit 31 down (nh > 0)
SY_SEED_HD constexpr uint32_t tail_mask(uint32_t nh) { return (uint32_t)(0xFFFFFFFF00000000ull >> (nh - (mask_words(nh) - 1u) * 32u)); }
// mask rows the pass's longest record (hg_max half-groups) reaches; the rows above are free for the survivors' list
SY_SEED_HD constexpr uint32_t rows_used(uint32_t hg_max) { const uint32_t r = (hg_max * 8u + 31u) >> 5; return r < (uint32_t)MASKW ? r : (uint32_t)MASKW; }
SY_SEED_HD constexpr bool listed(uint32_t total, uint32_t rows, uint32_t tpb) { return total <= ((uint32_t)MASKW - rows) * tpb; }
// counting-sort bin of a record with nh k-mers: longest first
SY_SEED_HD constexpr uint32_t deal_bin(uint32_t nh) { return 63u - half_groups(nh); }

// ---- hit bits set by LDS atomics (round 14) -----------------------------------------------------------------------------------------
// The hash loop may set a k-mer's hit bit with an LDS xor issued under the threshold compare's own lane mask.  The xor's data is
// one of 16 constants, hit_const(T) for k-mer T of its group of 16: the k-mer's bit of a 16-bit half, in BOTH halves of the word, so
// that the two groups of a word share the constants.  The words start as zero (deal_by_length: the pass's rows_used rows of every lane); after an EVEN group
// (a lone half-group of 8 included) a 16-bit store of zero clears the lower half (hit_clear_after, hit_cleared); the odd group then
// goes into both halves again.  The word ends up as upper = even ^ odd, lower = odd, and hit_decode brings back the layout of
// kmer_word / kmer_bit.  hit_decode is its own inverse — a second decode would return the encoded word — so a pass decodes its
// words exactly once, in a step of its own in front of everything that reads or strikes a bit (reads_block.h decode_hits).
SY_SEED_HD constexpr uint32_t hit_const(uint32_t t) { return 0x00010001u << (15u - t); }
SY_SEED_HD constexpr bool hit_clear_after(uint32_t g) { return (g & 1u) == 0u; }
SY_SEED_HD constexpr uint32_t hit_cleared(uint32_t m) { return m & 0xFFFF0000u; }
SY_SEED_HD constexpr uint32_t hit_decode(uint32_t m) { return m ^ (m << 16); }
// byte offset of group g's word behind the record's first word in a [MASKW][tpb] array (its lower half lies at that offset, the upper
// half two bytes on: group_half counts the same halves)
SY_SEED_HD constexpr uint32_t hit_word_offset(uint32_t g, uint32_t tpb) { return (g >> 1) * tpb * 4u; }
// The model of one record's column, as the loop writes it: hits[i] != 0 <=> k-mer i is below the threshold, for the i < 8 * n_half
// k-mers a wavefront with n_half half-groups walks; col[0 .. rows_used(n_half)) gets the ENCODED words.
inline void hit_encode_model(const uint8_t* hits, uint32_t n_half, uint32_t* col) {
    for (uint32_t w = 0; w < rows_used(n_half); w++) col[w] = 0;
    const uint32_t n_grp = n_half >> 1;
    for (uint32_t g = 0; g < n_grp + (n_half & 1u); g++) {
        uint32_t& word = col[hit_word_offset(g, 1) / 4u];
        const uint32_t n_t = g < n_grp ? 16u : 8u;
        for (uint32_t t = 0; t < n_t; t++)
            if (hits[g * 16u + t]) word ^= hit_const(t);
        if (hit_clear_after(g)) word = hit_cleared(word);
    }
}

// ---- XCD dealing ----------------------------------------------------------------------------------------------------------------
// Workgroups are dealt round-robin to the 8 XCDs (each with its own L2): position i of the dealing of n items gives every XCD one
// contiguous eighth.  The result may be >= n for the padding of the last XCD's range.
// (xcd_share: one XCD's eighth, for a caller that deals many positions of one n)
SY_SEED_HD constexpr uint32_t xcd_share(uint32_t n) { return (n + 7u) / 8u; }
SY_SEED_HD constexpr uint32_t xcd_deal_share(uint32_t i, uint32_t share) { return (i & 7u) * share + (i >> 3); }
SY_SEED_HD constexpr uint32_t xcd_deal(uint32_t i, uint32_t n) { return xcd_deal_share(i, xcd_share(n)); }
SY_SEED_HD constexpr uint32_t xcd_positions(uint32_t n) { return xcd_share(n) * 8u; }
// where the last tail_pct per cent of the positions begin, when they are a launch of their own: whole rounds of 8, at least 64 blocks
SY_SEED_HD constexpr uint32_t xcd_tail_cut(uint32_t n, uint32_t tail_pct) {
    const uint32_t n_round = xcd_positions(n);
    return (tail_pct && n_round >= 64u) ? (uint32_t)((uint64_t)n_round * (100u - tail_pct) / 100u) & ~7u : n_round;
}

// ---- the host's cut of a short-read batch -----------------------------------------------------------------------------------------
struct ReadsBlockPlan {
    int tpb;                // lanes of the kernel's variant
    uint32_t rt;            // aligned base coordinates per block
    uint32_t n_blk;
    uint32_t slot_cap;      // occurrence slots per block
    uint32_t spill_cap;     // slots of a block that is redone: every hashed k-mer of the records that start in it
    size_t lds_bytes;       // dynamic LDS: the stream
    uint64_t n_expect;      // occurrences the batch is expected to leave
};
// block size: about RTPB records per workgroup
// Equally long records fill the RTPB lanes of every block exactly.  With ragged records the number that start inside a
// block scatters around its mean (sigma ~ 6 for 35-151 bp reads) and every block above RTPB pays a whole second pass for a
// handful of records: aim 7 % lower, so that such blocks are rare (c3r: 0.83 -> 0.70 ms per 0.62 Gbp; sweep 85-100 %).
// Ragged input CAN take the kernel's 512-lane variant (ragged_tpb_wanted; SYLPH_HIP_READS_RAGGED_TPB=512) where a block of that many
// records still fits the stream's LDS window.  It is not the default: measured 8 % SLOWER on c3r (profiles/r06_ab_ragged.txt: 804 against
// 878 Gbp/s; 754 at five wavefronts per SIMD) — the lane-steps it saves in the hash loop are less than what eight wavefronts waiting
// for each other at the pass's barriers cost.
inline ReadsBlockPlan reads_block_plan(uint64_t n_bases, uint64_t n_records, uint32_t bias, uint32_t c, uint32_t k, bool ragged_tpb_wanted) {
    ReadsBlockPlan p{};
    const bool ragged = (n_bases % n_records) != 0;
    p.tpb = (ragged && ragged_tpb_wanted && (uint64_t)RTPB_RAGGED * 93 / 100 * n_bases / n_records <= (uint64_t)RT_MAX) ? RTPB_RAGGED : RTPB;
    const uint64_t target = ragged ? (uint64_t)p.tpb * 93 / 100 : (uint64_t)p.tpb;
    const uint64_t want = target * n_bases / n_records;
    p.rt = (uint32_t)(want < (uint64_t)RT_MIN ? RT_MIN : want > (uint64_t)RT_MAX ? RT_MAX : want);
    p.rt = (p.rt + 15u) & ~15u;
    p.n_blk = (uint32_t)((n_bases + bias) / p.rt) + 1;
    p.spill_cap = p.rt + RH;
    p.slot_cap = slot_capacity(p.spill_cap, (uint64_t)p.rt / c);
    p.lds_bytes = (size_t)lds_words(p.rt) * 4;
    p.n_expect = (n_bases > n_records * (uint64_t)(k - 1) ? n_bases - n_records * (uint64_t)(k - 1) : 0) / c;
    return p;
}

// ---- the block tables -------------------------------------------------------------------------------------------------------------
// layout of a session's slot_meta buffer, in 32-bit words: [blk_rec (n_blk+1) | blk_count (n_blk+1) | spill_slot_of_blk (n_blk+1) |
// blk_off (n_blk+1) | ReadsState].  The total — blk_off[n_blk] — and the two flag words the state begins with (long_record,
// spill.n_tiles) sit side by side and leave in ONE 12-byte copy.
struct SlotMeta {
    uint32_t *blk_rec, *blk_count, *spill_slot, *blk_off, *state_words;
    SlotMeta(uint32_t* base, uint32_t n_blk)
        : blk_rec(base), blk_count(blk_rec + (n_blk + 1)), spill_slot(blk_count + (n_blk + 1)), blk_off(spill_slot + (n_blk + 1)),
          state_words(blk_off + (n_blk + 1)) {}
    static size_t bytes(uint32_t n_blk, size_t state_bytes) { return ((size_t)n_blk + 1) * 4 * 4 + state_bytes + 16; }
};

// ---- what the comments above claim --------------------------------------------------------------------------------------------------
static_assert(RT_MIN % 16 == 0 && RT_MAX % 16 == 0 && RT_MIN <= RT_MAX && RH % 16 == 0, "blocks and halo are whole 16-base words");
static_assert(block_a0(0, RT_MAX) < 0 && block_a0(1, RT_MIN) >= 0 && !block_starts_inside(0) && block_starts_inside(1), "only the first block starts in front of the batch");
static_assert(MASKW * 32 >= NH_MAX, "a record's k-mers have a mask bit each");
static_assert(MASKW % 2 == 0, "the columns are zeroed two rows at a time (deal_by_length)");
static_assert(half_groups(NH_MAX) <= 63 && deal_bin(NH_MAX) < 64 && deal_bin(0) == 63, "63 bins hold the half-groups of the longest record");
static_assert(RTPB_RAGGED <= (1 << OWNER_LANE_BITS) && (uint64_t)MASKW * 32 <= (1ull << (32 - OWNER_LANE_BITS)), "the owner word tid | idx << 10 holds 512 lanes and MASKW * 32 indices");
static_assert(RTPB % 64 == 0 && RTPB_RAGGED % 64 == 0 && RTPB <= RTPB_RAGGED, "whole wavefronts");
static_assert(offs_staged(RTPB) + 4 >= 2 * RTPB && offs_staged(RTPB_RAGGED) + 4 >= 2 * RTPB_RAGGED, "the marker arrays alias the staged offsets");
// RPAD: the loop's highest word (the last record of the block, hashed by a lane of a wavefront whose longest record is the longest there
// is) and the highest window lie inside what lds_bytes pays for; the windows inside the loaded stream itself
static_assert(hash_hi_word(RH + RT_MIN - 1, NH_MAX) < lds_words(RT_MIN) && hash_hi_word(RH + RT_MAX - 1, NH_MAX) < lds_words(RT_MAX), "RPAD covers the idle lanes' reads");
static_assert(win64_hi_word(RH + RT_MAX - 1 + RH - 1) < stream_words(RT_MAX) && win64_hi_word(RH + RT_MIN - 1 + RH - 1) < stream_words(RT_MIN), "every window of a record or its mate is loaded");
static_assert((((TILE_WORDS + HALO_WORDS - 1) << 4) | 15) < (1 << 16), "the 16-bit descriptor (word << 4) | off holds TILE_WORDS + HALO_WORDS");
static_assert((TPB - 1) * WPT + 6 <= TILE_WORDS + HALO_WORDS && WPT + HALO_WORDS == 6, "a lane's six words end inside TILE_WORDS + HALO_WORDS");
static_assert(HALO_WORDS * 16 >= 31 && HALO_WORDS <= TPB, "the halo holds the k - 1 bases behind the tile");
static_assert(FLUSH_AT <= STAGE_CAP && LIST_CAP <= TILE_BASES && LIST_CAP <= (1 << 16), "staging and list sizes");
static_assert(slot_capacity(TILE_BASES, TILE_BASES) == TILE_BASES, "a tile never gets more slots than positions");

}  // namespace seed_plan
}  // namespace sylph
