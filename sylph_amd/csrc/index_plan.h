// index_plan.h — the arithmetic of a database's line index (contain_index.h), free of HIP: how the k-mer range is cut into buckets,
// how the build splits the buckets into passes, the division that finds a k-mer's bucket, what a slot and a descriptor hold, how
// many of a bucket's postings stay in its line, the writer of one bucket, the scan of one line, and the keys hits are sorted by.
// line_index.hip (build), contain_index.h / contain.hip (probe, reassignment) and hits.hip (coverage width) include this header;
// tests/test_index_plan.py compiles it with g++ (tests/index_plan_capi.cpp), builds a model index with the writer and looks k-mers
// up with the scan — the very code the kernels run — against a dictionary.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SY_INDEX_HD __host__ __device__ __forceinline__
#else
#define SY_INDEX_HD inline
#endif

// Slots per bucket line: 8 (a 64-byte line, lambda = 4 postings aimed at per line) or 4 (round 5: a 32-byte half-line, lambda = 2 —
// the same index bytes, twice the buckets; random 32 B reads come back at 1.8x the rate of random 64 B reads on this chip,
// profiles/r05_random_line_rates.txt).  A compile-time choice: the probe's loads and the slot scan are unrolled over it.
#ifndef SYLPH_LINE_SLOTS
#define SYLPH_LINE_SLOTS 8
#endif

namespace sylph {
namespace index_plan {

constexpr int LINE_SLOTS = SYLPH_LINE_SLOTS;   // x 8 B per bucket line
static_assert(LINE_SLOTS == 8 || LINE_SLOTS == 4, "a bucket line is 64 or 32 bytes");
constexpr int LINE_QUADS = LINE_SLOTS / 2;     // 16-byte loads per line
constexpr uint32_t DEFAULT_INDEX_LAMBDA = LINE_SLOTS / 2;
constexpr uint64_t SLOT_EMPTY = ~0ull;
constexpr uint32_t LONG_RUN_MIN = 48;          // an overflow run with a stored length of at least this is walked by a whole wavefront
constexpr uint64_t NO_LONG_RUN = ~0ull;

SY_INDEX_HD int bit_length(uint64_t v) { int b = 0; while (v) { b++; v >>= 1; } return b; }

// ---- slot codec ------------------------------------------------------------------------------------------------------------
//   posting    = remainder << gshift |                    genome id       (gshift = gb + 1, gb = bit length of the largest genome id)
//   descriptor = run start << gshift | 1 << (gshift - 1) | min(run length, 2^(gshift-1) - 1)
// The last slot of a bucket with more than LINE_SLOTS postings is a descriptor of the overflow run that holds the rest; an unused
// slot is all ones (which reads as a descriptor: whoever asks slot_is_descriptor of a line's last slot asks != SLOT_EMPTY too).
SY_INDEX_HD uint64_t slot_flag(int gshift) { return 1ull << (gshift - 1); }
SY_INDEX_HD uint64_t slot_genome_mask(int gshift) { return slot_flag(gshift) - 1; }
SY_INDEX_HD uint64_t encode_posting(uint64_t rem, uint32_t genome, int gshift) { return (rem << gshift) | (uint64_t)genome; }
SY_INDEX_HD uint64_t encode_descriptor(uint64_t run_start, uint64_t run_len, int gshift) {
    const uint64_t gmask = slot_genome_mask(gshift);
    return (run_start << gshift) | slot_flag(gshift) | (run_len < gmask ? run_len : gmask);
}
SY_INDEX_HD uint64_t slot_rem(uint64_t s, int gshift) { return s >> gshift; }          // of a posting
SY_INDEX_HD uint64_t slot_run_start(uint64_t s, int gshift) { return s >> gshift; }    // of a descriptor
SY_INDEX_HD bool slot_is_descriptor(uint64_t s, int gshift) { return (s & slot_flag(gshift)) != 0; }
SY_INDEX_HD uint32_t slot_genome(uint64_t s, int gshift) { return (uint32_t)(s & slot_genome_mask(gshift)); }
SY_INDEX_HD uint64_t slot_run_len(uint64_t s, int gshift) { return s & slot_genome_mask(gshift); }   // saturated
// an entry of an overflow run (sorted by (remainder, genome), closed by SLOT_EMPTY): nothing for `rem` at or behind it
SY_INDEX_HD bool run_stops(uint64_t y, uint64_t rem, int gshift) { return y == SLOT_EMPTY || slot_rem(y, gshift) > rem; }

// ---- geometry --------------------------------------------------------------------------------------------------------------
// Bucket b covers the `div` k-mer values from kmer_lo + b * div; about `lambda` postings per bucket; remainder < div <= div_cap
// keeps the all-ones pattern free.  why != 0: the index cannot be built (the caller raises it).
enum Refusal { BUILDABLE = 0, TOO_MANY_GENOMES = 1, TOO_MANY_BUCKETS = 2 };
struct Geometry {
    int why, gb, gshift;
    uint64_t div_cap, div, magic, n_buckets;   // magic = floor(2^64 / div) for div >= 2, else 0
};
SY_INDEX_HD uint64_t magic_of(uint64_t div) { return div > 1 ? (uint64_t)((((unsigned __int128)1) << 64) / div) : 0; }
SY_INDEX_HD Geometry geometry(uint64_t n_genomes, uint64_t kmer_lo, uint64_t max_key, uint64_t postings, uint64_t lambda) {
    Geometry g{BUILDABLE, 0, 0, 0, 1, 0, 0};
    g.gb = bit_length(n_genomes ? n_genomes - 1 : 0);
    if (g.gb < 1) g.gb = 1;
    g.gshift = g.gb + 1;
    if (g.gb > 30) { g.why = TOO_MANY_GENOMES; return g; }
    g.div_cap = (1ull << (63 - g.gb)) - 1;
    const uint64_t span = max_key - kmer_lo + 1;                          // bucket 0 starts at kmer_lo; 0 = wrapped: the full 2^64 range
    uint64_t want_buckets = postings / (lambda ? lambda : DEFAULT_INDEX_LAMBDA);
    if (want_buckets < 1) want_buckets = 1;
    uint64_t div = span / want_buckets + (span % want_buckets ? 1 : 0);
    if (span == 0) div = g.div_cap;
    if (div < 1) div = 1;
    if (div > g.div_cap) div = g.div_cap;
    g.div = div;
    g.magic = magic_of(div);
    g.n_buckets = (max_key - kmer_lo) / div + 1;
    if (g.n_buckets >= (1ull << 32) - 1) g.why = TOO_MANY_BUCKETS;
    return g;
}
// the run start of a descriptor has 62 - gb bits
SY_INDEX_HD bool overflow_fits(uint64_t n_ovf, int gb) { return n_ovf < (1ull << (62 - gb)); }

// ---- pass split ------------------------------------------------------------------------------------------------------------
// The build filters, sorts and writes about pass_max postings at a time: pass p of n_pass owns the buckets [b0, b1) and the k-mers
// [klo, khi); the last pass runs up to the shard's own bound kmer_hi (0 = open).  b1 * div <= max_key - kmer_lo before the last pass.
SY_INDEX_HD uint32_t n_passes(uint64_t n_buckets, uint64_t postings, uint64_t pass_max) {
    if (pass_max < 1) pass_max = 1;
    uint64_t n = postings / pass_max + (postings % pass_max ? 1 : 0);
    if (n > n_buckets) n = n_buckets;
    return (uint32_t)(n < 1 ? 1 : n);
}
struct Pass { uint32_t b0, b1; uint64_t klo, khi; };
SY_INDEX_HD Pass pass_of(uint32_t p, uint32_t n_pass, uint64_t n_buckets, uint64_t kmer_lo, uint64_t kmer_hi, uint64_t div) {
    Pass r;
    r.b0 = (uint32_t)(n_buckets * p / n_pass);
    r.b1 = (uint32_t)(n_buckets * (p + 1) / n_pass);
    r.klo = kmer_lo + (uint64_t)r.b0 * div;
    r.khi = p + 1 < n_pass ? kmer_lo + (uint64_t)r.b1 * div : kmer_hi;
    return r;
}

// ---- bucket / remainder ----------------------------------------------------------------------------------------------------
// x / div and x % div for x = k-mer - base, by the geometry's magic: floor(x * floor(2^64 / div) / 2^64) is the quotient or one less
SY_INDEX_HD void bucket_rem(uint64_t x, uint64_t div, uint64_t magic, uint64_t& q, uint64_t& rem) {
    if (div == 1) { q = x; rem = 0; return; }
#if defined(__HIP_DEVICE_COMPILE__)
    q = __umul64hi(x, magic);
#else
    q = (uint64_t)(((unsigned __int128)x * magic) >> 64);
#endif
    rem = x - q * div;
    if (rem >= div) { rem -= div; q++; }
}

// ---- per-bucket layout -----------------------------------------------------------------------------------------------------
// a bucket of c postings keeps all of them in its line, or — more than LINE_SLOTS — all but one slot's worth: the last slot becomes
// the descriptor, and the overflow run takes the rest and the closing sentinel
SY_INDEX_HD uint32_t postings_in_line(uint32_t c) { return c > (uint32_t)LINE_SLOTS ? (uint32_t)LINE_SLOTS - 1 : c; }
SY_INDEX_HD uint32_t overflow_need(uint32_t c) { return c > (uint32_t)LINE_SLOTS ? c - postings_in_line(c) + 1 : 0; }

// ---- the bucket writer -----------------------------------------------------------------------------------------------------
// One bucket: its c postings (keys ascending, genome ids ascending within a key; kbase = first k-mer value of the bucket) into the
// line s[] and, for a crowded bucket, into the overflow run at ovf[run_start ..], overflow_need(c) entries.
SY_INDEX_HD void write_bucket(const uint64_t* keys, const uint32_t* gids, uint32_t c, uint64_t kbase, int gshift, uint64_t run_start,
                              uint64_t (&s)[LINE_SLOTS], uint64_t* ovf) {
    const uint32_t inl = postings_in_line(c);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < LINE_SLOTS; j++) s[j] = (uint32_t)j < inl ? encode_posting(keys[j] - kbase, gids[j], gshift) : SLOT_EMPTY;
    if (c > inl) {
        s[LINE_SLOTS - 1] = encode_descriptor(run_start, c - inl, gshift);
        uint64_t* o = ovf + run_start;
        for (uint32_t j = inl; j < c; j++) *o++ = encode_posting(keys[j] - kbase, gids[j], gshift);
        *o = SLOT_EMPTY;
    }
}

// ---- the slot scan ---------------------------------------------------------------------------------------------------------
// Calls f(genome id) for every posting with remainder `rem` in the line s[] and, when the line's own postings do not already
// exceed `rem`, in the bucket's overflow run.  A run with a stored length of at least LONG_RUN_MIN is not walked here: its first
// entry goes to *long_start with the remainder in *long_rem (the caller's wavefront walks it); *long_start is untouched otherwise.
template <class F>
SY_INDEX_HD void scan_slots(const uint64_t (&s)[LINE_SLOTS], uint64_t rem, int gshift, const uint64_t* ovf, F&& f, uint64_t* long_start,
                            uint64_t* long_rem) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < LINE_SLOTS; j++)
        if (slot_rem(s[j], gshift) == rem && !slot_is_descriptor(s[j], gshift)) f(slot_genome(s[j], gshift));
    const uint64_t last = s[LINE_SLOTS - 1];
    if (slot_is_descriptor(last, gshift) && last != SLOT_EMPTY && slot_rem(s[LINE_SLOTS - 2], gshift) <= rem) {   // the rest of the bucket is relevant
        if (slot_run_len(last, gshift) >= LONG_RUN_MIN) { *long_start = slot_run_start(last, gshift); *long_rem = rem; return; }
        for (uint64_t i = slot_run_start(last, gshift);; i++) {
            const uint64_t y = ovf[i];
            if (run_stops(y, rem, gshift)) break;
            if (slot_rem(y, gshift) == rem) f(slot_genome(y, gshift));
        }
    }
}

// ---- hit keys --------------------------------------------------------------------------------------------------------------
// A hit is (row << 32) | count with row = sample * n_genomes + genome.  When the bit lengths of the largest count (cb) and of the
// row count (rb) fit 32 bits together, the sorted finish sorts (row << cb) | count as 4-byte keys instead.
SY_INDEX_HD uint64_t hit_key(uint64_t row, uint32_t count) { return (row << 32) | count; }
struct CompactKey { int cb, rb; bool fits; };
SY_INDEX_HD CompactKey compact_key(uint32_t max_count, uint64_t n_rows) {
    CompactKey k;
    k.cb = bit_length(max_count);
    k.rb = bit_length(n_rows);
    if (k.cb < 1) k.cb = 1;
    if (k.rb < 1) k.rb = 1;
    k.fits = k.cb + k.rb <= 32;
    return k;
}
// bytes per coverage value in a result block: the narrowest of 1, 2, 4 that holds the batch's largest count, where narrow values are wanted
SY_INDEX_HD uint32_t coverage_width(bool want_narrow, uint32_t max_count) {
    return !want_narrow ? 4u : max_count < 256u ? 1u : max_count < 65536u ? 2u : 4u;
}

}  // namespace index_plan
}  // namespace sylph
