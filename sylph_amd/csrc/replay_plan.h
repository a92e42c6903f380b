// replay_plan.h — the bucket map of the in-LDS replay (replay_lds.hip, replay_bucket.h) and of the partition in front of it
// (partition.h), free of HIP: which bucket a hash belongs to, where a bucket begins, which sub-range of its bucket a hash falls into,
// and the map the host derives from a sample's size.  The kernels include this header through partition.h; tests/test_replay_plan.py
// compiles the same header with g++ (tests/replay_plan_capi.cpp) and checks the arithmetic bucket by bucket.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SY_PLAN_HD __host__ __device__ __forceinline__
#else
#define SY_PLAN_HD inline
#endif

namespace sylph {
namespace replay_plan {

// The configurations of the replay kernel: slots per workgroup.  Buckets of up to CAP_SMALL occurrences (all of them, for ordinary
// samples) run in the 256-slot configuration — those of up to LANE_CAP with one occurrence per lane (replay_bucket_lane: LANE_CAP
// threads, LANE_CAP sub-ranges) — larger ones, and buckets that hold a deep k-mer (SEG_LIMIT), in the CAP_MID / CAP_LARGE ones.
constexpr int CAP_SMALL = 256, CAP_MID = 512, CAP_LARGE = 1024, LANE_CAP = 128;
// index of a configuration in BucketMap::sub_mult / sub_width / rank_bits
enum ReplayCfg : int { CFG_SMALL = 0, CFG_MID = 1, CFG_LARGE = 2, LANE_CFG = 3, N_CFG = 4 };
constexpr int cfg_of_cap(int cap) { return cap == CAP_SMALL ? CFG_SMALL : cap == CAP_MID ? CFG_MID : CFG_LARGE; }
constexpr uint32_t cap_of_cfg(int cfg) { return (uint32_t)(cfg == CFG_SMALL ? CAP_SMALL : cfg == CFG_MID ? CAP_MID : cfg == CFG_LARGE ? CAP_LARGE : LANE_CAP); }
constexpr int IDX_BITS = 10;         // arrival index inside a bucket (< CAP_LARGE)
// The marker test of the small configuration looks at every earlier occurrence of the k-mer: quadratic in a k-mer's coverage.
// A bucket holding a k-mer with SEG_LIMIT or more occurrences (a genome at ~100x and above) is handed to the medium / large
// configuration, whose marker test is a hash table in LDS: linear in the bucket size.
constexpr uint32_t SEG_LIMIT = 96;
constexpr uint32_t MAX_COARSE = 4096;     // coarse ranges of the partition (LDS counters of its histogram / scatter kernels)

SY_PLAN_HD int bits_of(uint64_t v) { int b = 0; while (v) { b++; v >>= 1; } return b; }
SY_PLAN_HD uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }
SY_PLAN_HD uint32_t mulhi_u32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }     // (one v_mul_hi_u32 on the device)
// bits of a hash kept in the 32-bit bucket key of an occurrence: key = hash >> key_shift(c) (hashes are below u64::MAX / c)
inline int key_shift(uint32_t c) { const int b = bits_of(UINT64_MAX / (uint64_t)(c ? c : 1u)) - 32; return b > 0 ? b : 0; }

// Bucket of a hash: hs = hash >> sh (its 32 most significant bits below the threshold), b = (hs * mult) >> 32 — B
// equal ranges for ANY B (not only powers of two), monotone in the hash.  Inverse used by the replay kernel: the
// smallest hs of bucket b is ceil(b * 2^32 / mult).
// range_hs = widest bucket in hs units; sub_mult[i] = floor(2^32 * CAP_i / range_hs) for the configuration i (ReplayCfg; the sub-range
// of a hash inside its bucket, see replay_bucket / replay_bucket_lane), 0 when a bucket is narrower than CAP_i hs units.
// rank_bits[i] > 0: (hash - lowest hash the sub-range can hold) << rank_bits | gather index fits in 64 bits for configuration
// i — the key the occurrences of a sub-range are ranked by with ONE compare; sub_width[i] = floor(range_hs / CAP_i) hs units (a
// lower bound of where sub-range s begins: s * sub_width).  inv_mult = floor(2^64 / mult) (2^64 - 1 for mult = 1): bucket_lo_key.
struct BucketMap { int sh; uint32_t mult; uint32_t B; int composite; uint32_t range_hs; uint32_t sub_mult[N_CFG]; uint32_t sub_width[N_CFG]; int rank_bits[N_CFG]; uint64_t inv_mult; };

SY_PLAN_HD uint32_t bucket_of_key(uint32_t key, const BucketMap m) { return min_u32(mulhi_u32(key, m.mult), m.B - 1u); }
// lowest hash that maps to bucket b: key >= ceil(b * 2^32 / mult), the exact inverse of bucket_of_key
SY_PLAN_HD uint64_t bucket_lo_hash(uint32_t b, uint32_t mult, int sh) { return ((((uint64_t)b << 32) + mult - 1u) / mult) << sh; }
// The same bound in key units — ceil(b * 2^32 / mult) — without the 64-bit division (about 130 scalar instructions per workgroup where
// the operands are uniform): q = floor(b * inv / 2^32) with inv = floor(2^64 / mult) falls short of b * 2^32 / mult by less than
// b / 2^32 < 1, so it is the true quotient's floor or one below; the remainder says which, and whether to round up.
SY_PLAN_HD uint64_t bucket_lo_key(uint32_t b, uint32_t mult, uint64_t inv) {
    uint64_t q = (uint64_t)b * (uint32_t)(inv >> 32) + (((uint64_t)b * (uint32_t)inv) >> 32);
    uint64_t r = ((uint64_t)b << 32) - q * mult;            // in [0, 2 * mult)
    if (r >= mult) { q++; r -= mult; }
    return q + (r ? 1u : 0u);
}
// sub-range (of `cap`) of a key's distance `res` to its bucket's lowest key; sub_mult = BucketMap::sub_mult of the configuration
SY_PLAN_HD uint32_t sub_range_of(uint32_t res, uint32_t sub_mult, uint32_t cap) {
    return sub_mult ? min_u32(mulhi_u32(res, sub_mult), cap - 1u) : min_u32(res, cap - 1u);
}

// The map of a sample sketched at rate 1/c: B = n_all / bucket_target equal hash ranges.  max_index = the largest index an occurrence
// can be gathered by (what a one-word ranking key has to leave room for).
inline BucketMap make_bucket_map(uint32_t c, uint32_t n_all, uint32_t bucket_target, uint64_t max_index) {
    const uint64_t thr = UINT64_MAX / (uint64_t)c;
    const uint64_t n_buckets = n_all / bucket_target;
    BucketMap bm{};
    bm.B = (uint32_t)(n_buckets < 1 ? 1 : n_buckets > (1u << 24) ? (1u << 24) : n_buckets);
    bm.sh = key_shift(c);
    const uint64_t hs_max = thr >> bm.sh;                              // hashes are < thr
    const uint64_t mult = ((uint64_t)bm.B << 32) / (hs_max + 1);
    bm.mult = (uint32_t)(mult < 0xFFFFFFFFull ? mult : 0xFFFFFFFFull);
    bm.inv_mult = bm.mult > 1 ? (uint64_t)(((unsigned __int128)1 << 64) / bm.mult) : ~0ull;
    // widest bucket in hs units is ceil(2^32 / mult) + 1; the key needs (range << sh) to fit in 64 - IDX_BITS bits
    const uint64_t range_hs = (0x100000000ull + bm.mult - 1) / (bm.mult ? bm.mult : 1u) + 1;
    bm.composite = bm.mult >= 1 && bits_of(range_hs) + bm.sh <= 64 - IDX_BITS;
    bm.range_hs = (uint32_t)(range_hs < 0xFFFFFFFFull ? range_hs : 0xFFFFFFFFull);
    // one-word ranking keys: sub-range s of configuration i (sub = floor(hs * sub_mult / 2^32), sub_mult rounded down) holds
    // hs values from s * width on (width = floor(range_hs / cap) <= 2^32 / sub_mult) and below (s + 1) * 2^32 / sub_mult;
    // the distance between the two grows with s: the last sub-range gives the span every residue stays below
    const int index_bits = bits_of(max_index | 1);
    for (int i = 0; i < N_CFG; i++) {
        const uint64_t cap = cap_of_cfg(i);
        bm.sub_mult[i] = range_hs > cap ? (uint32_t)((cap << 32) / range_hs) : 0u;
        bm.sub_width[i] = bm.sub_mult[i] ? (uint32_t)(range_hs / cap) : 1u;
        uint64_t span_hs = 1;
        if (bm.sub_mult[i]) {
            const uint64_t reach = ((cap << 32) + bm.sub_mult[i] - 1) / bm.sub_mult[i];
            span_hs = (range_hs < reach ? range_hs : reach) - (cap - 1) * bm.sub_width[i] + 1;
        }
        bm.rank_bits[i] = (bm.composite && bits_of(span_hs) + bm.sh + index_bits <= 64) ? index_bits : 0;
    }
    return bm;
}

}  // namespace replay_plan
}  // namespace sylph
