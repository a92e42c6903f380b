// bootstrap_plan.h — the arithmetic of the bootstrap confidence intervals (contain.rs:849-898 bootstrap_interval), free of HIP: where
// draw j of a fastrand stream stands without its predecessors, Lemire's bounded integer with the rejection it almost never takes, the
// value a drawn index has in `full_covs`, and the five numbers ratio_lambda (inference.rs:207-242) and ani_from_lambda
// (contain.rs:817-847) read off a resample's histogram.  bootstrap.hip includes this header, the host's statistics
// (host/inference.cpp) run their own loop through it, and tests/test_bootstrap_plan.py compiles it with g++
// (tests/bootstrap_plan_capi.cpp) and checks it against a sequential generator.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SY_BOOT_HD __host__ __device__ __forceinline__
#else
#define SY_BOOT_HD inline
#endif

namespace sylph {
namespace bootstrap_plan {

// fastrand 2.1.1 (third party, restated from its published definition): WyRand adds WY_ADD to its state on every call and returns
// the folded 128-bit product of the state and the state ^ WY_XOR.
constexpr uint64_t WY_ADD = 0x2d358dccaa6c78a5ULL, WY_XOR = 0x8bb84b93962eacc9ULL;
// Bins of a resample's histogram on the device: kept coverage values are 1 .. BINS - 1.  A genome only gets a lambda at a median
// coverage of at most 2, where the Poisson cut-off (contain.rs:666-675) keeps values below ~20; an item with a larger value declines.
constexpr uint32_t BINS = 64;

// what one resample contributes (the layout of sylph_bootstrap_summary, include/sylph_hip.h)
struct Summary {
    uint32_t n_nonzero;     // drawn values != 0
    uint32_t n_distinct;    // distinct non-zero values, saturating at 2
    uint32_t mode;          // the non-zero value drawn most often; ties go to the LARGER value (inference.rs:228-230)
    uint32_t mode_count;
    uint32_t next_count;    // how often mode + 1 was drawn, 0 if never
};

// a * b as {lo, hi}, from 32-bit halves: four 32 x 32 -> 64 multiplies, three of them with a 64-bit addend (v_mad_u64_u32 on the device).
// No partial sum overflows: (2^32 - 1)^2 + 2 (2^32 - 1) < 2^64.
SY_BOOT_HD void mul_64x64(uint64_t a, uint64_t b, uint64_t& lo, uint64_t& hi) {
    const uint32_t a0 = (uint32_t)a, a1 = (uint32_t)(a >> 32), b0 = (uint32_t)b, b1 = (uint32_t)(b >> 32);
    const uint64_t p00 = (uint64_t)a0 * b0;
    const uint64_t p01 = (uint64_t)a0 * b1 + (p00 >> 32);
    const uint64_t p10 = (uint64_t)a1 * b0 + (uint32_t)p01;
    hi = (uint64_t)a1 * b1 + (p01 >> 32) + (p10 >> 32);
    lo = (p10 << 32) | (uint32_t)p00;
}
// r * n for n below 2^32: bits 64..95 of the product and its low 64 bits (one multiply and one v_mad_u64_u32)
SY_BOOT_HD uint32_t mul_64x32(uint64_t r, uint32_t n, uint64_t& lo) {
    const uint64_t a = (uint64_t)(uint32_t)r * n;
    const uint64_t b = (uint64_t)(uint32_t)(r >> 32) * n + (a >> 32);
    lo = (b << 32) | (uint32_t)a;
    return (uint32_t)(b >> 32);
}

// state of the stream seeded with `seed` when it makes its draw j (j = 0 is the first): no draw needs its predecessor
SY_BOOT_HD uint64_t bootstrap_state(uint64_t seed, uint64_t j) { return seed + (j + 1) * WY_ADD; }
SY_BOOT_HD uint64_t wyrand_output(uint64_t state) {
    uint64_t lo, hi;
    mul_64x64(state, state ^ WY_XOR, lo, hi);
    return lo ^ hi;
}
// Lemire's bounded integer of the generator output r, fastrand's usize(..n): the high half of r * n.  *rejected is set exactly when
// fastrand would draw again (lo < n and lo < (0 - n) % n = 2^64 mod n, which is below n: the second test alone decides; the first
// keeps the division out of the way of all but n in 2^64 draws).  A rejected draw shifts every later draw of the stream by one.
SY_BOOT_HD uint64_t bounded(uint64_t r, uint64_t n, bool* rejected) {
    uint64_t lo, hi;
    if (n >> 32) mul_64x64(r, n, lo, hi);
    else hi = mul_64x32(r, (uint32_t)n, lo);
    *rejected = lo < n && lo < (0 - n) % n;
    return hi;
}
// draw j of the stream seeded with `seed`, as an index below n (n != 0), assuming no draw before it was rejected
SY_BOOT_HD uint64_t bootstrap_draw(uint64_t seed, uint64_t j, uint64_t n, bool* rejected) {
    return bounded(wyrand_output(bootstrap_state(seed, j)), n, rejected);
}

// full_covs (contain.rs:679-684) is n_total - keep zeros followed by the first `keep` coverage values of the genome, ascending
template <class T>
SY_BOOT_HD uint32_t value_of_draw(uint64_t idx, uint64_t n_total, uint64_t keep, const T* kept) {
    const uint64_t n_zero = n_total - keep;
    return idx < n_zero ? 0u : (uint32_t)kept[idx - n_zero];
}

// The summary of a histogram: hist[v] = how often the value v was drawn, v < bins; hist[0] is not looked at.
template <class T>
SY_BOOT_HD Summary summary_of_histogram(const T* hist, uint32_t bins) {
    Summary s{0, 0, 0, 0, 0};
    for (uint32_t v = 1; v < bins; v++) {
        const uint32_t c = (uint32_t)hist[v];
        if (!c) continue;
        s.n_nonzero += c;
        if (s.n_distinct < 2) s.n_distinct++;
        if (c >= s.mode_count) { s.mode = v; s.mode_count = c; }      // ascending v: a tie goes to the larger value
    }
    s.next_count = (s.mode_count && s.mode + 1 < bins) ? (uint32_t)hist[s.mode + 1] : 0u;
    return s;
}

}  // namespace bootstrap_plan
}  // namespace sylph
