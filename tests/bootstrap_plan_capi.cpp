// C wrapper around sylph_amd/csrc/bootstrap_plan.h for tests/test_bootstrap_plan.py (g++, no HIP): the very header bootstrap.hip and
// the host's statistics include — position-addressed draws, the rejection flag, the value of a draw and the summary of a histogram,
// evaluated for arrays.  Test infrastructure: the product never runs this.
#include "../sylph_amd/csrc/bootstrap_plan.h"

using namespace sylph::bootstrap_plan;

extern "C" {

uint32_t bp_bins() { return BINS; }
uint32_t bp_summary_bytes() { return (uint32_t)sizeof(Summary); }
uint64_t bp_state(uint64_t seed, uint64_t j) { return bootstrap_state(seed, j); }
uint64_t bp_output(uint64_t state) { return wyrand_output(state); }
// draws first .. first + count - 1 of the stream seeded with `seed`, as indices below n
void bp_draws(uint64_t seed, uint64_t first, uint64_t count, uint64_t n, uint64_t* idx, uint8_t* rejected) {
    for (uint64_t i = 0; i < count; i++) {
        bool rej = false;
        idx[i] = bootstrap_draw(seed, first + i, n, &rej);
        rejected[i] = rej ? 1 : 0;
    }
}
void bp_mul(uint64_t a, uint64_t b, uint64_t* lo, uint64_t* hi) { mul_64x64(a, b, *lo, *hi); }
void bp_values(const uint64_t* idx, uint64_t count, uint64_t n_total, uint64_t keep, const uint32_t* kept, uint32_t* out) {
    for (uint64_t i = 0; i < count; i++) out[i] = value_of_draw(idx[i], n_total, keep, kept);
}
void bp_summary(const uint32_t* hist, uint32_t bins, uint32_t* out5) {
    const Summary s = summary_of_histogram(hist, bins);
    out5[0] = s.n_nonzero; out5[1] = s.n_distinct; out5[2] = s.mode; out5[3] = s.mode_count; out5[4] = s.next_count;
}

}  // extern "C"
