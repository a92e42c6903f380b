// C ABI over what the read kernel's lanes carry through their hash loop (sylph_amd/csrc/seed_plan.h: rel_bias / record_rel32, MarkerBases,
// stream_word_range, emission_lane) for tests/test_pass_state_plan.py: g++, no HIP.
#include "../sylph_amd/csrc/seed_plan.h"

using namespace sylph::seed_plan;

extern "C" {
uint32_t ps_emission_lane(uint32_t i, uint32_t len4) { return emission_lane(i, len4); }
uint64_t ps_emission_rank(uint32_t i, uint32_t nh, int avx2_compat) { return emission_rank(i, nh, avx2_compat); }
// every i < nh of a record with nh k-mers (a multiple of 4, nh >= 4) from i_lo on, at most n_i of them: how many differ from the division
uint64_t ps_emission_mismatches(uint32_t nh, uint32_t i_lo, uint32_t n_i) {
    const uint32_t len4 = nh >> 2;
    uint64_t bad = 0;
    for (uint32_t i = i_lo; i < nh && i - i_lo < n_i; i++) {
        const uint32_t lane = i / len4;
        bad += emission_lane(i, len4) != lane;
        bad += emission_rank(i, nh, 1) != (uint64_t)(i - lane * len4) * 4 + lane;
        bad += emission_rank(i, nh, 0) != i;
    }
    return bad;
}
uint64_t ps_n_hashed_kmers(uint64_t L, uint32_t k, int avx2_compat, int positions) { return n_hashed_kmers(L, k, avx2_compat, positions); }
uint32_t ps_record_rel(uint64_t start, uint32_t bias, int64_t a0) { return record_rel(start, bias, a0); }
uint32_t ps_rel_bias(uint32_t bias, int64_t a0) { return rel_bias(bias, a0); }
uint32_t ps_record_rel32(uint64_t start, uint32_t rb) { return record_rel32(start, rb); }
// starts[0 .. n): how many differ between the 64-bit step and the 32-bit one
uint64_t ps_rel_mismatches(const uint64_t* starts, uint64_t n, uint32_t bias, int64_t a0) {
    const uint32_t rb = rel_bias(bias, a0);
    uint64_t bad = 0;
    for (uint64_t j = 0; j < n; j++) bad += record_rel32(starts[j], rb) != record_rel(starts[j], bias, a0);
    return bad;
}
void ps_single_marker_bases(uint32_t rel, uint32_t L, uint32_t* out) { const MarkerBases m = single_marker_bases(rel, L); out[0] = m.ba; out[1] = m.bb; }
void ps_pair_marker_bases(uint32_t rel1, uint32_t rel2, uint32_t L1, uint32_t L2, uint32_t* out) {
    const MarkerBases m = pair_marker_bases(rel1, rel2, L1, L2); out[0] = m.ba; out[1] = m.bb;
}
void ps_stream_word_range(int64_t a0, uint64_t n_al, uint32_t n_words, uint32_t* out) { stream_word_range(a0, n_al, n_words, out[0], out[1]); }
int ps_block_starts_inside(uint32_t blk) { return block_starts_inside(blk) ? 1 : 0; }
int64_t ps_block_a0(uint32_t blk, uint32_t rt) { return block_a0(blk, rt); }
uint32_t ps_stream_words(uint32_t rt) { return stream_words(rt); }
}
