// C ABI over the hit-bit model of sylph_amd/csrc/seed_plan.h ("hit bits set by LDS atomics") for tests/test_hit_bits_plan.py: g++, no HIP.
#include "../sylph_amd/csrc/seed_plan.h"

using namespace sylph::seed_plan;

extern "C" {
uint32_t hb_const(uint32_t t) { return hit_const(t); }
uint32_t hb_decode(uint32_t m) { return hit_decode(m); }
uint32_t hb_cleared(uint32_t m) { return hit_cleared(m); }
int hb_clear_after(uint32_t g) { return hit_clear_after(g) ? 1 : 0; }
uint32_t hb_word_offset(uint32_t g, uint32_t tpb) { return hit_word_offset(g, tpb); }
uint32_t hb_group_half(uint32_t g, uint32_t tpb) { return group_half(g, tpb); }
// the column as the hash loop of a wavefront with n_half half-groups leaves it: rows_used(n_half) encoded words
void hb_encode(const uint8_t* hits, uint32_t n_half, uint32_t* col) { hit_encode_model(hits, n_half, col); }
// what count_hits makes of the column of a record with nh k-mers: its mask_words(nh) words decoded `decodes` times (the kernel: once),
// the tail cleared from the last; the words above stay as they are.  Returns the record's hits.
uint32_t hb_count(uint32_t* col, uint32_t nh, uint32_t decodes) {
    const uint32_t nw = mask_words(nh);
    for (uint32_t d = 0; d < decodes; d++)
        for (uint32_t w = 0; w < nw; w++) col[w] = hit_decode(col[w]);
    if (nw) col[nw - 1] &= tail_mask(nh);
    uint32_t cnt = 0;
    for (uint32_t w = 0; w < nw; w++) cnt += (uint32_t)__builtin_popcount(col[w]);
    return cnt;
}
}
