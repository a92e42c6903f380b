// C wrapper around sylph_amd/csrc/seed_plan.h for tests/test_seed_plan.py (g++, no HIP): the very header reads.hip, reads_block.h,
// seeds.hip and partition.h include — the geometry of the seeding kernels, evaluated for whole ranges of blocks, records and k-mers.
// Test infrastructure: the product never runs this.
#include "../sylph_amd/csrc/seed_plan.h"

#include <cstring>

using namespace sylph::seed_plan;

extern "C" {

// RTPB, RTPB_RAGGED, RT_MIN, RT_MAX, RH, RPAD, MASKW, OFFS_256, NH_MAX, TPB, WPT, TILE_WORDS, TILE_BASES, HALO_WORDS, LIST_CAP, STAGE_CAP, FLUSH_AT
void sp_constants(int32_t* out) {
    const int32_t v[17] = {RTPB, RTPB_RAGGED, RT_MIN, RT_MAX, RH, RPAD, MASKW, OFFS_256, NH_MAX, TPB, WPT, TILE_WORDS, TILE_BASES, HALO_WORDS, LIST_CAP, STAGE_CAP, FLUSH_AT};
    memcpy(out, v, sizeof v);
}
// tpb, rt, n_blk, slot_cap, spill_cap, lds_bytes, n_expect
void sp_plan(uint64_t n_bases, uint64_t n_records, uint32_t bias, uint32_t c, uint32_t k, int ragged_tpb_wanted, uint64_t* out) {
    const ReadsBlockPlan p = reads_block_plan(n_bases, n_records, bias, c, k, ragged_tpb_wanted != 0);
    out[0] = (uint64_t)p.tpb; out[1] = p.rt; out[2] = p.n_blk; out[3] = p.slot_cap; out[4] = p.spill_cap; out[5] = p.lds_bytes; out[6] = p.n_expect;
}
uint32_t sp_slot_capacity(uint64_t full, uint64_t expect) { return slot_capacity(full, expect); }
uint32_t sp_stream_words(uint32_t rt) { return stream_words(rt); }
uint32_t sp_lds_words(uint32_t rt) { return lds_words(rt); }

// Over every stream base rel a record that starts in a block of rt coordinates can have and every nh_max in [0, nh_top]: out[0] = the
// highest word the hash loop reads; out[1] = the highest word of a 64-bit window — a survivor's k-mer (index < nh_top), the second marker
// of a single record (rel + L / 2), the mate 2 behind a mate 1 of the block (rel + L1), L and L1 up to RH; out[2] = the same for the
// mate-1 windows of a block that starts with a mate 2 (stream base rel - L1 of a mate 2 at rel).  out[3] = the stream base of a mate 1 of RH bases in
// front of a mate 2 on the block's first coordinate, from block_a0 / record_rel as the kernel computes it (as a signed number: it must not be negative).
void sp_window_max(uint32_t rt, uint32_t nh_top, int64_t* out) {
    uint32_t loop_hi = 0, win_hi = 0, mate_hi = 0;
    for (uint32_t rel = RH; rel < RH + rt; rel++) {
        for (uint32_t nh_max = 0; nh_max <= nh_top; nh_max++) { const uint32_t h = hash_hi_word(rel, nh_max); if (h > loop_hi) loop_hi = h; }
        const uint32_t w[3] = {win64_hi_word(rel + (nh_top ? nh_top - 1 : 0)), win64_hi_word(rel + RH / 2), win64_hi_word(rel + RH)};
        for (uint32_t x : w) if (x > win_hi) win_hi = x;
    }
    for (uint32_t b = 0; b < RH + rt; b++) { const uint32_t x = win64_hi_word(b); if (x > mate_hi) mate_hi = x; }   // rel - L1, L1 in [0, RH]
    // block 3 at bias 5: mate 2 starts on the block's first coordinate, its mate 1 RH bases earlier
    const uint64_t s2 = block_begin(3, rt) - 5, s1 = s2 - RH;
    out[0] = loop_hi; out[1] = win_hi; out[2] = mate_hi;
    out[3] = (int64_t)(s1 + 5) - block_a0(3, rt);
    if ((int64_t)record_rel(s1, 5, block_a0(3, rt)) != out[3] || record_rel(s2, 5, block_a0(3, rt)) != (uint32_t)RH) out[3] = -1;
}

// The hash loop's stores of one lane that hashes record slot `slot` in a wavefront whose longest record has nh_max k-mers: hit[t] says
// whether k-mer t passed (16 * groups entries).  The loop shifts a k-mer's verdict into bit 0 of `mask` (kmer_step); whole groups are
// stored as they are, the odd half-group shifted up by 8.  col[w] = word w of the slot's mask column afterwards (MASKW words; the array
// starts out as `fill`).
void sp_mask_sim(const uint8_t* hit, uint32_t nh_max, uint32_t tpb, uint32_t slot, uint32_t fill, uint32_t* col) {
    uint32_t* s_mask = new uint32_t[(size_t)MASKW * tpb];
    for (size_t i = 0; i < (size_t)MASKW * tpb; i++) s_mask[i] = fill;
    // the record's column seen as 16-bit halves, little-endian as on the device (memcpy: the host compiler may not alias the two views)
    auto store_half = [&](uint32_t half, uint16_t v) { memcpy(reinterpret_cast<unsigned char*>(s_mask + slot) + 2 * (size_t)half, &v, 2); };
    const uint32_t n_half = half_groups(nh_max), n_grp = n_half >> 1;
    for (uint32_t g = 0; g < n_grp; g++) {
        uint32_t mask = 0;
        for (uint32_t t = 0; t < 16; t++) mask = 2 * mask + hit[g * 16 + t];
        store_half(group_half(g, tpb), (uint16_t)mask);
    }
    if (n_half & 1u) {
        uint32_t mask = 0;
        for (uint32_t t = 0; t < 8; t++) mask = 2 * mask + hit[n_grp * 16 + t];
        store_half(group_half(n_grp, tpb), (uint16_t)(mask << 8));
    }
    for (uint32_t w = 0; w < (uint32_t)MASKW; w++) col[w] = s_mask[(size_t)w * tpb + slot];
    delete[] s_mask;
}
uint32_t sp_kmer_word(uint32_t i) { return kmer_word(i); }
uint32_t sp_kmer_bit(uint32_t i) { return kmer_bit(i); }
uint32_t sp_mask_words(uint32_t nh) { return mask_words(nh); }
uint32_t sp_tail_mask(uint32_t nh) { return tail_mask(nh); }
uint32_t sp_half_groups(uint32_t nh) { return half_groups(nh); }
uint32_t sp_deal_bin(uint32_t nh) { return deal_bin(nh); }
uint32_t sp_rows_used(uint32_t hg_max) { return rows_used(hg_max); }
int sp_listed(uint32_t total, uint32_t rows, uint32_t tpb) { return listed(total, rows, tpb) ? 1 : 0; }

// blk_rec[b] for b in [0, n_blk] (what block_records_kernel writes) and rel[r] = the stream base of record r in ITS block
void sp_blocks(const uint64_t* off, uint64_t n_rec, uint32_t bias, uint32_t rt, uint32_t n_blk, uint64_t* blk_rec, uint32_t* rel) {
    for (uint32_t b = 0; b <= n_blk; b++) blk_rec[b] = first_record_of_block(off, n_rec, bias, b, rt);
    for (uint32_t b = 0; b < n_blk; b++)
        for (uint64_t r = blk_rec[b]; r < blk_rec[b + 1]; r++) rel[r] = record_rel(off[r], bias, block_a0(b, rt));
}
int64_t sp_block_a0(uint32_t blk, uint32_t rt) { return block_a0(blk, rt); }

uint32_t sp_xcd_deal(uint32_t i, uint32_t n) { return xcd_deal(i, n); }
uint32_t sp_xcd_positions(uint32_t n) { return xcd_positions(n); }
uint32_t sp_xcd_tail_cut(uint32_t n, uint32_t tail_pct) { return xcd_tail_cut(n, tail_pct); }

// word offsets of blk_rec, blk_count, spill_slot, blk_off, state_words from the buffer's start, then its size in bytes
void sp_slot_meta(uint32_t n_blk, uint64_t state_bytes, uint64_t* out) {
    out[5] = SlotMeta::bytes(n_blk, state_bytes);
    uint32_t* const base = new uint32_t[out[5] / 4];
    const SlotMeta m(base, n_blk);
    uint32_t* const p[5] = {m.blk_rec, m.blk_count, m.spill_slot, m.blk_off, m.state_words};
    for (int i = 0; i < 5; i++) out[i] = (uint64_t)(p[i] - base);
    delete[] base;
}

}  // extern "C"
