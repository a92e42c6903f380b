// fasta_plan.h — the bookkeeping of the FASTA index and join (fasta.hip), free of HIP: what a lane makes of its 16 bytes of text, what
// a line is worth in the one scan over the lines, where a lane's kept bytes go, and how a tile's compacted bytes are cut into aligned
// 16-byte stores.  The kernels include this header; tests/test_fasta_plan.py compiles the same header with g++
// (tests/fasta_plan_capi.cpp) into a sequential model of the index and the join and compares it with the host reader's records.
//
// The text is read as an aligned stream of 16-byte words (text = aligned + bias); a tile is 256 lanes x 16 bytes = 4 KiB of that stream.
// Per lane every byte class is a 16-bit mask, bit b = byte b of the lane (lowest address first).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SY_FA_HD __host__ __device__ __forceinline__
#else
#define SY_FA_HD inline
#endif

namespace sylph {
namespace fasta_plan {

constexpr uint32_t LANE_BYTES = 16, TILE_LANES = 256, TILE_BYTES = LANE_BYTES * TILE_LANES;
// a text this long or longer is refused: the bases of a text then sum to less than 2^32 (the low word of the packed scan), and the
// tiles of the aligned stream stay below 2^20
constexpr uint64_t MAX_TEXT_BYTES = (1ull << 32) - 4096;
SY_FA_HD bool text_size_ok(uint64_t n_bytes) { return n_bytes > 0 && n_bytes < MAX_TEXT_BYTES; }
// n_newlines + 1 lines (the last one needs no newline): at most 2^32 - 1, so that line numbers and the header count fit 32 bits
SY_FA_HD bool line_count_ok(uint64_t n_newlines) { return n_newlines + 1 < (1ull << 32); }
constexpr uint64_t HEADER_UNIT = 1ull << 32;      // what a header line adds to the packed scan; a sequence line adds its length

// bit 7 of every byte of x that equals the byte repeated in pat4 (exact: no borrow runs from one byte into the next)
SY_FA_HD uint32_t swar_eq_flags(uint32_t x, uint32_t pat4) {
    x ^= pat4;
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | x | 0x7F7F7F7Fu);
}
// the four flag bits (bit 7 of each byte) of a dword as bits 0..3
SY_FA_HD uint32_t flags_to_bits(uint32_t f) { return (((f >> 7) & 0x01010101u) * 0x00204081u >> 21) & 0xFu; }
// mask of the lane's bytes (four dwords, lowest address first) that equal c
SY_FA_HD uint32_t lane_mask(const uint32_t w[4], uint8_t c) {
    const uint32_t p = 0x01010101u * c;
    return flags_to_bits(swar_eq_flags(w[0], p)) | flags_to_bits(swar_eq_flags(w[1], p)) << 4 | flags_to_bits(swar_eq_flags(w[2], p)) << 8 |
           flags_to_bits(swar_eq_flags(w[3], p)) << 12;
}
// mask of the lane's bytes that lie inside the text [0, n); i0 = index in the text of the lane's first byte (negative in front of it)
SY_FA_HD uint32_t lane_valid(int64_t i0, uint64_t n) {
    if (i0 >= (int64_t)n || i0 + (int64_t)LANE_BYTES <= 0) return 0u;
    const uint32_t lo = i0 < 0 ? (uint32_t)(-i0) : 0u;
    const uint32_t hi = (uint64_t)(i0 + LANE_BYTES) > n ? (uint32_t)((int64_t)n - i0) : LANE_BYTES;      // one past the last valid byte
    return (0xFFFFu >> (LANE_BYTES - hi)) & (0xFFFFu << lo);
}
// '\r' bytes of the lane that are NOT directly followed by '\n' or by the end of the text.  cr / nl / valid: masks of the lane (cr and nl
// inside valid); next_ok: the byte behind the lane is '\n' or lies behind the text
SY_FA_HD uint32_t lane_stray_cr(uint32_t cr, uint32_t nl, uint32_t valid, bool next_ok) {
    uint32_t ok = (nl >> 1) | (next_ok ? 0x8000u : 0u);
    if (!(valid & 0x8000u)) ok |= valid & ~(valid >> 1);        // the text ends inside the lane: its last byte
    return cr & ~ok & 0xFFFFu;
}

// One line of the text: raw = its bytes without the '\n', first / last = its first / last byte (any value when raw == 0).
SY_FA_HD bool line_is_header(uint64_t raw, uint8_t first) { return raw > 0 && first == '>'; }
SY_FA_HD uint64_t line_len(uint64_t raw, uint8_t last) { return raw - ((raw > 0 && last == '\r') ? 1u : 0u); }      // without its '\r'
// what the line adds to the packed scan: headers counted in the high word, sequence bytes summed in the low word
SY_FA_HD uint64_t line_value(uint64_t raw, uint8_t first, uint8_t last) { return line_is_header(raw, first) ? HEADER_UNIT : line_len(raw, last); }
// the exclusive scan of line_value at line L (and at L + 1): headers in front of the line, sequence bytes in front of the line
SY_FA_HD uint32_t scan_headers(uint64_t s) { return (uint32_t)(s >> 32); }
SY_FA_HD uint32_t scan_bases(uint64_t s) { return (uint32_t)s; }
SY_FA_HD bool scan_line_is_header(uint64_t s_line, uint64_t s_next) { return scan_headers(s_line) != scan_headers(s_next); }

// Kept bytes in front of text position p, which lies in line L (start of the line, scan at L and at L + 1): the sequence bytes in front of
// the line plus those of the line in front of p — none for a header, never more than the line's length (p may be its '\r' or '\n').
SY_FA_HD uint32_t dest_at(uint64_t p, uint64_t line_start, uint64_t s_line, uint64_t s_next) {
    const uint64_t in_line = p - line_start, len = scan_bases(s_next) - scan_bases(s_line);
    return scan_bases(s_line) + (uint32_t)(in_line < len ? in_line : len);
}
// The lane's bytes that are sequence: not '\n', not '\r' (every '\r' of an accepted text belongs to a line end), not in a header line.
// header_in: the line of the lane's first valid byte is a header; gt = mask of '>' bytes.  A '\n' makes the byte behind it a line start.
SY_FA_HD uint32_t lane_keep(uint32_t nl, uint32_t cr, uint32_t gt, uint32_t valid, bool header_in) {
    const uint32_t starts = (nl << 1) & 0xFFFFu;
    uint32_t keep = 0;
    bool hdr = header_in;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t b = 0; b < LANE_BYTES; b++) {
        const uint32_t bit = 1u << b;
        if (starts & bit) hdr = (gt & bit) != 0;
        if (!hdr) keep |= bit;
    }
    return keep & valid & ~(nl | cr);
}

// A tile's kept bytes lie compacted in LDS from index `shift` on (shift = low four bits of the address their first byte goes to), so that
// 16-byte chunk j of the LDS buffer goes to the 16-byte aligned address (first address - shift) + 16 j.  Chunks of a tile, and the bytes
// [lo, hi) of chunk j that are the tile's (a whole chunk is one aligned 16-byte store, the first and last chunk may be partial).
SY_FA_HD uint32_t store_chunks(uint32_t shift, uint32_t kept) { return kept ? (shift + kept + LANE_BYTES - 1) / LANE_BYTES : 0u; }
SY_FA_HD void store_chunk_range(uint32_t j, uint32_t shift, uint32_t kept, uint32_t& lo, uint32_t& hi) {
    const uint32_t a = j * LANE_BYTES, b = a + LANE_BYTES, end = shift + kept;
    lo = (a > shift ? a : shift) - a;
    hi = (b < end ? b : end) - a;
}

}  // namespace fasta_plan
}  // namespace sylph
