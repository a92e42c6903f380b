// inflate_plan.h — the bookkeeping of the device-side gzip inflate (csrc/inflate.hip), host-compilable: nothing here touches HIP,
// so tests/inflate_plan_capi.cpp builds it with g++ and the CPU suite checks it against zlib (tests/test_inflate_plan.py).
//
// What the device cannot do side by side is what makes DEFLATE a chain: a block may copy from the 32 KiB before it, and where a
// block ENDS is known only once it has been decoded.  csrc/inflate.hip turns both into table work:
//   * every bit position of the file is tested for "a dynamic-Huffman block header starts here" (complete code-length code,
//     complete literal/length and distance codes, an end-of-block code) — the CANDIDATES, a superset of the true block starts;
//   * one wavefront decodes each candidate's block without the window (16-bit cells: a byte, or "byte w of the 32 KiB in front
//     of this block") and reports where it ended and how long its output is;
//   * this file walks the chain over those reports (chain_walk): start of the stream -> where that block ended -> the candidate
//     that starts there -> ... -> the final block of the member -> its trailer, the next member's header -> ...; candidates that
//     are not on the chain were never block starts and are dropped with their output;
//   * the windows are resolved down the chain in groups (inflate.hip) and the cells become bytes;
//   * CRC-32 and ISIZE of every member are checked: the CRC of a member is put together from the CRCs of 1 KiB pieces computed
//     anywhere on the device (crc32 is linear over GF(2): crc_shift, from stream_plan.h, which also holds the files of a call).
// Where every candidate's cells go — its region and how much fits, the buffer's size, the packing of the blocks decoded a second time,
// the window groups — is arithmetic at the end of this file (decode_job and its neighbours): inflate.hip only calls it.
// Anything that does not add up — a chain that breaks, a block whose output did not fit its region, a CRC that differs — makes
// the whole call decline (SYLPH_ERR_FORMAT) and the caller inflates the file with zlib as before: this road can make a file
// faster, never different.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "stream_plan.h"

namespace sylph {
namespace inflate_plan {

constexpr uint32_t WINDOW = 32768;

// ---- what a decoding wavefront reports per candidate ----------------------------------------------------------------------------
enum : uint32_t {
    ST_NONE = 0,
    ST_NEXT_DYNAMIC = 1,   // stopped in front of a dynamic block's header at end_bit (that block is another candidate's)
    ST_FINAL = 2,          // decoded a block with BFINAL set; end_bit = first bit behind its end-of-block code
    ST_ERR_CODE = 16,      // invalid Huffman code / header
    ST_ERR_DISTANCE = 17,  // a copy from further back than a window reaches (or from before the stream's start)
    ST_ERR_OVERRUN = 18,   // ran out of input
    ST_ERR_STORED = 19,    // stored block: LEN != ~NLEN
    ST_OVERFLOW = 20,      // more cells than a block may have here (2^32 - 256)
};
struct BlockResult {
    unsigned long long end_bit;
    uint32_t n_out;        // cells written
    uint32_t status;
    uint32_t flags;        // bit 0: the output holds window references; bit 1: the region was too small — end_bit and n_out are right, the
                           // cells are not all there: the block is decoded once more into a region of n_out cells
    uint32_t pad;
    unsigned long long region;   // where the block's cells begin in the cells buffer (its own region, or the spill region it moved to)
    uint32_t stats[4];     // diagnostics (SYLPH_HIP_INFLATE_STATS=1): symbols decoded, copies served from global memory, shader
                           // kilo-cycles spent on headers + tables, kilo-cycles in all
};

// ---- CRC-32 (reflected, polynomial 0xEDB88320): stream_plan.h's family in zlib's bit order --------------------------------------
// zlib's crc32() of a member = crc_finish(XOR over its pieces of crc_shift(raw register of the piece started at 0, bytes behind the
// piece in the member), the member's length); crc_byte_table / crc_raw: host reference for the tests (the device builds its slicing
// tables from the same recurrence)
using Crc = stream_plan::Crc32<true>;
constexpr uint32_t CRC_POLY = Crc::POLY;
SYLPH_HD inline uint32_t crc_multmodp(uint32_t a, uint32_t b) { return Crc::multmodp(a, b); }
inline void crc_x2n_table(uint32_t t[64]) { Crc::x2n_table(t); }
SYLPH_HD inline uint32_t crc_x8n(const uint32_t* x2n, unsigned long long n_bytes) { return Crc::x8n(x2n, n_bytes); }
SYLPH_HD inline uint32_t crc_shift(const uint32_t* x2n, uint32_t crc, unsigned long long n_bytes) { return Crc::shift(x2n, crc, n_bytes); }
inline uint32_t crc_finish(const uint32_t* x2n, uint32_t raw, unsigned long long n_bytes) { return Crc::finish(x2n, raw, n_bytes); }
inline void crc_byte_table(uint32_t t[256]) { Crc::byte_table(t); }
inline uint32_t crc_raw(const uint32_t* t, uint32_t reg, const uint8_t* p, size_t n) { return Crc::raw(t, reg, p, n); }

// ---- gzip member header (RFC 1952) ----------------------------------------------------------------------------------------------
// -> offset of the first deflate byte of the member at d[p..), or 0 when there is no well-formed header there
inline size_t member_body(const uint8_t* d, size_t n, size_t p) {
    if (p + 18 > n || d[p] != 0x1f || d[p + 1] != 0x8b || d[p + 2] != 8 || (d[p + 3] & 0xE0)) return 0;
    const unsigned flg = d[p + 3];
    size_t q = p + 10;
    if (flg & 4) { if (q + 2 > n) return 0; q += 2 + (d[q] | (size_t)d[q + 1] << 8); }
    if (flg & 8) { while (q < n && d[q]) q++; q++; }
    if (flg & 16) { while (q < n && d[q]) q++; q++; }
    if (flg & 2) q += 2;
    return q + 8 <= n ? q : 0;
}

// ---- the chain ------------------------------------------------------------------------------------------------------------------
struct ChainBlock {
    uint32_t cand;            // index into the sorted candidates
    uint32_t member;
    uint64_t out_off;         // where its bytes go in the text
    uint32_t n_out;
    uint32_t flags;           // BlockResult::flags
};
struct HostPiece {            // a member that was inflated on the host (its first block is no candidate and it is small)
    size_t gz_begin, gz_end;  // the member's bytes in the file
    uint64_t out_off;
    uint32_t member;
};
struct Member {
    uint64_t out_begin, out_end;
    uint32_t crc, isize;      // from the trailer
    bool on_host;             // inflated and checked by zlib already: no device CRC needed
    uint32_t file;            // which of the call's files it lies in
};
struct Chain {
    std::vector<ChainBlock> blocks;
    std::vector<Member> members;
    std::vector<HostPiece> host;
    uint64_t total = 0;
    std::string why;          // non-empty: the attempt is given up, and this is the reason
};

// The compressed bytes: one file, or several taken as ONE stream of gzip members (the two mates of a pair: a member never crosses from
// one file into the next, so every header, trailer and small member is read inside one segment).
using stream_plan::Segments;
using stream_plan::one_segment;

// cand_bits: sorted, unique candidate start bits (the first member's first block is among them whatever its type);
// res[i]: the report of candidate i.
// host_inflate(begin, &end, &n_out): inflate the member that starts at byte `begin` with the CPU (zlib), report where it ends
// and how many bytes it gave; false = it cannot or will not (too large).  The caller keeps the bytes.
template <class HostInflate>
Chain chain_walk(const Segments& S, const std::vector<uint64_t>& cand_bits, const BlockResult* res, HostInflate&& host_inflate) {
    Chain c;
    const size_t n = S.total();
    size_t p = 0;                                     // the current member starts at byte p
    while (true) {
        const size_t si = S.find(p);
        const uint8_t* gz = S.ptr[si];
        const size_t gb = S.base[si], gn = S.base[si + 1] - gb;
        const size_t body_local = member_body(gz, gn, p - gb);
        if (!body_local) { c.why = "no gzip member header at byte " + std::to_string(p); return c; }
        const size_t body = body_local + gb;
        const uint32_t m = (uint32_t)c.members.size();
        Member mem{c.total, c.total, 0, 0, false, (uint32_t)si};
        uint64_t bit = (uint64_t)body * 8;
        size_t trailer = 0;
        auto it = std::lower_bound(cand_bits.begin(), cand_bits.end(), bit);
        if (it == cand_bits.end() || *it != bit) {
            // the member's first block is not dynamic: a small member (an empty one ends every BGZF file) goes through zlib
            size_t end = 0;
            uint64_t n_out = 0;
            if (!host_inflate(p, &end, &n_out)) { c.why = "member at byte " + std::to_string(p) + " does not start with a dynamic block and is not small"; return c; }
            mem.on_host = true;
            mem.out_end = c.total + n_out;
            if (n_out) c.host.push_back(HostPiece{p, end, c.total, m});
            c.total += n_out;
            c.members.push_back(mem);
            p = end;
        } else {
            while (true) {
                const size_t i = (size_t)(it - cand_bits.begin());
                const BlockResult& r = res[i];
                if (r.status != ST_NEXT_DYNAMIC && r.status != ST_FINAL) {
                    c.why = "block at bit " + std::to_string(bit) + ": decoder status " + std::to_string(r.status);
                    return c;
                }
                c.blocks.push_back(ChainBlock{(uint32_t)i, m, c.total, r.n_out, r.flags});
                c.total += r.n_out;
                if (r.status == ST_FINAL) { trailer = (size_t)((r.end_bit + 7) / 8); break; }
                bit = r.end_bit;
                it = std::lower_bound(it, cand_bits.end(), bit);
                if (it == cand_bits.end() || *it != bit) { c.why = "chain breaks at bit " + std::to_string(bit) + " (no candidate starts there)"; return c; }
            }
            if (trailer + 8 > gb + gn) { c.why = "member trailer beyond the end of the file"; return c; }
            const uint8_t* t = gz + (trailer - gb);
            mem.crc = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
            mem.isize = t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
            mem.out_end = c.total;
            if ((uint32_t)(mem.out_end - mem.out_begin) != mem.isize) { c.why = "member at byte " + std::to_string(p) + ": ISIZE differs from the decoded length"; return c; }
            c.members.push_back(mem);
            p = trailer + 8;
        }
        if (p == n) return c;
        if (p > gb + gn) { c.why = "member runs past the end of the file"; return c; }
        // bytes behind a member that are no further member: zlib's gzread treats them as garbage to ignore only after at least one
        // member — needletail (flate2 MultiGzDecoder) errors; either way not this road's business
        if (p < gb + gn && !member_body(gz, gn, p - gb)) { c.why = "trailing bytes behind the last member"; return c; }
    }
}

// ---- where the cells go ---------------------------------------------------------------------------------------------------------
// one candidate for a wavefront: where its block starts, where its cells go (offset into the cells buffer) and how many fit
// limit_words (0: all the words of the launch): the words of the compressed bytes this block may read — a slice of the stream ends there
struct DecodeJob { unsigned long long start_bit, region; uint32_t cap, have_window; unsigned long long limit_words; };
constexpr uint32_t MAX_BLOCK_CELLS = 0xFFFFFF00u;      // a block of more cells is not even countable (ST_OVERFLOW)

// A single-member file says how well it deflates (ISIZE in its trailer): its blocks get 1.5 x that + 2 cells per compressed byte
// instead of the flat ratio.  Several members (BGZF ends with an empty one), a wrapped ISIZE, a ratio outside [1.5, 40] in any
// file: the flat ratio.  Every file holds a member (>= 18 bytes).
inline uint64_t region_ratio_from_isize(const Segments& files, uint64_t flat) {
    double worst = 0;
    for (size_t i = 0; i + 1 < files.base.size(); i++) {
        const uint64_t n_bytes = files.base[i + 1] - files.base[i];
        const uint8_t* tr = files.ptr[i] + n_bytes - 4;
        const double isize = (double)(tr[0] | (uint32_t)tr[1] << 8 | (uint32_t)tr[2] << 16 | (uint32_t)tr[3] << 24), r = isize / (double)n_bytes;
        if (r < 1.5 || r > 40) return flat;
        worst = std::max(worst, r);
    }
    return std::min<uint64_t>(flat, (uint64_t)(worst * 1.5) + 2);
}
// candidate i of K (cand: their sorted start bits; the first block's body starts at byte body0, the bytes end at byte_end): its
// region lies `ratio` cells per compressed byte from the buffer's start + `slack` per candidate in front of it, and holds `ratio`
// cells per byte up to the next candidate + `slack`
inline DecodeJob decode_job(uint32_t i, const uint64_t* cand, uint32_t K, uint64_t body0, uint64_t byte_end, uint64_t ratio, uint64_t slack) {
    const uint64_t b0 = cand[i] >> 3, b1 = i + 1 < K ? cand[i + 1] >> 3 : byte_end;
    return DecodeJob{cand[i], (b0 - body0) * ratio + (uint64_t)i * slack, (uint32_t)std::min<uint64_t>(MAX_BLOCK_CELLS, (b1 - b0) * ratio + slack), i != 0, 0};
}
// the cells buffer: the K candidates' regions, then (from a multiple of 64 cells) the spill arena's spill_slots regions of spill_cells
struct CellsLayout { uint64_t n_cells, spill_base, total; };
inline CellsLayout cells_layout(uint64_t span_bytes, uint32_t K, uint64_t ratio, uint64_t slack, uint64_t spill_slots, uint64_t spill_cells) {
    CellsLayout l;
    l.n_cells = span_bytes * ratio + (uint64_t)K * slack + 64;
    l.spill_base = (l.n_cells + 63) & ~(uint64_t)63;
    l.total = l.spill_base + spill_slots * spill_cells + 64;
    return l;
}
// Blocks of the chain that outgrew their region (BlockResult::flags bit 1) are decoded once more, each into a region of exactly its
// size in a buffer of their own: regions start at multiples of 64 cells (128 bytes: the ring leaves in 16-byte stores).
struct RedoPlan {
    std::vector<DecodeJob> jobs;
    std::vector<uint32_t> which;          // jobs[q] is chain block which[q]
    std::vector<uint64_t> region;         // per chain block: its region in that buffer, ~0 = it is not decoded again
    uint64_t cells = 0;                   // the buffer's size (+ 64 of slack when allocated)
};
inline RedoPlan redo_plan(const std::vector<ChainBlock>& blocks, const uint64_t* cand) {
    RedoPlan p;
    p.region.assign(blocks.size(), ~0ull);
    for (uint32_t i = 0; i < blocks.size(); i++) {
        const ChainBlock& cb = blocks[i];
        if (!(cb.flags & 2)) continue;
        p.jobs.push_back(DecodeJob{cand[cb.cand], p.cells, cb.n_out, cb.cand != 0, 0});
        p.which.push_back(i);
        p.region[i] = p.cells;
        p.cells += ((uint64_t)cb.n_out + 63) & ~(uint64_t)63;
    }
    return p;
}
// windows are resolved in groups of G chain blocks: the smallest G with G * G >= KB, at least 8
inline uint32_t window_group(uint32_t KB) {
    uint32_t G = 1;
    while ((uint64_t)G * G < KB) G++;
    return std::max(G, 8u);
}

}  // namespace inflate_plan
}  // namespace sylph
