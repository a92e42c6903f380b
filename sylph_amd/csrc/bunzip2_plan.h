// bunzip2_plan.h — the bookkeeping of the device-side bzip2 decoder (csrc/bunzip2.hip), host-compilable: nothing here touches HIP,
// so tests/bunzip2_plan_capi.cpp builds it with g++ and the CPU suite checks it against Python's bz2 (tests/test_bunzip2_host.py).
//
// A bzip2 stream is "BZh" + a level '1'-'9', then bit-aligned blocks, each behind the 48-bit magic 0x314159265359 and holding at most
// level x 100 000 bytes of BWT column, then the end-of-stream magic 0x177245385090, the stream's combined CRC and padding to a byte.
// Blocks carry no length, so where one ENDS is known only once it has been decoded.  csrc/bunzip2.hip makes that table work:
//   * every bit position of the file is tested for the block magic — the CANDIDATES, a superset of the true block starts (a false
//     one turns up with odds 2^-48 per bit position);
//   * one wavefront decodes each candidate and reports where its end-of-block symbol ended (BlockReport);
//   * this file walks the chain over those reports (chain_step, one link at a time; ChainWalk is its whole-file use,
//     bunzip2_stream_plan.h SliceWalk the resumable one): the stream header -> the candidate at bit 32 -> the one where that
//     block ended -> ... -> the end-of-stream magic -> the combined CRC -> the next stream's header -> ...; a candidate that is not
//     on the chain was never a block start;
//   * the block CRCs (CRC-32 with polynomial 0x04C11DB7, MSB first: the non-reflected form, unlike gzip's) are put together from
//     the CRCs of pieces computed anywhere on the device (crc_shift: the CRC is linear over GF(2); the arithmetic is stream_plan.h's,
//     shared with gzip's bit order, as is Segments, the files of a call), and the run-length decode of a block is a scan of small
//     state-transfer functions (RleFn).
// Anything that does not add up makes the whole call decline (SYLPH_ERR_FORMAT): the caller decodes the file with libbz2 as before.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "stream_plan.h"

namespace sylph {
namespace bunzip2_plan {

constexpr uint64_t BLOCK_MAGIC = 0x314159265359ull;
constexpr uint64_t EOS_MAGIC = 0x177245385090ull;
constexpr uint32_t MAX_BLOCK = 900000;        // bytes of BWT column in a block at level 9
constexpr uint32_t MAX_SELECTORS = 18002;     // what libbz2 1.0.8 keeps (2 + 900 000 / 50); a block that sends more is declined

// ---- CRC-32/BZIP2 (polynomial 0x04C11DB7, MSB first): stream_plan.h's family in the bit order that is not reflected ------------
// a block's CRC = crc_finish(XOR over its pieces of crc_shift(register of the piece started at 0, bytes behind the piece in the
// block), the block's length)
using Crc = stream_plan::Crc32<false>;
constexpr uint32_t CRC_POLY = Crc::POLY;
SYLPH_HD inline uint32_t crc_multmodp(uint32_t a, uint32_t b) { return Crc::multmodp(a, b); }
inline void crc_x2n_table(uint32_t t[64]) { Crc::x2n_table(t); }
SYLPH_HD inline uint32_t crc_x8n(const uint32_t* x2n, unsigned long long n_bytes) { return Crc::x8n(x2n, n_bytes); }
SYLPH_HD inline uint32_t crc_shift(const uint32_t* x2n, uint32_t reg, unsigned long long n_bytes) { return Crc::shift(x2n, reg, n_bytes); }
inline uint32_t crc_finish(const uint32_t* x2n, uint32_t raw, unsigned long long n_bytes) { return Crc::finish(x2n, raw, n_bytes); }
inline void crc_byte_table(uint32_t t[256]) { Crc::byte_table(t); }
SYLPH_HD inline uint32_t crc_raw(const uint32_t* t, uint32_t reg, const uint8_t* p, size_t n) { return Crc::raw(t, reg, p, n); }
// a stream's combined CRC, block after block
inline uint32_t combine_stream(uint32_t c, uint32_t block_crc) { return ((c << 1) | (c >> 31)) ^ block_crc; }

// ---- the run-length decode as a scan -------------------------------------------------------------------------------------------
// The inverse BWT gives the "RLE1" text: after 4 equal bytes the next byte is a repeat count (0-255) of the fourth.  The state in
// front of a byte is k = the length of the current run of equal non-count bytes (4: the byte is a count).  Seen from a chunk that
// begins with byte b, what came before matters only through eff_k: 4 when a count is due, k in 1..3 when the run's byte is b,
// 0 otherwise.  RleFn is the chunk's map eff_k -> (k behind its last byte, bytes it writes); behind a chunk with k_out >= 1 the
// run's byte is the chunk's last byte.
struct RleFn {
    uint32_t len[5];
    uint32_t k_out;        // 3 bits per eff_k
    SYLPH_HD uint32_t kout(uint32_t k) const { return (k_out >> (3 * k)) & 7; }
};
SYLPH_HD inline RleFn rle_fn(const uint8_t* p, uint32_t n) {
    RleFn f;
    f.k_out = 0;
    for (uint32_t k0 = 0; k0 < 5; k0++) {
        uint32_t k = k0, len = 0;
        uint8_t c = p[0];                          // (eff_k 1..3: the run's byte is the first byte)
        for (uint32_t i = 0; i < n; i++) {
            const uint8_t x = p[i];
            if (k == 4) { len += x; k = 0; }
            else if (k > 0 && x == c) { k++; len++; }
            else { c = x; k = 1; len++; }
        }
        f.len[k0] = len;
        f.k_out |= k << (3 * k0);
    }
    return f;
}
// eff_k in front of a chunk that begins with `first`, behind a chunk that ended in state k_out with last byte `last`
SYLPH_HD inline uint32_t rle_eff(uint32_t k_out, uint8_t last, uint8_t first) {
    return k_out == 4 ? 4u : (k_out >= 1 && last == first ? k_out : 0u);
}
// expands p[0..n) from eff_k into out (run byte in front: `prev`, used when eff_k = 4); returns the bytes written
SYLPH_HD inline uint32_t rle_expand(const uint8_t* p, uint32_t n, uint32_t k, uint8_t prev, uint8_t* out) {
    uint8_t c = k == 4 ? prev : p[0];
    uint32_t o = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t x = p[i];
        if (k == 4) { for (uint32_t r = 0; r < x; r++) out[o++] = c; k = 0; }
        else if (k > 0 && x == c) { k++; out[o++] = x; }
        else { c = x; k = 1; out[o++] = x; }
    }
    return o;
}

// ---- what a decoding wavefront reports per candidate -------------------------------------------------------------------------
enum : uint32_t {
    ST_OK = 0,
    ST_ERR_MAGIC = 16,      // no block magic at the candidate (cannot happen: the scan found one)
    ST_ERR_HEADER = 17,     // symbol map / groups / selectors / code lengths out of range
    ST_ERR_CODE = 18,       // a Huffman code longer than 20 bits or outside the table, a selector past the last
    ST_ERR_SIZE = 19,       // more than MAX_BLOCK bytes, or a run too long
    ST_ERR_ORIG = 20,       // origPtr outside the block
    ST_ERR_OVERRUN = 21,    // ran out of input
    ST_ERR_SELECTORS = 22,  // more selectors than libbz2 keeps
};
struct BlockReport {
    unsigned long long end_bit;   // first bit behind the end-of-block symbol
    uint32_t status;
    uint32_t n;                   // bytes of BWT column
    uint32_t orig_ptr;
    uint32_t crc;                 // the block CRC the stream stores
    uint32_t randomised;
    uint32_t symbols;             // (diagnostics) symbols decoded
};

// ---- the chain ------------------------------------------------------------------------------------------------------------------
using stream_plan::Segments;      // the files of one call: each its own bytes; in the device's buffer they lie back to back
// the k <= 48 bits at `bit` (MSB-first) of d[0, n), zero beyond n bytes
inline uint64_t bits_at(const uint8_t* d, uint64_t n, uint64_t bit, unsigned k) {
    uint64_t v = 0;
    for (unsigned i = 0; i < k; i++) {
        const uint64_t b = bit + i;
        v = (v << 1) | (b / 8 < n ? (d[b / 8] >> (7 - b % 8)) & 1u : 0u);
    }
    return v;
}
inline int stream_level(const uint8_t* d, uint64_t n, uint64_t p) {
    return p + 4 <= n && d[p] == 'B' && d[p + 1] == 'Z' && d[p + 2] == 'h' && d[p + 3] >= '1' && d[p + 3] <= '9' ? d[p + 3] - '0' : 0;
}

struct ChainBlock { uint32_t cand, file, stream; uint32_t n; };

// Where a file's chain stands: `bit` (of the FILE) is where the next block / end-of-stream magic starts (in_stream), or 8 x the byte of
// the next stream header.  Everything a walk needs to go on from there, so it is also what the streamed decoder carries from one slice
// to the next (bunzip2_stream_plan.h Carry).
struct ChainPos {
    uint64_t bit = 0;
    bool in_stream = false;
    int level = 0;               // in_stream: that stream's level ...
    uint32_t combined = 0;       // ... and its combined CRC so far
    uint64_t n_streams = 0;      // streams begun / blocks taken so far
    uint64_t n_blocks = 0;
};
// what `find` of chain_step answers for the block magic at a bit of the file: the candidate there and its report (end_bit: of the FILE),
// or HOLD: the walk waits in front of that block (its report is not in yet; the slice ends there)
struct BlockAt {
    enum What { HAVE, HOLD } what = HOLD;
    size_t cand = 0;
    const BlockReport* r = nullptr;
    uint64_t end_bit = 0;
};
enum class Link { HEADER, TRAILER, BLOCK, HOLD, DECLINED };
// ONE link of a file's chain, the only copy of it: a stream header, an end-of-stream trailer with its combined CRC, or a block whose
// report `find(bit, why)` hands over.  Headers and trailers are read in d[0, fn), the host's copy of the file, which is whole.
// DECLINED: `why` says what does not add up.  BLOCK: *got is the block taken.
template <class Find>
Link chain_step(const uint8_t* d, uint64_t fn, uint32_t file, ChainPos& p, Find&& find, std::string& why, BlockAt* got) {
    const uint64_t lb = p.bit;
    if (!p.in_stream) {
        p.level = stream_level(d, fn, lb / 8);
        if (!p.level) { why = "no bzip2 stream header at byte " + std::to_string(lb / 8) + " of file " + std::to_string(file); return Link::DECLINED; }
        p.in_stream = true;
        p.combined = 0;
        p.bit += 32;
        p.n_streams++;
        return Link::HEADER;
    }
    const uint64_t m = bits_at(d, fn, lb, 48);
    if (m == EOS_MAGIC) {
        if (lb + 80 > fn * 8) { why = "end-of-stream trailer beyond the end of the file"; return Link::DECLINED; }
        const uint32_t stored = (uint32_t)bits_at(d, fn, lb + 48, 32);
        if (stored != p.combined) { why = "stream " + std::to_string(p.n_streams - 1) + ": combined CRC differs"; return Link::DECLINED; }
        p.in_stream = false;
        p.bit = (lb + 80 + 7) / 8 * 8;
        return Link::TRAILER;
    }
    if (m != BLOCK_MAGIC) { why = "chain breaks at bit " + std::to_string(lb) + " of file " + std::to_string(file) + " (neither a block nor the end of the stream)"; return Link::DECLINED; }
    const BlockAt at = find(lb, why);
    if (!why.empty()) return Link::DECLINED;
    if (at.what == BlockAt::HOLD) return Link::HOLD;
    const BlockReport& r = *at.r;
    if (r.status != ST_OK) { why = "block at bit " + std::to_string(lb) + ": decoder status " + std::to_string(r.status); return Link::DECLINED; }
    if (r.randomised) { why = "block at bit " + std::to_string(lb) + " is randomised"; return Link::DECLINED; }
    if (r.n > (uint32_t)p.level * 100000u) { why = "block at bit " + std::to_string(lb) + " is larger than the stream's level allows"; return Link::DECLINED; }
    if (at.end_bit + 48 > fn * 8) { why = "block at bit " + std::to_string(lb) + " runs past the end of its file"; return Link::DECLINED; }
    if (at.end_bit <= lb) { why = "block at bit " + std::to_string(lb) + " does not move on"; return Link::DECLINED; }
    p.combined = combine_stream(p.combined, r.crc);
    p.bit = at.end_bit;
    p.n_blocks++;
    *got = at;
    return Link::BLOCK;
}

// The whole-file use of chain_step: the files of a call back to back in one buffer, one chain through all of them (file 1's blocks
// come behind all of file 0's).  Walks one step at a time as candidates' reports come in (the device decodes them in batches, in bit
// order): step() follows the chain while the report it needs is there; it stops in front of a candidate index >= `have`.
struct ChainWalk {
    const Segments* S = nullptr;
    const std::vector<uint64_t>* cand = nullptr;   // sorted candidate bits (of the buffer)
    std::vector<ChainBlock> blocks;
    uint32_t n_streams = 0;
    std::string why;                               // non-empty: declined, and why
    bool done = false;
    uint32_t file = 0;
    ChainPos pos;                                  // in `file`
    size_t next_cand = 0;                          // candidates before it lie behind the chain

    void start(const Segments* s, const std::vector<uint64_t>* c) {
        S = s; cand = c;
        file = 0; pos = ChainPos{}; done = false;
        skip_empty_files();
    }
    void skip_empty_files() {        // (a file without a byte is no bzip2 file)
        if (file + 1 < S->base.size() && S->base[file + 1] == S->base[file]) why = "file " + std::to_string(file) + " is empty";
    }
    // -> index of the candidate at `b`, or SIZE_MAX
    size_t find(uint64_t b) {
        while (next_cand < cand->size() && (*cand)[next_cand] < b) next_cand++;
        return next_cand < cand->size() && (*cand)[next_cand] == b ? next_cand : SIZE_MAX;
    }
    // follow the chain; reports of candidates [0, have) are known.  Returns false when it stopped for a report it has not got.
    bool step(const BlockReport* rep, size_t have) {
        while (!done && why.empty()) {
            const uint64_t fb = S->base[file], fn = S->base[file + 1] - fb;   // the file's bytes; the candidates count bits of the whole buffer
            BlockAt got;
            const Link l = chain_step(S->ptr[file], fn, file, pos, [&](uint64_t lb, std::string& w) {
                BlockAt at;
                const size_t i = find(fb * 8 + lb);
                if (i == SIZE_MAX) { w = "block magic at bit " + std::to_string(lb) + " is no candidate"; return at; }
                if (i >= have) return at;
                at.what = BlockAt::HAVE;
                at.cand = i;
                at.r = &rep[i];
                at.end_bit = rep[i].end_bit - fb * 8;
                return at;
            }, why, &got);
            n_streams = (uint32_t)pos.n_streams;
            if (l == Link::DECLINED) return true;
            if (l == Link::HOLD) return false;
            if (l == Link::BLOCK) blocks.push_back(ChainBlock{(uint32_t)got.cand, file, n_streams - 1, got.r->n});
            if (l == Link::TRAILER && pos.bit == fn * 8) {
                file++;
                pos.bit = 0;
                if (file + 1 == S->base.size()) { done = true; return true; }
                skip_empty_files();
            }
        }
        return true;
    }
};

}  // namespace bunzip2_plan
}  // namespace sylph
