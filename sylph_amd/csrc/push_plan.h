// push_plan.h — how a host batch is cut into the chunks that travel to the device one by one (sketch.hip push_host_batch),
// host-compilable: whole records (whole pairs), a bounded number of bases and records, and, for pageable input, bases and offsets that
// fit one pinned staging buffer together.  tests/test_push_plan.py checks it.
#pragma once
#include <algorithm>
#include <cstdint>

namespace sylph {
namespace push_plan {

constexpr uint64_t STAGE_BYTES = 32ull << 20;        // one pinned staging buffer (sketch.hip asserts it is sylph_ctx::STAGE_BYTES)
constexpr uint64_t STAGE_BASE_BYTES = 24ull << 20;   // what of it the bases of a pageable chunk may take; the rest is for its offsets
constexpr uint64_t MAX_CHUNK_BASES = 1ull << 31;     // a chunk is a batch of its own: 32-bit flat positions, with room for the bias
constexpr uint64_t LIMIT_SLACK = 8;                  // bases a chunk stays under its limit by (partial first and last byte, alignment)

// Chunk limits: page-locked input (DMA'd in place) is only bounded by the device slots; pageable input must fit a staging buffer,
// max_bytes of bases and (max_recs + 1) offsets.  push_chunk_bytes: the ctx option (at least 64).
struct Limits { uint64_t max_bytes, max_recs; };
inline Limits chunk_limits(bool pinned, uint64_t push_chunk_bytes) {
    return Limits{std::min<uint64_t>(push_chunk_bytes, pinned ? MAX_CHUNK_BASES : STAGE_BASE_BYTES),
                  pinned ? (4ull << 20) : ((STAGE_BYTES - STAGE_BASE_BYTES) / 8 - 2)};
}

// Records [r0, r1), bases [b0, b1) of the batch.  bpb: bases per byte of the stream (1 ASCII, 4 packed).
struct Chunk {
    uint64_t r0, r1, b0, b1;
    uint64_t n_records() const { return r1 - r0; }
    uint64_t n_bases() const { return b1 - b0; }
    uint64_t byte0(uint64_t bpb) const { return b0 / bpb; }                  // the bytes [byte0, byte1) hold every base of the chunk
    uint64_t byte1(uint64_t bpb) const { return (b1 + bpb - 1) / bpb; }
    uint64_t n_bytes(uint64_t bpb) const { return byte1(bpb) - byte0(bpb); }
    uint32_t phase(uint64_t bpb) const { return (uint32_t)(b0 % bpb); }      // bases of byte0 in front of the chunk's first
    uint64_t off_bytes() const { return (n_records() + 1) * 8; }             // the raw offsets r0 .. r1
    uint64_t staged_off_at(uint64_t bpb) const { return (n_bytes(bpb) + 7) & ~7ull; }   // where the offsets go in the staging buffer
    // bases and offsets travel through ONE staging buffer (8 bytes kept for aligning the offsets); every chunk within chunk_limits
    // does, a forced one (a record or pair beyond them) may not and then takes the plain staged copy
    bool fits_stage(uint64_t bpb) const { return n_bytes(bpb) + off_bytes() + 8 <= STAGE_BYTES; }
};

// The chunk that starts at record r0 < n_records: as many records as stay under min(max_bytes * bpb, 2^31) - 8 bases and max_recs
// records, an even number of them for pairs; a single record (pair) longer than that is a chunk of its own — forced progress.
inline Chunk next_chunk(const uint64_t* rec_off, uint64_t n_records, uint64_t r0, bool paired, uint64_t bpb, uint64_t max_bytes,
                        uint64_t max_recs) {
    const uint64_t b0 = rec_off[r0];
    uint64_t hi = std::min(n_records, r0 + max_recs);
    const uint64_t limit = b0 + std::min<uint64_t>(max_bytes * bpb, MAX_CHUNK_BASES) - LIMIT_SLACK;
    if (rec_off[hi] > limit) hi = (uint64_t)(std::upper_bound(rec_off + r0, rec_off + hi + 1, limit) - rec_off) - 1;
    if (paired) hi -= (hi - r0) & 1;
    if (hi <= r0) hi = std::min(n_records, r0 + (paired ? 2 : 1));
    return Chunk{r0, hi, b0, rec_off[hi]};
}

}  // namespace push_plan
}  // namespace sylph
