// fasta_reads_plan.h — the bookkeeping of FASTA text read as a SAMPLE (fasta.hip: sylph_sketch_push_fasta, sylph_fasta_index_window),
// free of HIP: the order of a batch's items, the map from a byte of the gathered batch to the byte of a file's joined bases it is a
// copy of, a lane's walk over the record boundaries inside its 16 output bytes, how 16 bytes from any address are cut out of two
// aligned 16-byte words and laid into the lane's store, and which records of a window of a longer text are complete.  fa_batch_kernel
// includes this header; tests/test_fasta_reads_plan.py compiles the same header with g++ (tests/fasta_reads_plan_capi.cpp) and holds
// it against a Python model.
//
// A batch is records [first, first + n_items) of file a — in a paired session item i is record first + i of a, then record first + i
// of b — side by side behind the offsets off[0 .. n_rec] (32-bit: a batch holds fewer than 2^32 - 64 bases).  The batch is cut by
// OUTPUT bytes: tile t is bytes [4096 t, 4096 t + 4096), lane l of it owns the 16 bytes from 4096 t + 16 l on.  What a lane does depends
// on its 16 bytes alone: a record of 5 Mbp and 10^5 records of one base cost the same per byte.
#pragma once
#include <cstdint>

#include "fasta_plan.h"

namespace sylph {
namespace fasta_reads_plan {

constexpr uint32_t LANE_BYTES = fasta_plan::LANE_BYTES, TILE_LANES = fasta_plan::TILE_LANES, TILE_BYTES = fasta_plan::TILE_BYTES;
constexpr uint32_t SEARCH_STEPS = 32;                 // a batch holds fewer than 2^31 records: the binary search ends within 32 halvings

// ---- the batch's item order ---------------------------------------------------------------------------------------------------
SY_FA_HD uint64_t batch_records(uint64_t n_items, bool paired) { return paired ? 2 * n_items : n_items; }
SY_FA_HD uint32_t mate_of(uint64_t j, bool paired) { return paired ? (uint32_t)(j & 1) : 0u; }          // 0: file a, 1: file b
SY_FA_HD uint64_t record_of(uint64_t j, bool paired, uint64_t first) { return first + (paired ? j >> 1 : j); }   // in its file
// length of batch record j from the two files' record offsets (first base of every record, one entry behind the last)
SY_FA_HD uint32_t batch_len(const uint64_t* rec_off_a, const uint64_t* rec_off_b, uint64_t first, uint64_t j) {
    const bool paired = rec_off_b != nullptr;
    const uint64_t* ro = mate_of(j, paired) ? rec_off_b : rec_off_a;
    const uint64_t r = record_of(j, paired, first);
    return (uint32_t)(ro[r + 1] - ro[r]);
}

// ---- from an output byte to its record ----------------------------------------------------------------------------------------
// The record of output byte p < off[n_rec]: the LAST j with off[j] <= p (records of length 0 own no byte and are passed over).
SY_FA_HD uint64_t record_at(const uint32_t* off, uint64_t n_rec, uint64_t p) {
    uint64_t lo = 0, hi = n_rec;                       // off[lo] <= p < off[hi]
    for (uint32_t s = 0; s < SEARCH_STEPS && hi - lo > 1; s++) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}
// ... when the record in front of p was j (off[j + 1] == p): nearly always j + 1; records of length 0 in between are searched over
SY_FA_HD uint64_t record_after(const uint32_t* off, uint64_t n_rec, uint64_t j, uint64_t p) {
    if (off[j + 2] > p) return j + 1;
    uint64_t lo = j + 2, hi = n_rec;
    for (uint32_t s = 0; s < SEARCH_STEPS && hi - lo > 1; s++) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}
// where byte p of the batch, which lies in batch record j, comes from: its index in the joined bases of the record's file
SY_FA_HD uint64_t source_of(const uint32_t* off, const uint64_t* rec_off_a, const uint64_t* rec_off_b, uint64_t first, uint64_t j, uint64_t p) {
    const bool paired = rec_off_b != nullptr;
    const uint64_t* ro = mate_of(j, paired) ? rec_off_b : rec_off_a;
    return ro[record_of(j, paired, first)] + (p - off[j]);
}

// ---- a lane's walk ------------------------------------------------------------------------------------------------------------
// The lane whose first output byte is o (a multiple of 16) owns bytes [o, min(o + 16, total)): the runs of them that lie in one record
// each, in order.  piece(j, p, b0, len): bytes [p, p + len) of the batch are bytes [b0, b0 + len) of the lane and lie in record j.
// At most 16 pieces (each holds a byte), so at most 16 boundaries are crossed; every search is bounded by SEARCH_STEPS.
template <class Piece>
SY_FA_HD void lane_walk(const uint32_t* off, uint64_t n_rec, uint64_t total, uint64_t o, Piece&& piece) {
    if (o >= total) return;
    const uint64_t end = o + LANE_BYTES < total ? o + LANE_BYTES : total;
    uint64_t p = o, j = record_at(off, n_rec, o);
    for (uint32_t step = 0; step < LANE_BYTES && p < end; step++) {
        const uint64_t rec_end = off[j + 1], stop = rec_end < end ? rec_end : end;
        piece(j, p, (uint32_t)(p - o), (uint32_t)(stop - p));
        p = stop;
        if (p < end) j = record_after(off, n_rec, j, p);
    }
}

// ---- 16 bytes from any address, laid into the lane's store ---------------------------------------------------------------------
// A lane's bytes are two 64-bit words, byte b of the lane = bits [8 b, 8 b + 8) of lo (b < 8) or of hi.
// src[0 .. 16) for a source address whose low four bits are sh, from the aligned words in front of and behind it (q0 q1 | q2 q3)
SY_FA_HD void cut16(uint64_t q0, uint64_t q1, uint64_t q2, uint64_t q3, uint32_t sh, uint64_t& lo, uint64_t& hi) {
    const bool up = (sh & 8u) != 0;
    const uint64_t x0 = up ? q1 : q0, x1 = up ? q2 : q1, x2 = up ? q3 : q2;
    const uint32_t bits = (sh & 7u) * 8;
    lo = bits ? (x0 >> bits) | (x1 << (64 - bits)) : x0;
    hi = bits ? (x1 >> bits) | (x2 << (64 - bits)) : x1;
}
// the first len bytes of (lo, hi) become bytes [b0, b0 + len) of the lane's store (b0 + len <= 16, len >= 1); the other bytes stay
SY_FA_HD void lay16(uint64_t lo, uint64_t hi, uint32_t b0, uint32_t len, uint64_t& out_lo, uint64_t& out_hi) {
    // keep `len` bytes
    if (len < 8) { lo &= (1ull << (8 * len)) - 1; hi = 0; }
    else if (len < 16) hi &= (1ull << (8 * (len - 8))) - 1;      // (len == 8: mask 0)
    // move them up by b0 bytes
    if (b0 >= 8) { hi = lo << (8 * (b0 - 8)); lo = 0; }
    else if (b0) { hi = (hi << (8 * b0)) | (lo >> (64 - 8 * b0)); lo <<= 8 * b0; }
    out_lo |= lo;
    out_hi |= hi;
}

// ---- the records of a window of a longer text ------------------------------------------------------------------------------------
// A text that goes on behind the window (final == 0): a record is complete once the NEXT header has been seen, so the window's records
// are its headers but the last, and the text from the last header's '>' on is kept for the next window.  One header alone: no record,
// nothing consumed.  final != 0: every header is a record and the whole text is consumed.
SY_FA_HD uint64_t window_records(uint64_t n_headers, bool final) { return final ? n_headers : (n_headers ? n_headers - 1 : 0); }
SY_FA_HD uint64_t window_consumed(uint64_t n_headers, bool final, uint64_t n_bytes, uint64_t last_header_at) {
    return final ? n_bytes : (n_headers >= 2 ? last_header_at : 0);
}

}  // namespace fasta_reads_plan
}  // namespace sylph
