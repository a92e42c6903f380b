// C wrapper around sylph_amd/csrc/push_plan.h for tests/test_push_plan.py (g++, no HIP): the very header sketch.hip's push_host_batch
// includes — how a host batch is cut into chunks, evaluated over whole offset tables.
// Test infrastructure: the product never runs this.
#include "../sylph_amd/csrc/push_plan.h"

using namespace sylph::push_plan;

extern "C" {

// STAGE_BYTES, STAGE_BASE_BYTES, MAX_CHUNK_BASES, LIMIT_SLACK
void pp_constants(uint64_t* out) { out[0] = STAGE_BYTES; out[1] = STAGE_BASE_BYTES; out[2] = MAX_CHUNK_BASES; out[3] = LIMIT_SLACK; }

// max_bytes, max_recs
void pp_limits(int pinned, uint64_t push_chunk_bytes, uint64_t* out) {
    const Limits l = chunk_limits(pinned != 0, push_chunk_bytes);
    out[0] = l.max_bytes; out[1] = l.max_recs;
}

// The walk of push_host_batch: next_chunk from record 0, each chunk starting where the one before ended, until one ends at n_records.
// Per chunk 10 words: r0, r1, b0, b1, byte0, byte1, phase, off_bytes, staged_off_at, fits_stage.  Returns the number of chunks, or -1 when
// there are more than `cap` of them or one makes no progress (out then holds the chunks so far).
int64_t pp_chunks(const uint64_t* rec_off, uint64_t n_records, int paired, uint64_t bpb, uint64_t max_bytes, uint64_t max_recs, uint64_t* out,
                  uint64_t cap) {
    uint64_t n = 0;
    for (uint64_t r0 = 0; r0 < n_records; n++) {
        if (n == cap) return -1;
        const Chunk c = next_chunk(rec_off, n_records, r0, paired != 0, bpb, max_bytes, max_recs);
        uint64_t* o = out + n * 10;
        o[0] = c.r0; o[1] = c.r1; o[2] = c.b0; o[3] = c.b1; o[4] = c.byte0(bpb); o[5] = c.byte1(bpb); o[6] = c.phase(bpb);
        o[7] = c.off_bytes(); o[8] = c.staged_off_at(bpb); o[9] = c.fits_stage(bpb) ? 1 : 0;
        if (c.r0 != r0 || c.r1 <= r0 || c.n_records() != c.r1 - c.r0 || c.n_bases() != c.b1 - c.b0 || c.n_bytes(bpb) != o[5] - o[4]) return -1;
        r0 = c.r1;
    }
    return (int64_t)n;
}

}  // extern "C"
