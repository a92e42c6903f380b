// position_road.h — the road that seeds a batch by flat position and annotates afterwards (position_road.hip): what the session
// (sketch.hip) and the genome sketch (genomes.hip) call.
#pragma once
#include "sketch_session.h"

namespace sylph {

// The survivors of one batch, sorted by flat position.  The arrays live in the ctx's scratch pool (common.h, sylph_ctx::scratch) and
// stay valid until the next call that takes those slots.
struct PosSeeds { const uint32_t* pos; const uint64_t* hash; uint32_t n; };

// Runs K1 (seeds.hip) over d_bases[0, n_bases) with capacity retry.  d_count: one device word of the caller's for the unordered
// kernel's count.  Synchronises: the stream is idle on return.
PosSeeds seeds_sorted_by_pos(sylph_ctx* ctx, const uint8_t* d_bases, uint64_t n_bases, uint32_t c, uint32_t k, uint32_t* d_count);

// K2 over the survivors `s` of a read batch (records d_off[0..n_records] over d_bases; positions carry `bias`): the session's hash
// array — and, unless `plain`, its occurrence records — from sk->n_occ on, which the caller has grown by s.n entries.
void annotate_reads(sylph_sketch* sk, const uint8_t* d_bases, const uint64_t* d_off, uint64_t n_records, uint64_t n_bases, uint32_t bias,
                    const PosSeeds& s, bool plain);

}  // namespace sylph
