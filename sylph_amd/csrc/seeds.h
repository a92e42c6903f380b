// seeds.h — the host entries of the position seeding kernels K1 (seeds.hip), for the position road (position_road.hip).
#pragma once
#include "common.h"

namespace sylph {

// Unordered K1 on ctx->stream: survivors in any order, counted in *d_count (zeroed by the caller, read by the caller; it keeps
// counting beyond out_cap).
void launch_seeds(sylph_ctx* ctx, const uint8_t* d_bases, uint32_t n_bases, uint32_t c, uint32_t k, uint64_t* d_out_hash,
                  uint32_t* d_out_pos, uint32_t out_cap, uint32_t* d_count);

// Ordered K1: fills per-tile slots + tile counts; the caller scans tile_count and calls launch_compact_slots.
uint32_t seeds_slot_capacity(uint32_t c);
uint32_t seeds_n_tiles(uint64_t n_bases);
uint32_t seeds_tile_bases();
// tile_list == nullptr: first pass over all tiles of the batch.  Otherwise: redo pass over `n_list` overflowed tiles with
// seeds_tile_bases() slots each (d_slot_* = the spill regions), recording each tile's spill slot in d_spill_slot_of_tile.
void launch_seeds_slots(sylph_ctx* ctx, const uint8_t* d_bases, uint32_t n_bases, uint32_t c, uint32_t k, uint32_t slot_cap,
                        uint64_t* d_slot_hash, uint32_t* d_slot_pos, uint32_t* d_tile_count, SpillState* d_spill,
                        const uint32_t* d_tile_list, uint32_t n_list, uint32_t* d_spill_slot_of_tile);
void launch_compact_slots(sylph_ctx* ctx, const uint64_t* d_slot_hash, const uint32_t* d_slot_pos, const uint32_t* d_tile_count,
                          const uint32_t* d_tile_off, uint32_t n_tiles, uint32_t slot_cap, const uint64_t* d_spill_hash,
                          const uint32_t* d_spill_pos, const uint32_t* d_spill_slot_of_tile, uint32_t* d_out_pos,
                          uint64_t* d_out_hash);

}  // namespace sylph
