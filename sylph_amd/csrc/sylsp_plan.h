// sylsp_plan.h — the arithmetic of a pre-sketched sample's table (sylph_table_from_entries, sylsp.hip), free of HIP: how a .sylsp
// file's entry stream is cut into tiles, which 16-byte vectors a tile loads and where a lane finds its three dwords among them,
// how an entry is decoded, when the stream counts as ascending, and which entries of the sorted stream stay in the table.
// sylsp.hip (kernels and host entry) includes this header; tests/test_sylsp_plan.py compiles it with g++
// (tests/sylsp_plan_capi.cpp) and checks it against numpy, a lane-by-lane replay of the unpack kernel included.
//
// The table of a .sylsp file is bincode's Vec<(u64, u32)> (types.rs:132-138): after the 8-byte length, n packed little-endian
// entries of 12 bytes — k-mer, count — with no padding.  The stride is 12, so an entry is three dwords and nothing wider is
// aligned; the stream's base is 4-byte aligned at best (file offset 8 of a page-aligned mapping: 8 bytes off a 16-byte boundary).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SY_SYLSP_HD __host__ __device__ __forceinline__
#else
#define SY_SYLSP_HD inline
#endif

namespace sylph {
namespace sylsp_plan {

constexpr uint32_t ENTRY_BYTES = 12, ENTRY_DWORDS = 3;
constexpr uint64_t TABLE_FILE_OFFSET = 8;          // the entries of a .sylsp file start behind bincode's u64 length
constexpr uint64_t MAX_ENTRIES = 1ull << 31;       // n_entries must stay below: entry indices are 32-bit on the device
constexpr uint32_t MARGIN_BYTES = 16;              // a device stream must be readable this far either side (the aligned window below)

// ---- tile geometry ---------------------------------------------------------------------------------------------------------
// One workgroup of TILE lanes unpacks TILE consecutive entries, one per lane: 768 dwords = 3 KiB of input, 48 coalesced 64-byte
// lines.  A tile's first dword lies 3 * TILE * t dwords behind the base — a multiple of 4 — so every tile of a stream sits at
// the same `phase`: the number of dwords (0..3) the base lies behind a 16-byte boundary.  The tile loads the 16-byte-aligned
// window that covers its dwords: `phase` dwords in front of its first entry belong to the previous tile (or to the margin in
// front of the stream), up to 3 behind its last one to the next tile (or to the margin behind the stream).  Vector v of the
// window goes to LDS dwords [4 v, 4 v + 4); the entry of lane l is then LDS dwords phase + 3 l + {0, 1, 2}: consecutive lanes
// read at a stride of 3 dwords, which is odd — no two lanes of a 32-lane group meet on a bank.
constexpr uint32_t TILE = 256;
constexpr uint32_t TILE_DWORDS = TILE * ENTRY_DWORDS;
constexpr uint32_t TILE_VECS_MAX = (TILE_DWORDS + 3 + 3) / 4;       // phase 3: 771 dwords in 193 vectors
constexpr uint32_t LDS_DWORDS = TILE_VECS_MAX * 4;

SY_SYLSP_HD uint32_t base_phase(uint64_t base_addr) { return (uint32_t)(base_addr >> 2) & 3u; }     // base_addr: 4-byte aligned
SY_SYLSP_HD uint32_t n_tiles(uint64_t n) { return (uint32_t)((n + TILE - 1) / TILE); }
SY_SYLSP_HD uint32_t tile_entries(uint32_t tile, uint64_t n) {
    const uint64_t first = (uint64_t)tile * TILE;
    return n - first < TILE ? (uint32_t)(n - first) : TILE;
}
// the tile's window: its first vector starts `first_dword` dwords from the stream's base (-phase for tile 0), n_vecs vectors
struct TileWindow { int64_t first_dword; uint32_t n_vecs; };
SY_SYLSP_HD TileWindow tile_window(uint32_t tile, uint64_t n, uint32_t phase) {
    TileWindow w;
    w.first_dword = (int64_t)tile * TILE_DWORDS - (int64_t)phase;
    w.n_vecs = (phase + tile_entries(tile, n) * ENTRY_DWORDS + 3) / 4;
    return w;
}
SY_SYLSP_HD uint32_t lane_lds_dword(uint32_t lane, uint32_t phase) { return phase + lane * ENTRY_DWORDS; }
// where the key of entry i - 1 lies, in dwords from the stream's base (the first lane of a tile reads its predecessor there)
SY_SYLSP_HD uint64_t prev_key_dword(uint64_t i) { return (i - 1) * ENTRY_DWORDS; }

// ---- entry decode ----------------------------------------------------------------------------------------------------------
struct Entry { uint64_t kmer; uint32_t count; };
SY_SYLSP_HD uint64_t key_from_words(uint32_t w0, uint32_t w1) { return (uint64_t)w0 | ((uint64_t)w1 << 32); }
SY_SYLSP_HD Entry entry_from_words(uint32_t w0, uint32_t w1, uint32_t w2) {
    Entry e;
    e.kmer = key_from_words(w0, w1);
    e.count = w2;
    return e;
}

// ---- order rule ------------------------------------------------------------------------------------------------------------
// The unpacked arrays are the table as they are iff the keys ascend STRICTLY: entry i breaks the order iff key[i] <= key[i - 1]
// (equal neighbours too: a repeated key keeps only its last value); entry 0 never does; tile boundaries are no exception.
SY_SYLSP_HD bool breaks_order(uint64_t i, uint64_t prev_key, uint64_t key) { return i != 0 && key <= prev_key; }

// ---- keep rule of the general road -----------------------------------------------------------------------------------------
// types.rs:117-129 rebuilds a map by insertion: a repeated key keeps the value inserted last.  After a STABLE sort by key the
// entries of one key lie in file order, so entry i of the sorted stream stays iff it is the last of its run.  A kept count of 0
// stays in the table (the probe ignores it).
SY_SYLSP_HD bool last_of_run(uint64_t i, uint64_t n, uint64_t key, uint64_t next_key) { return i + 1 == n || next_key != key; }

}  // namespace sylsp_plan
}  // namespace sylph
