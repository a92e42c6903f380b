// C entry points over sylph_amd/csrc/sylsp_plan.h for tests/test_sylsp_plan.py (ctypes) and tests/sylsp_plan_sanitize_main.cpp:
// the plan's functions one by one, sp_model_unpack — the unpack launch of sylsp.hip replayed on the host, tile by tile and lane by
// lane, with the very functions the kernel calls — and sp_model_table, the general road (stable sort, last-of-run flags, exclusive
// sum, compaction) with the plan's keep rule.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "../sylph_amd/csrc/sylsp_plan.h"

using namespace sylph::sylsp_plan;

extern "C" {

void sp_constants(uint64_t* out) {
    out[0] = ENTRY_BYTES; out[1] = ENTRY_DWORDS; out[2] = TABLE_FILE_OFFSET; out[3] = MAX_ENTRIES; out[4] = MARGIN_BYTES;
    out[5] = TILE; out[6] = TILE_DWORDS; out[7] = TILE_VECS_MAX; out[8] = LDS_DWORDS;
}
uint32_t sp_base_phase(uint64_t addr) { return base_phase(addr); }
uint32_t sp_n_tiles(uint64_t n) { return n_tiles(n); }
uint32_t sp_tile_entries(uint32_t tile, uint64_t n) { return tile_entries(tile, n); }
void sp_tile_window(uint32_t tile, uint64_t n, uint32_t phase, int64_t* out) {
    const TileWindow w = tile_window(tile, n, phase);
    out[0] = w.first_dword; out[1] = w.n_vecs;
}
uint32_t sp_lane_lds_dword(uint32_t lane, uint32_t phase) { return lane_lds_dword(lane, phase); }
uint64_t sp_prev_key_dword(uint64_t i) { return prev_key_dword(i); }
void sp_entry_from_words(uint32_t w0, uint32_t w1, uint32_t w2, uint64_t* kmer, uint32_t* count) {
    const Entry e = entry_from_words(w0, w1, w2);
    *kmer = e.kmer; *count = e.count;
}
int sp_breaks_order(uint64_t i, uint64_t prev_key, uint64_t key) { return breaks_order(i, prev_key, key); }
int sp_last_of_run(uint64_t i, uint64_t n, uint64_t key, uint64_t next_key) { return last_of_run(i, n, key, next_key); }

// The unpack launch over n packed entries (`entries`: n * 12 bytes at any alignment) laid `phase` dwords behind a 16-byte boundary,
// the way the kernel sees a device stream: margins of MARGIN_BYTES either side, filled with a pattern nothing may depend on.
// Every workgroup in turn, its lanes in turn on either side of what is the barrier on the device.  -> the order flag (0 / 1), or
// a negative number when a load left the stream and its margins, an LDS index left the array, or a vector was misaligned.
int sp_model_unpack(const uint8_t* entries, uint64_t n, uint32_t phase, uint64_t* kmers, uint32_t* counts) {
    if (phase > 3 || n >= MAX_ENTRIES) return -1;
    const uint64_t stream_bytes = n * ENTRY_BYTES;
    std::vector<uint32_t> mem((MARGIN_BYTES + 4 * phase + stream_bytes + MARGIN_BYTES + 3) / 4 + 4, 0xA5A5A5A5u);   // mem[0] stands on a 16-byte boundary
    const int64_t base = MARGIN_BYTES / 4 + phase;                      // dword index of the stream's base
    if (stream_bytes) memcpy(mem.data() + base, entries, stream_bytes);
    const int64_t lo = base - MARGIN_BYTES / 4, hi = base + (int64_t)(stream_bytes / 4) + MARGIN_BYTES / 4;   // what a device stream promises readable
    if (base_phase((uint64_t)base * 4) != phase) return -2;
    uint32_t flag = 0;
    std::vector<uint32_t> lds(LDS_DWORDS);
    for (uint32_t tile = 0; tile < n_tiles(n); tile++) {
        std::fill(lds.begin(), lds.end(), 0x5A5A5A5Au);                 // (what another tile left there must not matter)
        const TileWindow w = tile_window(tile, n, phase);
        if (w.n_vecs > TILE || w.n_vecs > TILE_VECS_MAX) return -3;     // one vector per lane at the most
        for (uint32_t lane = 0; lane < w.n_vecs; lane++) {
            const int64_t at = base + w.first_dword + 4 * (int64_t)lane;
            if (at & 3) return -4;                                      // 16-byte aligned
            if (at < lo || at + 4 > hi) return -5;
            for (int d = 0; d < 4; d++) lds[4 * lane + d] = mem[(size_t)(at + d)];
        }
        const uint32_t m = tile_entries(tile, n);
        for (uint32_t lane = 0; lane < m; lane++) {
            const uint32_t at = lane_lds_dword(lane, phase);
            if (at + 2 >= LDS_DWORDS || at + 2 >= 4 * w.n_vecs) return -6;
            const Entry e = entry_from_words(lds[at], lds[at + 1], lds[at + 2]);
            const uint64_t i = (uint64_t)tile * TILE + lane;
            kmers[i] = e.kmer;
            counts[i] = e.count;
            uint64_t prev = 0;
            if (lane) {
                prev = key_from_words(lds[at - ENTRY_DWORDS], lds[at - ENTRY_DWORDS + 1]);
            } else if (i) {
                const int64_t d = base + (int64_t)prev_key_dword(i);
                if (d < base || d + 2 > base + (int64_t)(stream_bytes / 4)) return -7;
                prev = key_from_words(mem[(size_t)d], mem[(size_t)d + 1]);
            }
            if (breaks_order(i, prev, e.kmer)) flag |= 1u;
        }
    }
    return (int)flag;
}

// The general road over unpacked arrays: a stable sort by key (what the device's radix sort over all 64 bits is), the keep flags,
// their exclusive sum, the compaction.  out_* have room for n entries; -> entries of the table.
uint64_t sp_model_table(const uint64_t* kmers, const uint32_t* counts, uint64_t n, uint64_t* out_kmers, uint32_t* out_counts) {
    std::vector<uint64_t> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return kmers[a] < kmers[b]; });
    std::vector<uint32_t> keep(n), pos(n);
    for (uint64_t i = 0; i < n; i++) keep[i] = last_of_run(i, n, kmers[order[i]], i + 1 < n ? kmers[order[i + 1]] : 0) ? 1u : 0u;
    uint32_t sum = 0;
    for (uint64_t i = 0; i < n; i++) { pos[i] = sum; sum += keep[i]; }
    for (uint64_t i = 0; i < n; i++)
        if (keep[i]) { out_kmers[pos[i]] = kmers[order[i]]; out_counts[pos[i]] = counts[order[i]]; }
    return n ? pos[n - 1] + keep[n - 1] : 0;
}

}  // extern "C"
