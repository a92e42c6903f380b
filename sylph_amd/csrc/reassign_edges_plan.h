// reassign_edges_plan.h — the arithmetic of the reassignment log (sylph_db_reassign_edges, reassign_edges.hip), free of HIP: the work
// list of the count launch, which entries of the winner array a workgroup counts, which counts are reported, where a reported entry
// lands in the workgroup's reservation, how large the edge list is made and remade, and the order the library returns the edges in.
// reassign_edges.hip (kernels and host entry) includes this header; tests/test_reassign_edges_plan.py compiles it with g++
// (tests/reassign_edges_plan_capi.cpp) and checks it against numpy, a lane-by-lane model of the count kernel included.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SY_EDGE_HD __host__ __device__ __forceinline__
#else
#define SY_EDGE_HD inline
#endif

namespace sylph {
namespace edge_plan {

// One edge: `count` k-mer occurrences of the genome of rank `loser` belong to the genome of rank `winner` (ranks in the passing
// list).  Laid out as sylph_reassign_edge of the ABI.
struct Edge { uint32_t winner, loser, count; };

constexpr uint32_t NO_WINNER = 0xFFFFFFFFu;   // winner array: no passing genome holds the k-mer
constexpr uint32_t COUNT_TPB = 256;           // lanes of a count workgroup = entries of one compaction tile
constexpr uint32_t COUNT_WAVES = COUNT_TPB / 64;
// Winner ranks one count workgroup keeps counters for, 4 bytes of LDS each.  8192 (32 KB: several workgroups per CU, and a real
// profile's few thousand passing genomes are one window) is a guess nobody has measured; the context option
// "reassign_edge_window" lowers it (the tests do, to get several windows at small shapes).
constexpr uint32_t WINDOW_MAX = 8192;
constexpr uint32_t WINDOW_DEFAULT = WINDOW_MAX;

// ---- work list of the count launch -----------------------------------------------------------------------------------------
// One workgroup per (loser, window of winner ranks); a loser without k-mers has no item.  `losers` = the ranks with a non-empty
// k-mer list, ascending; item b is loser slot b / n_windows, window b % n_windows.
SY_EDGE_HD uint32_t n_windows(uint32_t n_passing, uint32_t window) { return n_passing ? (n_passing - 1) / window + 1 : 0; }
// -> number of losers written to out (room for n_passing)
inline uint32_t work_losers(const uint64_t* kmer_off, uint32_t n_passing, uint32_t* out) {
    uint32_t n = 0;
    for (uint32_t r = 0; r < n_passing; r++)
        if (kmer_off[r + 1] > kmer_off[r]) out[n++] = r;
    return n;
}
SY_EDGE_HD uint64_t n_work_items(uint32_t n_losers, uint32_t n_passing, uint32_t window) { return (uint64_t)n_losers * n_windows(n_passing, window); }
struct WorkItem { uint32_t loser_slot, window_base, window_len; };
SY_EDGE_HD WorkItem work_item(uint32_t b, uint32_t n_passing, uint32_t window) {
    const uint32_t nw = n_windows(n_passing, window);
    WorkItem it;
    it.loser_slot = b / nw;
    it.window_base = (b % nw) * window;
    it.window_len = n_passing - it.window_base < window ? n_passing - it.window_base : window;
    return it;
}

// ---- what a workgroup counts, what it reports ------------------------------------------------------------------------------
// a winner array entry counts for the item's window when its rank lies in the window and is not the loser's own (NO_WINNER lies
// beyond every window: window_base + window_len <= n_passing < 2^32 - 1)
SY_EDGE_HD bool counts_in_window(uint32_t winner, uint32_t loser, uint32_t window_base, uint32_t window_len) {
    return winner - window_base < window_len && winner >= window_base && winner != loser;
}
SY_EDGE_HD uint32_t effective_min_count(uint32_t min_count) { return min_count ? min_count : 1u; }
SY_EDGE_HD bool reported(uint32_t count, uint32_t min_count) { return count >= effective_min_count(min_count); }

// ---- compaction order ------------------------------------------------------------------------------------------------------
// A workgroup's reported entries take consecutive slots from its reservation in ascending winner order.  The window is scanned
// in tiles of COUNT_TPB entries, one per lane: a reported entry's slot = reservation + reported entries of earlier tiles + of
// earlier wavefronts of its tile (wave_totals) + of lower lanes of its wavefront (the wavefront's ballot).
SY_EDGE_HD uint32_t below_lane(uint64_t ballot, uint32_t lane) {
    return (uint32_t)__builtin_popcountll(ballot & ((1ull << lane) - 1ull));
}
SY_EDGE_HD uint32_t slot_in_tile(const uint32_t (&wave_totals)[COUNT_WAVES], uint32_t wave, uint32_t below_in_wave) {
    uint32_t s = below_in_wave;
    for (uint32_t w = 0; w < COUNT_WAVES; w++) s += w < wave ? wave_totals[w] : 0u;
    return s;
}
SY_EDGE_HD uint32_t tile_total(const uint32_t (&wave_totals)[COUNT_WAVES]) {
    uint32_t s = 0;
    for (uint32_t w = 0; w < COUNT_WAVES; w++) s += wave_totals[w];
    return s;
}

// ---- capacity of the edge list ---------------------------------------------------------------------------------------------
// A loser of n k-mers has at most min(n_passing - 1, n / min_count) reported edges; their sum bounds the list.  The first launch
// gets the bound or, where that is large, room for FIRST_EDGES_PER_RANK edges per passing genome (no n_passing^2 memory); a launch
// that needed more says how many (its cursor), and the one retry gets exactly that — which the bound still bounds.
constexpr uint64_t FIRST_EDGES_MIN = 1u << 16, FIRST_EDGES_PER_RANK = 16;
inline uint64_t edge_bound(const uint64_t* kmer_off, uint32_t n_passing, uint32_t min_count) {
    const uint64_t mc = effective_min_count(min_count);
    uint64_t s = 0;
    for (uint32_t r = 0; r < n_passing; r++) s += std::min<uint64_t>(n_passing - 1, (kmer_off[r + 1] - kmer_off[r]) / mc);
    return s;
}
inline uint64_t first_capacity(uint64_t bound, uint32_t n_passing) {
    return std::min<uint64_t>(bound, std::max<uint64_t>(FIRST_EDGES_MIN, FIRST_EDGES_PER_RANK * n_passing));
}
// cursor = edges the launch wanted to write; -> 0: they all fitted, else the capacity of the retry
inline uint64_t retry_capacity(uint64_t cursor, uint64_t capacity) { return cursor > capacity ? cursor : 0; }

// ---- the order edges are returned in ---------------------------------------------------------------------------------------
SY_EDGE_HD bool edge_less(const Edge& a, const Edge& b) { return a.loser != b.loser ? a.loser < b.loser : a.winner < b.winner; }
// sorts n edges by (loser, winner) and adds up the counts of entries with the same pair; -> entries left
inline size_t sort_and_merge(Edge* e, size_t n) {
    std::sort(e, e + n, [](const Edge& a, const Edge& b) { return edge_less(a, b); });
    size_t m = 0;
    for (size_t i = 0; i < n; i++) {
        if (m && e[m - 1].loser == e[i].loser && e[m - 1].winner == e[i].winner) e[m - 1].count += e[i].count;
        else e[m++] = e[i];
    }
    return m;
}

}  // namespace edge_plan
}  // namespace sylph
