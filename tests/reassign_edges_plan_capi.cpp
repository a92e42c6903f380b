// C entry points over sylph_amd/csrc/reassign_edges_plan.h for tests/test_reassign_edges_plan.py (ctypes) and
// tests/reassign_edges_sanitize_main.cpp: the plan's functions one by one, and ep_model_count — the count launch of
// reassign_edges.hip replayed on the host, work item by work item and lane by lane, with the very functions the kernel calls.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../sylph_amd/csrc/reassign_edges_plan.h"

using namespace sylph::edge_plan;

extern "C" {

void ep_constants(uint64_t* out) { out[0] = NO_WINNER; out[1] = COUNT_TPB; out[2] = COUNT_WAVES; out[3] = WINDOW_MAX; out[4] = WINDOW_DEFAULT; out[5] = sizeof(Edge); out[6] = FIRST_EDGES_MIN; out[7] = FIRST_EDGES_PER_RANK; }
uint32_t ep_n_windows(uint32_t n_passing, uint32_t window) { return n_windows(n_passing, window); }
uint32_t ep_work_losers(const uint64_t* kmer_off, uint32_t n_passing, uint32_t* out) { return work_losers(kmer_off, n_passing, out); }
uint64_t ep_n_work_items(uint32_t n_losers, uint32_t n_passing, uint32_t window) { return n_work_items(n_losers, n_passing, window); }
void ep_work_item(uint32_t b, uint32_t n_passing, uint32_t window, uint32_t* out) {
    const WorkItem it = work_item(b, n_passing, window);
    out[0] = it.loser_slot; out[1] = it.window_base; out[2] = it.window_len;
}
int ep_counts_in_window(uint32_t winner, uint32_t loser, uint32_t base, uint32_t len) { return counts_in_window(winner, loser, base, len); }
int ep_reported(uint32_t count, uint32_t min_count) { return reported(count, min_count); }
uint64_t ep_edge_bound(const uint64_t* kmer_off, uint32_t n_passing, uint32_t min_count) { return edge_bound(kmer_off, n_passing, min_count); }
uint64_t ep_first_capacity(uint64_t bound, uint32_t n_passing) { return first_capacity(bound, n_passing); }
uint64_t ep_retry_capacity(uint64_t cursor, uint64_t capacity) { return retry_capacity(cursor, capacity); }
uint64_t ep_sort_and_merge(Edge* e, uint64_t n) { return sort_and_merge(e, n); }

// The count launch over a winner array: every work item in turn (any order would do: one reservation each), its lanes in turn
// between what are barriers on the device.  edges has room for cap entries; -> the cursor (edges wanted).
uint64_t ep_model_count(const uint32_t* winner, const uint64_t* kmer_off, uint32_t n_passing, uint32_t window, uint32_t min_count, Edge* edges,
                        uint64_t cap) {
    std::vector<uint32_t> losers(n_passing ? n_passing : 1);
    const uint32_t n_losers = work_losers(kmer_off, n_passing, losers.data());
    const uint64_t n_items = n_work_items(n_losers, n_passing, window);
    uint64_t cursor = 0;
    std::vector<uint32_t> cnt(WINDOW_MAX);
    for (uint64_t b = 0; b < n_items; b++) {
        const WorkItem it = work_item((uint32_t)b, n_passing, window);
        const uint32_t loser = losers[it.loser_slot];
        for (uint32_t t = 0; t < it.window_len; t++) cnt[t] = 0;
        for (uint64_t i = kmer_off[loser]; i < kmer_off[loser + 1]; i++)
            if (counts_in_window(winner[i], loser, it.window_base, it.window_len)) cnt[winner[i] - it.window_base]++;
        uint32_t total = 0;
        for (uint32_t t = 0; t < it.window_len; t++) total += reported(cnt[t], min_count);
        if (!total) continue;
        const uint64_t reservation = cursor;
        cursor += total;
        uint32_t before = 0;
        for (uint32_t t0 = 0; t0 < it.window_len; t0 += COUNT_TPB) {
            uint64_t ballot[COUNT_WAVES];
            uint32_t wt[COUNT_WAVES];
            for (uint32_t w = 0; w < COUNT_WAVES; w++) {
                ballot[w] = 0;
                for (uint32_t lane = 0; lane < 64; lane++) {
                    const uint32_t t = t0 + w * 64 + lane;
                    if (t < it.window_len && reported(cnt[t], min_count)) ballot[w] |= 1ull << lane;
                }
                wt[w] = (uint32_t)__builtin_popcountll(ballot[w]);
            }
            for (uint32_t tid = 0; tid < COUNT_TPB; tid++) {
                const uint32_t t = t0 + tid, w = tid >> 6, lane = tid & 63;
                if (!((ballot[w] >> lane) & 1)) continue;
                const uint64_t slot = reservation + before + slot_in_tile(wt, w, below_lane(ballot[w], lane));
                if (slot < cap) edges[slot] = Edge{it.window_base + t, loser, cnt[t]};
            }
            before += tile_total(wt);
        }
    }
    return cursor;
}

}  // extern "C"
