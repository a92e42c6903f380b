// A stand-alone program over sylph_amd/csrc/reassign_edges_plan.h (through tests/reassign_edges_plan_capi.cpp), to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_reassign_edges_plan.py does both): it makes winner arrays of its own
// (a fixed generator; passing lists of 1 .. 3 windows + 5 with empty losers in between, winners at the window edges, NO_WINNER,
// self-winners), replays the count launch with the plan's functions into an edge list that is too small at first (the retry
// sizing), sorts and merges, and compares with a std::map.  Exits 0 and prints a line; a mismatch or a sanitizer report fails.
#include <cstdint>
#include <cstdio>
#include <map>
#include <utility>
#include <vector>

struct Edge { uint32_t winner, loser, count; };
extern "C" {
uint64_t ep_model_count(const uint32_t* winner, const uint64_t* kmer_off, uint32_t n_passing, uint32_t window, uint32_t min_count, Edge* edges, uint64_t cap);
uint64_t ep_retry_capacity(uint64_t cursor, uint64_t capacity);
uint64_t ep_edge_bound(const uint64_t* kmer_off, uint32_t n_passing, uint32_t min_count);
uint64_t ep_sort_and_merge(Edge* e, uint64_t n);
}

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((state >> 33) % n);
}

int main() {
    uint64_t cases = 0, edges_seen = 0, retries = 0;
    for (uint32_t window : {1u, 7u, 64u, 256u, 257u}) {
        for (uint32_t n_passing : {0u, 1u, window - 1, window, window + 1, 3 * window + 5}) {
            for (uint32_t min_count : {0u, 1u, 3u}) {
                std::vector<uint64_t> off(n_passing + 1, 0);
                for (uint32_t r = 0; r < n_passing; r++) off[r + 1] = off[r] + (r % 3 == 1 ? 0 : rnd(40));   // every third loser is empty
                std::vector<uint32_t> winner(off[n_passing]);
                std::map<std::pair<uint32_t, uint32_t>, uint32_t> want;                                     // (loser, winner) -> count
                for (uint32_t r = 0; r < n_passing; r++)
                    for (uint64_t i = off[r]; i < off[r + 1]; i++) {
                        const uint32_t pick = rnd(8);
                        uint32_t w = pick == 0 ? 0xFFFFFFFFu : pick == 1 ? r : pick == 2 ? (r / window) * window : pick == 3 ? n_passing - 1 : rnd(n_passing < 6 ? n_passing : 6);
                        winner[i] = w;
                        if (w != 0xFFFFFFFFu && w != r) want[{r, w}]++;
                    }
                const uint32_t mc = min_count ? min_count : 1;
                for (auto it = want.begin(); it != want.end();) it = it->second < mc ? want.erase(it) : ++it;
                uint64_t cap = want.size() / 2;                                                              // too small unless there is nothing
                std::vector<Edge> edges(cap);
                uint64_t cursor = ep_model_count(winner.data(), off.data(), n_passing, window, min_count, edges.data(), cap);
                if (const uint64_t again = ep_retry_capacity(cursor, cap)) {
                    retries++;
                    cap = again;
                    edges.assign(cap, Edge{0, 0, 0});
                    cursor = ep_model_count(winner.data(), off.data(), n_passing, window, min_count, edges.data(), cap);
                    if (ep_retry_capacity(cursor, cap)) return 3;
                }
                if (cursor != want.size() || cursor > ep_edge_bound(off.data(), n_passing, min_count)) return 4;
                if (ep_sort_and_merge(edges.data(), cursor) != cursor) return 5;
                uint64_t j = 0;
                for (const auto& kv : want) {                                                                // a map walks in (loser, winner) order
                    if (edges[j].loser != kv.first.first || edges[j].winner != kv.first.second || edges[j].count != kv.second) return 6;
                    j++;
                }
                cases++;
                edges_seen += cursor;
            }
        }
    }
    printf("reassign edges sanitize run ok: %llu cases, %llu edges, %llu retries\n", (unsigned long long)cases, (unsigned long long)edges_seen,
           (unsigned long long)retries);
    return 0;
}
