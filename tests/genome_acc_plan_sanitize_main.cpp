// A stand-alone program over sylph_amd/csrc/genome_acc_plan.h (through tests/genome_acc_plan_capi.cpp), to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_genome_acc_plan.py does both): the cut over crafted and pseudo-random
// length lists with every property checked again here, lengths and sums where 64-bit arithmetic could wrap, the capacity rule up to
// its ceiling and the bounds at their edges.  Exits 0 and prints a line; a violation or a sanitizer report fails.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
void gap_constants(uint64_t* out);
uint64_t gap_cut(const uint64_t* lens, uint64_t n_contigs, uint64_t from, uint64_t limit, uint64_t* runs, uint64_t max_runs, uint64_t* n_runs);
uint64_t gap_capacity_for(uint64_t cap, uint64_t need, uint64_t first);
int gap_contigs_fit(uint64_t have, uint64_t more);
int gap_seeds_fit(uint64_t have, uint64_t more);
int gap_push_fits(uint64_t n_bases, uint64_t bias);
}

// 0: the cut of `lens` under `limit` is whole, in order, below the limit, greedy, and stops at the first misfit
static int check_cut(const std::vector<uint64_t>& lens, uint64_t limit, uint64_t* total_runs) {
    const uint64_t n = lens.size();
    std::vector<uint64_t> runs(3 * (n + 1));
    uint64_t n_runs = 0;
    const uint64_t at = gap_cut(lens.data(), n, 0, limit, runs.data(), n + 1, &n_runs);
    uint64_t misfit = n;
    for (uint64_t i = 0; i < n; i++) if (lens[i] >= limit) { misfit = i; break; }
    if (at != misfit || n_runs > n) return 1;
    uint64_t next = 0;
    for (uint64_t r = 0; r < n_runs; r++) {
        const uint64_t first = runs[3 * r], cnt = runs[3 * r + 1], bases = runs[3 * r + 2];
        if (first != next || cnt == 0) return 2;
        uint64_t sum = 0;
        for (uint64_t i = first; i < first + cnt; i++) sum += lens[i];   // < limit per run: no wrap
        if (sum != bases || bases >= limit) return 3;
        next = first + cnt;
        if (next < misfit && lens[next] < limit - bases) return 4;        // the next contig would have fitted
    }
    if (next != misfit) return 5;
    *total_runs += n_runs;
    return 0;
}

int main() {
    uint64_t k[4];
    gap_constants(k);
    const uint64_t L = k[0];
    if (L != (1ull << 32) - 4096 || k[1] != (1ull << 32) - 1 || k[2] != (1ull << 32) - 2) return 2;
    uint64_t total_runs = 0;
    const std::vector<std::vector<uint64_t>> crafted = {
        {}, {0}, {1}, {L - 1}, {L}, {L - 1, 0, 1}, {L - 1, 1, 0}, {0, 0, 0}, {1, L - 2, 1}, {L - 2, 1, 1}, {5, L, 5}, {~0ull}, {1, ~0ull, 1},
        {L - 1, L - 1, L - 1, L - 1, L - 1, L - 1, L - 1, L - 1, L - 1},   // a sum beyond 2^35
        {1ull << 31, 1ull << 31, 1ull << 31, 1ull << 31, 1ull << 31},
    };
    for (const auto& lens : crafted)
        for (uint64_t limit : {L, (uint64_t)1, (uint64_t)2, (uint64_t)50000, (uint64_t)1 << 30})
            if (int rc = check_cut(lens, limit, &total_runs)) return 10 + rc;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (int round = 0; round < 400; round++) {
        std::vector<uint64_t> lens;
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        const uint64_t n = x % 60, limit = 1 + (x >> 20) % 5000;
        for (uint64_t i = 0; i < n; i++) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            lens.push_back((x >> 8) % 16 == 0 ? 0 : (x >> 12) % (limit + limit / 8 + 1));
        }
        if (int rc = check_cut(lens, limit, &total_runs)) return 20 + rc;
    }
    // the capacity rule: monotone, reaches need, ends at the ceiling
    const uint64_t needs[] = {0, 1, 63, 64, 65, 1ull << 20, (1ull << 20) + 1, (1ull << 31) + 1, k[2] - 1, k[2]};
    for (uint64_t first : {(uint64_t)1, (uint64_t)64, k[3]}) {
        uint64_t cap = 0, prev = 0;
        for (uint64_t need : needs) {
            cap = gap_capacity_for(cap, need, first);
            if (cap < need || cap < prev || cap > k[2]) return 30;
            prev = cap;
        }
        if (cap != k[2]) return 31;
    }
    if (!gap_seeds_fit(0, k[2]) || gap_seeds_fit(0, k[2] + 1) || gap_seeds_fit(1, k[2]) || gap_seeds_fit(~0ull, ~0ull)) return 40;
    if (!gap_contigs_fit(0, k[1]) || gap_contigs_fit(0, k[1] + 1) || gap_contigs_fit(k[1], 1) || gap_contigs_fit(~0ull, 1)) return 41;
    if (!gap_push_fits((1ull << 32) - 1, 0) || gap_push_fits(1ull << 32, 0) || gap_push_fits((1ull << 32) - 15, 15) || gap_push_fits(~0ull, 15)) return 42;
    printf("genome acc plan sanitize run ok: %llu runs checked\n", (unsigned long long)total_runs);
    return total_runs ? 0 : 50;
}
