// A stand-alone program over sylph_amd/csrc/row_stats_plan.h (through tests/row_stats_plan_capi.cpp) and the host's split statistics
// (sylph_amd/host/inference.cpp: row_cut_table, stats_head, stats_head_from_summary), to be built with -fsanitize=address,undefined and
// run on the CPU (tests/test_row_stats_plan.py does both): rows of its own making at every length around the chunk boundaries — one
// value, a full chunk, one more, thousands —, at the three widths, each allocated at exactly its size so that a load behind the row
// is a report; outliers the cut drops, values at the width boundaries, sums that wrap, the largest value there is.  The replay of
// the kernel's split must equal the sequential summary, and the statistics from the summary those from the row.  Exits 0 and
// prints a line; a mismatch or a sanitizer report fails.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>

#include "../sylph_amd/host/sylph_host.hpp"

extern "C" {
int rs_summarise(const void* row, uint32_t width, uint32_t len, const uint32_t* cut, uint32_t* out);
int rs_replay(const void* row, uint32_t width, uint32_t len, const uint32_t* cut, uint32_t* out);
int rs_surely_rejected(const uint32_t* summary, uint32_t contain_count, uint64_t n_genome_kmers, const void* filter);
}

using namespace sylph_host;

int main() {
    std::mt19937_64 rng(3);
    const uint32_t* cut = row_cut_table();
    ContainArgs args;
    args.no_ci = true;
    const sylph_row_filter filter = row_filter_for(args, 31);
    unsigned long long rows = 0, n_cut = 0, n_long = 0, n_passed = 0, n_dropped = 0;
    const uint32_t lens[] = {1, 2, 3, 24, 25, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1000, 5000};
    for (uint32_t len : lens) {
        for (int kind = 0; kind < 12; kind++) {
            std::poisson_distribution<uint32_t> pois(kind % 4 == 0 ? 0.1 : kind % 4 == 1 ? 1.0 : kind % 4 == 2 ? 2.2 : 20.0);
            std::vector<uint32_t> v(len);
            for (auto& x : v) x = pois(rng) + 1;
            if (kind == 4) std::fill(v.begin(), v.end(), 2u);                                   // one run over every chunk
            if (kind == 5 && len > 2) v[0] = v[1] = v[2] = 1u << 31;                            // the sum wraps (or the cut drops them)
            if (kind == 6) v[len - 1] = 0xFFFFFFFFu;
            if (kind == 7) v[len / 3] = 255, v[len / 2] = 256;
            if (kind == 8) v[len / 3] = 65535, v[len / 2] = 65536;
            std::sort(v.begin(), v.end());
            const uint32_t top = v.back(), width = top < 256 ? 1 : top < 65536 ? 2 : 4;
            std::vector<uint8_t> narrow8;
            std::vector<uint16_t> narrow16;
            const void* p = v.data();
            if (width == 1) { narrow8.assign(v.begin(), v.end()); p = narrow8.data(); }
            if (width == 2) { narrow16.assign(v.begin(), v.end()); p = narrow16.data(); }
            uint32_t a[9], b[9], c[9];
            if (rs_summarise(p, width, len, cut, a) || rs_replay(p, width, len, cut, b) || rs_summarise(v.data(), 4, len, cut, c)) return 2;
            if (memcmp(a, b, sizeof(a)) || memcmp(a, c, sizeof(a))) { fprintf(stderr, "replay differs at len %u kind %d\n", len, kind); return 3; }
            row_stats_plan::RowSummary s;
            memcpy(&s, a, sizeof(s));
            const size_t n_kmers = (size_t)len * (kind % 3 == 0 ? 1 : kind % 3 == 1 ? 3 : 200);      // ANI 1, 0.965, 0.84
            std::vector<uint32_t> copy = v;
            const StatsHead h1 = stats_head(args, copy, n_kmers, 31, std::nullopt), h2 = stats_head_from_summary(args, s, n_kmers, 31, std::nullopt);
            if ((bool)h1.result != (bool)h2.result || h1.keep != h2.keep || h1.rejected_ani != h2.rejected_ani) return 4;
            if (h1.result && (h1.result->final_est_ani != h2.result->final_est_ani || h1.result->final_est_cov != h2.result->final_est_cov)) return 5;
            const int dropped = rs_surely_rejected(a, len, n_kmers, &filter);
            if (dropped && h1.result) return 6;                                                 // soundness
            rows++;
            n_cut += s.keep < len;
            n_long += len > 128;
            n_passed += (bool)h1.result;
            n_dropped += dropped;
        }
    }
    printf("row stats sanitize run ok: %llu rows, %llu cut, %llu long, %llu passed, %llu dropped\n", rows, n_cut, n_long, n_passed, n_dropped);
    return n_passed && n_dropped ? 0 : 7;
}
