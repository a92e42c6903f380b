// A stand-alone program over sylph_amd/csrc/bootstrap_plan.h and the host's split statistics (sylph_amd/host/inference.cpp: stats_head,
// bootstrap_host, finish_ci), to be built with -fsanitize=address,undefined and run on the CPU (tests/test_bootstrap_plan.py does both):
// the corners where an index could leave its array — one-value genomes, nothing kept, a mode in the last bin, outliers beyond the
// Poisson cap, values no histogram is sized for, rejected draws.  Exits 0 and prints a line; a sanitizer report fails the run.
#include <cstdio>
#include <random>

#include "../sylph_amd/host/sylph_host.hpp"

using namespace sylph_host;

int main() {
    std::mt19937_64 rng(1);
    ContainArgs args;
    args.minimum_ani = 0.;
    double acc = 0;
    int with_ci = 0;
    for (int trial = 0; trial < 120; trial++) {
        const size_t n_kmers = 50 + rng() % 4000;
        std::poisson_distribution<uint32_t> pois(trial % 4 == 0 ? 0.05 : trial % 4 == 1 ? 0.4 : trial % 4 == 2 ? 1.2 : 6.0);
        std::vector<uint32_t> covs;
        for (size_t i = 0; i < n_kmers; i++) { const uint32_t c = pois(rng); if (c && rng() % 10 < 8) covs.push_back(c); }
        if (trial % 7 == 0 && covs.size() > 3) covs[0] = covs[1] = covs[2] = 100000;                 // beyond the cap
        if (trial % 11 == 0 && !covs.empty()) covs.back() = 3000000;                               // no histogram is sized for it
        if (trial == 5) covs.assign(1, 1);
        if (trial == 6) covs.clear();
        const auto whole = stats_from_covs(args, covs, n_kmers, 31, std::nullopt);
        std::vector<uint32_t> sorted = covs;
        StatsHead h = stats_head(args, sorted, n_kmers, 31, std::nullopt);
        if (h.result && h.want_ci) bootstrap_host(sorted.data(), h.keep, h.n_total, 31., args, *h.result);
        if ((bool)whole != (bool)h.result) return 2;
        if (whole) {
            if (whole->ani_ci_lo != h.result->ani_ci_lo || whole->lambda_ci_hi != h.result->lambda_ci_hi) return 3;
            acc += whole->final_est_ani + whole->ani_ci_lo.value_or(0.);
            with_ci += whole->ani_ci_lo ? 1 : 0;
        }
    }
    {   // resampling corners: nothing kept, everything kept, one value
        AniResult r;
        const uint32_t kept[3] = {1, 2, 2};
        bootstrap_host(kept, 0, 1, 31., args, r);
        bootstrap_host(kept, 0, 40, 31., args, r);
        bootstrap_host(kept, 3, 3, 31., args, r);
        bootstrap_host(kept, 1, 1, 31., args, r);
    }
    {   // the plan on its own: draws around the 96- / 128-bit seam and where half of them are rejected; a mode in the last bin
        uint64_t sum = 0, rejected = 0;
        for (uint64_t n : {1ull, 2ull, 0xFFFFFFFFull, 0x100000000ull, (1ull << 63) + 1, ~0ull})
            for (uint64_t j = 0; j < 2000; j++) { bool rej = false; const uint64_t idx = bootstrap_plan::bootstrap_draw(7, j, n, &rej); if (idx >= n) return 4; sum += idx; rejected += rej; }
        if (!rejected) return 5;
        uint32_t hist[bootstrap_plan::BINS] = {};
        hist[bootstrap_plan::BINS - 1] = 9; hist[1] = 9;
        const auto s = bootstrap_plan::summary_of_histogram(hist, bootstrap_plan::BINS);
        if (s.mode != bootstrap_plan::BINS - 1 || s.next_count != 0 || s.n_distinct != 2) return 6;
        acc += (double)(sum % 1000);
    }
    printf("bootstrap sanitize run ok: %d intervals, checksum %.6f\n", with_ci, acc);
    return with_ci > 20 ? 0 : 7;
}
