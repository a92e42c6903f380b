// A stand-alone program over sylph_amd/csrc/table_summary_plan.h (through tests/table_summary_plan_capi.cpp), to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_table_summary_plan.py does both): tables of its own making at every
// length around the chunk, tile and group boundaries, each allocated at exactly its size so that a load behind the table is a
// report, as are an index behind the chunk records or a wrapped shift; shallow and deep depths, ones, zeros, outliers up to
// 2^32 - 1, the never-closing alternation.  The model of the device's passes must equal the plain walk or decline.  Exits 0 and
// prints a line; a mismatch or a sanitizer report fails.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../sylph_amd/csrc/table_summary_plan.h"

using sylph::table_summary_plan::Summary;
namespace tsp = sylph::table_summary_plan;

extern "C" {
void ts_walk(const uint32_t* counts, uint64_t n, Summary* out);
int ts_model(const uint32_t* counts, uint64_t n, const uint32_t* caps, const uint32_t* chunks, uint32_t n_rungs, uint32_t max_open, Summary* out);
}

int main() {
    std::mt19937_64 rng(5);
    const uint32_t ladders[][2][3] = {{{4, 16, 0}, {8, 8, 0}}, {{2, 0, 0}, {1, 0, 0}}, {{8, 64, 4096}, {33, 65, 31}}, {{64, 1024, 16384}, {4096, 16384, 262144}}};
    const uint32_t n_rungs[] = {2, 1, 3, 3};
    const uint64_t lens[] = {0, 1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 70000};
    unsigned long long tables = 0, n_declined = 0, n_later = 0, n_open = 0;
    for (uint64_t len : lens) {
        for (int kind = 0; kind < 10; kind++) {
            std::poisson_distribution<uint32_t> pois(kind % 5 == 0 ? 0.4 : kind % 5 == 1 ? 2.5 : kind % 5 == 2 ? 9.0 : kind % 5 == 3 ? 40.0 : 500.0);
            std::vector<uint32_t> v(len);
            for (auto& x : v) x = pois(rng);
            if (kind == 5) for (uint64_t i = 0; i < len; i++) v[i] = i % 2 ? 1000000u : 2u;
            if (kind == 6 && len > 2) v[0] = v[len - 1] = 1u << 31, v[len / 2] = 0xFFFFFFFFu;
            if (kind == 7) for (uint64_t i = len / 3; i < 2 * len / 3; i++) v[i] = 1;
            v.shrink_to_fit();
            Summary want;
            ts_walk(v.data(), len, &want);
            for (int l = 0; l < 4; l++) {
                if (len > 4097 && l == 1) continue;                   // (chunks of one entry: only the short tables)
                Summary got;
                if (ts_model(v.data(), len, ladders[l][0], ladders[l][1], n_rungs[l], 64, &got)) return 2;
                tables++;
                if (got.total_counts != want.total_counts || got.steps != want.steps || got.num_1s != want.num_1s || got.num_not1s != want.num_not1s) {
                    fprintf(stderr, "sums differ at len %llu kind %d ladder %d\n", (unsigned long long)len, kind, l);
                    return 3;
                }
                if (got.flags & tsp::DECLINED) { n_declined++; continue; }
                if (got.median_sum != want.median_sum || got.max_state != want.max_state || got.flags != 0) {
                    fprintf(stderr, "walk differs at len %llu kind %d ladder %d\n", (unsigned long long)len, kind, l);
                    return 4;
                }
                n_later += got.rung > 0;
                n_open += got.open_chunks;
            }
        }
    }
    printf("table summary sanitize run ok: %llu tables, %llu declined, %llu later-rung, %llu open chunks\n", tables, n_declined, n_later, n_open);
    return n_declined && n_later && n_open ? 0 : 7;
}
