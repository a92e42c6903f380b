// A stand-alone program over sylph_amd/csrc/hits_plan.h (through tests/hits_plan_capi.cpp), to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_hits_plan.py does both): every walk of the hit finish's driver from every
// start under every sequence of answers, the stretches of the hit list at the sizes where their arithmetic could wrap, the row
// counters' bijection, the geometry at its limits and the two row lists filled to the brim.  Exits 0 and prints a line; a violation or
// a sanitizer report fails.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
void hp_walk_all(uint64_t* out);
uint32_t hp_stretch_check(uint32_t n, uint32_t grid);
int hp_rc_bijection(uint32_t R2);
uint64_t hp_rc_shared_lines(uint32_t R2, uint32_t first, uint32_t count);
void hp_geometry(uint64_t n_rows, uint64_t cap, uint64_t n_guess, uint64_t* out);
uint64_t hp_place_rows(const uint32_t* counts, uint64_t n_rows, uint64_t cap, uint32_t* out);
}

int main() {
    uint64_t w[14];
    hp_walk_all(w);
    if (w[0] == 0 || w[1] != 0) return 3;                        // a walk that does not end, a step out of place, a flag that claims too much
    if (w[2] == 0 || w[4] != 2 || w[5] != 2) return 4;           // some walks fail; at most two probes and two assemblies
    const uint32_t sizes[] = {0u, 1u, 255u, 256u, 257u, 6143u, 6144u, (1u << 20) + 1u, 0xFFFFFFFFu}, grids[] = {16u, 17u, 64u, 768u};
    for (uint32_t n : sizes)
        for (uint32_t g : grids)
            if (hp_stretch_check(n, g) != 0) return 5;
    for (uint32_t R2 = 1024; R2 <= (1u << 16); R2 <<= 1)
        if (!hp_rc_bijection(R2) || hp_rc_shared_lines(R2, 0, R2 - 16) != 0) return 6;
    uint64_t g[12];
    const uint64_t rows[] = {0, 1, 2047, 2048, 2049, 524352, (1ull << 31) - 1, 1ull << 31}, caps[] = {1, 1ull << 20, (1ull << 32) - 1};
    for (uint64_t r : rows)
        for (uint64_t c : caps) {
            hp_geometry(r, c, c / 2, g);
            if (g[0] != (r != 0 && r < (1ull << 31))) return 7;
            if (g[0] && (g[2] < r || g[8] < (g[11] + 2 + g[5]) * 4 || g[6] < 16 || g[6] > 768)) return 7;
        }
    // the two lists meet exactly: 3072 small rows and 1024 long ones fill the 4096 entries of 4096 rows
    std::vector<uint32_t> counts(4096);
    uint64_t cap = 0;
    for (uint32_t r = 0; r < 4096; r++) { counts[r] = r % 4 == 3 ? 65 : 1; cap += counts[r]; }
    uint32_t len[2] = {0, 0};
    if (hp_place_rows(counts.data(), counts.size(), cap, len) != 0 || len[0] + len[1] != 4096) return 8;
    printf("hits plan sanitize run ok: %llu walks (%llu failed), longest %llu steps, at most %llu probes and %llu assemblies\n",
           (unsigned long long)w[0], (unsigned long long)w[2], (unsigned long long)w[3], (unsigned long long)w[4], (unsigned long long)w[5]);
    return 0;
}
