// A stand-alone program over sylph_amd/csrc/sylsp_plan.h (through tests/sylsp_plan_capi.cpp), to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_sylsp_plan.py does both): it makes entry streams of its own (a fixed
// generator; 0, 1, 2, T - 1, T, T + 1 and 2 T + 1 entries; ascending, shuffled, shuffled with repeated keys one of which ends on a
// count of 0; the keys 0 and 2^64 - 1, the counts 0 and 2^32 - 1; a break at a tile boundary only), lays each at every dword phase
// and at every byte alignment of the source, replays the unpack launch and — where the order flag is set — the general road with
// the plan's functions, and compares with a std::map filled by insertion.  Exits 0 and prints a line; a mismatch or a sanitizer
// report fails.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

extern "C" {
int sp_model_unpack(const uint8_t* entries, uint64_t n, uint32_t phase, uint64_t* kmers, uint32_t* counts);
uint64_t sp_model_table(const uint64_t* kmers, const uint32_t* counts, uint64_t n, uint64_t* out_kmers, uint32_t* out_counts);
}

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return state;
}

int main() {
    const uint32_t T = 256;
    uint64_t cases = 0, n_ascending = 0, n_sorted = 0;
    for (uint64_t n : {0u, 1u, 2u, T - 1, T, T + 1, 2 * T + 1}) {
        for (int kind = 0; kind < 4; kind++) {          // 0 ascending, 1 shuffled, 2 shuffled with repeats, 3 ascending but for entry T
            std::vector<uint64_t> k(n);
            std::vector<uint32_t> c(n);
            uint64_t at = 0;
            for (uint64_t i = 0; i < n; i++) { at += 1 + (rnd64() >> 20); k[i] = at; c[i] = (uint32_t)(rnd64() % 1000) + 1; }
            if (n >= 2) { k[0] = 0; k[n - 1] = ~0ull; c[0] = 0; c[n - 1] = 0xFFFFFFFFu; }
            if (kind == 1 || kind == 2)
                for (uint64_t i = n; i > 1; i--) { const uint64_t j = rnd64() % i; std::swap(k[i - 1], k[j]); std::swap(c[i - 1], c[j]); }
            if (kind == 2 && n >= 2)
                for (uint64_t r = 0; r <= n / 100; r++) {
                    const uint64_t dst = rnd64() % n, src = (dst + 1 + rnd64() % (n - 1)) % n;
                    k[dst] = k[src];
                    if (r == 0) c[dst > src ? dst : src] = 0;
                }
            if (kind == 3) { if (n <= T) continue; k[T] = k[T - 1]; }
            std::map<uint64_t, uint32_t> want;
            for (uint64_t i = 0; i < n; i++) want[k[i]] = c[i];                 // insertion: a repeated key keeps its last value
            bool ascending = true;
            for (uint64_t i = 1; i < n; i++) ascending = ascending && k[i] > k[i - 1];
            for (uint32_t phase = 0; phase < 4; phase++) {
                const uint32_t shift = phase;                                   // the source bytes at every alignment, too
                std::vector<uint8_t> raw(n * 12 + shift);
                for (uint64_t i = 0; i < n; i++) { memcpy(&raw[shift + i * 12], &k[i], 8); memcpy(&raw[shift + i * 12 + 8], &c[i], 4); }
                std::vector<uint64_t> uk(n), tk(n);
                std::vector<uint32_t> uc(n), tc(n);
                const int flag = sp_model_unpack(raw.data() + shift, n, phase, uk.data(), uc.data());
                if (flag < 0) { fprintf(stderr, "model_unpack %d at n %llu phase %u\n", flag, (unsigned long long)n, phase); return 2; }
                if ((flag != 0) == ascending) return 3;
                if (uk != k || uc != c) return 4;
                uint64_t m = n;
                if (flag) m = sp_model_table(uk.data(), uc.data(), n, tk.data(), tc.data());
                else { tk = uk; tc = uc; }
                if (m != want.size()) return 5;
                uint64_t j = 0;
                for (const auto& kv : want) {                                   // a map walks in ascending key order
                    if (tk[j] != kv.first || tc[j] != kv.second) return 6;
                    j++;
                }
                cases++;
                (flag ? n_sorted : n_ascending)++;
            }
        }
    }
    printf("sylsp plan sanitize run ok: %llu cases, %llu ascending, %llu sorted\n", (unsigned long long)cases, (unsigned long long)n_ascending,
           (unsigned long long)n_sorted);
    return 0;
}
