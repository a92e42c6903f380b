// A stand-alone program over sylph_amd/csrc/index_plan.h (through tests/index_plan_capi.cpp), to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_index_plan.py does both, for 8 and for 4 slots per line): it reads a
// posting set and a list of k-mers from a file the test wrote, builds the model index with the plan's bucket writer, looks every
// k-mer up with the plan's slot scan and compares the genomes with a std::map's.  File: u64 {n, n_genomes, lambda, pass_max, n_queries},
// n k-mers, n genome ids (u64 each), n_queries k-mers.  Exits 0 and prints a line; a mismatch or a sanitizer report fails the run.
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

extern "C" {
void* ip_model_build(const uint64_t* keys, const uint32_t* gids, uint64_t n, uint64_t n_genomes, uint64_t kmer_lo, uint64_t kmer_hi,
                     uint64_t lambda, uint64_t pass_max);
void ip_model_free(void* m);
uint64_t ip_model_lookup(const void* m, uint64_t km, uint32_t* out, uint64_t cap, int* long_run);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[5];
    if (fread(h, 8, 5, f) != 5) return 2;
    const uint64_t n = h[0], nq = h[4];
    std::vector<uint64_t> keys(n), g64(n), queries(nq);
    if (fread(keys.data(), 8, n, f) != n || fread(g64.data(), 8, n, f) != n || fread(queries.data(), 8, nq, f) != nq) return 2;
    fclose(f);
    std::vector<uint32_t> gids(g64.begin(), g64.end());
    std::map<uint64_t, std::vector<uint32_t>> want;
    for (uint64_t i = 0; i < n; i++) want[keys[i]].push_back(gids[i]);
    void* m = ip_model_build(keys.data(), gids.data(), n, h[1], 0, 0, h[2], h[3]);
    if (!m) return 3;
    uint64_t found = 0, long_runs = 0;
    std::vector<uint32_t> got(n + 1);
    for (uint64_t km : queries) {
        int long_run = 0;
        const uint64_t c = ip_model_lookup(m, km, got.data(), got.size(), &long_run);
        const auto it = want.find(km);
        const size_t e = it == want.end() ? 0 : it->second.size();
        if (c != e) return 4;
        for (size_t j = 0; j < e; j++) if (got[j] != it->second[j]) return 5;
        found += c;
        long_runs += (uint64_t)long_run;
    }
    ip_model_free(m);
    printf("index sanitize run ok: %llu k-mers, %llu genomes found, %llu long runs\n", (unsigned long long)nq, (unsigned long long)found,
           (unsigned long long)long_runs);
    return 0;
}
