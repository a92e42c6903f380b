// C wrapper over sylph_amd/csrc/genome_acc_plan.h for tests/test_genome_acc_plan.py (g++, no HIP).
#include "../sylph_amd/csrc/genome_acc_plan.h"

using namespace sylph::genome_acc_plan;

extern "C" {

void gap_constants(uint64_t* out) {
    out[0] = PUSH_LIMIT;
    out[1] = MAX_CONTIGS;
    out[2] = MAX_SEEDS;
    out[3] = FIRST_CAPACITY;
}

// the run that begins at `from`: out = first, n, bases
void gap_next_run(const uint64_t* lens, uint64_t n_contigs, uint64_t from, uint64_t limit, uint64_t* out) {
    const Run r = next_run(lens, n_contigs, from, limit);
    out[0] = r.first;
    out[1] = r.n;
    out[2] = r.bases;
}

// the runs from `from` up to the first misfit: runs[3 i ..] = first, n, bases for up to max_runs runs; *n_runs counts them all.
// Returns the misfit's index (n_contigs: none).
uint64_t gap_cut(const uint64_t* lens, uint64_t n_contigs, uint64_t from, uint64_t limit, uint64_t* runs, uint64_t max_runs, uint64_t* n_runs) {
    uint64_t n = 0;
    const uint64_t at = cut(lens, n_contigs, from, limit, [&](const Run& r) {
        if (n < max_runs) { runs[3 * n] = r.first; runs[3 * n + 1] = r.n; runs[3 * n + 2] = r.bases; }
        n++;
    });
    *n_runs = n;
    return at;
}

uint64_t gap_capacity_for(uint64_t cap, uint64_t need, uint64_t first) { return capacity_for(cap, need, first); }
uint64_t gap_capacity_default(uint64_t cap, uint64_t need) { return capacity_for(cap, need); }
int gap_contigs_fit(uint64_t have, uint64_t more) { return contigs_fit(have, more) ? 1 : 0; }
int gap_seeds_fit(uint64_t have, uint64_t more) { return seeds_fit(have, more) ? 1 : 0; }
int gap_push_fits(uint64_t n_bases, uint64_t bias) { return push_fits(n_bases, bias) ? 1 : 0; }

}  // extern "C"
