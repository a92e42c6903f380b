// genome_acc_plan.h — the plan of the genome accumulator (genome_acc.hip) and of the host that feeds it (host/cmd_sketch.cpp),
// host-compilable: how a file's contigs are cut into pushes, how the accumulated arrays grow, and the bounds of one accumulator.
// All arithmetic is 64-bit and written so that nothing wraps for any u64 input.  tests/test_genome_acc_plan.py compiles it with g++
// (tests/genome_acc_plan_capi.cpp).
//
// Why a cut at a contig boundary is exact: the seeding hashes the k-mers of one contig from that contig's bases alone, the contig rule
// (n_hashed_kmers) looks at one contig's length, and the spacing chain restarts at every contig (sketch.rs:606).  What spans contigs is
// the duplicate set alone (sketch.rs:590-600), and that is applied by the finish over everything accumulated.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sylph {
namespace genome_acc_plan {

// one push (one sylph_sketch_genomes batch) holds fewer bases than this: 2^32 less the room the seeding kernels' alignment bias and
// tile padding take
constexpr uint64_t PUSH_LIMIT = (1ull << 32) - 4096;
// contig numbers are u32
constexpr uint64_t MAX_CONTIGS = (1ull << 32) - 1;
// the finish indexes seeds by u32 and scans n + 1 entries (the sentinel), as sketch_genomes_impl does
constexpr uint64_t MAX_SEEDS = (1ull << 32) - 2;
constexpr uint64_t FIRST_CAPACITY = 1ull << 20;   // seeds; 16 bytes each

// ---- the cut -------------------------------------------------------------------------------------------------------------------
// A run: contigs [first, first + n) with `bases` bases in all, bases < limit.
struct Run { uint64_t first, n, bases; };

// The run that begins at contig `from`, greedy: it takes whole contigs for as long as the sum stays below `limit`, so it ends at the
// end of the list or where the next contig would not fit.  n == 0 with from < n_contigs: contig `from` alone holds `limit` bases or
// more (a misfit); from >= n_contigs gives the empty run at n_contigs.
inline Run next_run(const uint64_t* lens, uint64_t n_contigs, uint64_t from, uint64_t limit) {
    Run r{from < n_contigs ? from : n_contigs, 0, 0};
    for (uint64_t i = r.first; i < n_contigs; i++) {
        if (limit == 0 || lens[i] >= limit - r.bases) break;   // bases < limit here, so the difference is positive
        r.bases += lens[i];
        r.n++;
    }
    return r;
}

// The runs of contigs [from, ...) up to the first misfit, through `emit(Run)`.  Returns the index of that misfit, n_contigs when there
// is none: a caller that may skip a contig (one genome per record) goes on behind it, one that may not (one genome per file) gives up.
template <class F>
inline uint64_t cut(const uint64_t* lens, uint64_t n_contigs, uint64_t from, uint64_t limit, F&& emit) {
    uint64_t at = from < n_contigs ? from : n_contigs;
    while (at < n_contigs) {
        const Run r = next_run(lens, n_contigs, at, limit);
        if (r.n == 0) return at;
        emit(r);
        at += r.n;
    }
    return n_contigs;
}

// ---- the accumulated arrays ----------------------------------------------------------------------------------------------------
// The capacity (seeds) that holds `need` <= MAX_SEEDS seeds, from an array of `cap` (0: none yet): unchanged while it fits, else
// max(cap, first) doubled until it does, never beyond MAX_SEEDS.  Monotone in need and in cap; >= need.
inline uint64_t capacity_for(uint64_t cap, uint64_t need, uint64_t first = FIRST_CAPACITY) {
    if (need <= cap) return cap;
    uint64_t c = cap > first ? cap : first;
    if (c < 1) c = 1;
    while (c < need && c < MAX_SEEDS) c = c > MAX_SEEDS / 2 ? MAX_SEEDS : c * 2;
    return c < MAX_SEEDS ? c : MAX_SEEDS;   // (a need beyond MAX_SEEDS is the caller's to refuse: seeds_fit)
}

// ---- the bounds ----------------------------------------------------------------------------------------------------------------
inline bool contigs_fit(uint64_t have, uint64_t more) { return have <= MAX_CONTIGS && more <= MAX_CONTIGS - have; }
inline bool seeds_fit(uint64_t have, uint64_t more) { return have <= MAX_SEEDS && more <= MAX_SEEDS - have; }
inline bool push_fits(uint64_t n_bases, uint64_t bias) { return n_bases < (1ull << 32) && bias < (1ull << 32) - n_bases; }

}  // namespace genome_acc_plan
}  // namespace sylph
