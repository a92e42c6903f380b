// genomes.h — the batch genome sketch of genomes.hip, for the callers that gather their batch on the device (fasta.hip).
#pragma once
#include "common.h"

namespace sylph {

// sketch_genome for genomes [genome_contig_off[g], genome_contig_off[g + 1]) of the contigs at `bases` (mem: SYLPH_MEM_HOST or
// SYLPH_MEM_DEVICE); the ABI's sylph_sketch_genomes without its guard.  *out_kmers / *out_tracked are malloc'ed.
void sketch_genomes_impl(sylph_ctx* ctx, const uint8_t* bases, const uint64_t* contig_off, uint64_t n_contigs,
                         const uint64_t* genome_contig_off, uint64_t n_genomes, uint32_t c, uint32_t k, int seed_mode,
                         uint64_t min_spacing, int pseudotax, int mem, uint64_t** out_kmers, uint64_t* kmer_off, uint64_t** out_tracked,
                         uint64_t* tracked_off);

}  // namespace sylph
