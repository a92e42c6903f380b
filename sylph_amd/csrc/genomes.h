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

// n >= 1 survivors in (genome, contig, position) order, on the device: the sort key (the hash, or INVALID_HASH for a survivor the
// contig rule drops), the hash, the contig, the end position inside it, the genome, and idx[i] = i.
struct AnnotatedSeeds {
    const uint64_t *key, *hash;
    const uint32_t *contig, *end, *gid, *idx;
    uint32_t n;
};
// The genome-wide duplicate removal and the spacing filter over them (sketch.rs:590-614), copied out as sketch_genomes_impl's
// outputs.  The caller holds ctx->mu.
void filter_annotated_genomes(sylph_ctx* ctx, const AnnotatedSeeds& a, uint64_t n_genomes, uint64_t min_spacing, int pseudotax,
                              uint64_t** out_kmers, uint64_t* kmer_off, uint64_t** out_tracked, uint64_t* tracked_off);

}  // namespace sylph
