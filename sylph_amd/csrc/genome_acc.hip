// genome_acc.hip — sketch_genome (sketch.rs:550-622) for ONE genome that does not fit one device batch: the genome arrives in pushes
// of whole contigs, each push below the batch limit of genomes.hip.  A push seeds its contigs (K1, position_road.hip), applies the
// contig rule and appends what is left of every valid seed — hash, global contig number, end position inside the contig: 16 bytes —
// to three arrays in HBM; nothing of the bases is kept.  The finish runs the genome-wide duplicate removal and the spacing filter of
// genomes.hip (filter_annotated_genomes) over everything accumulated, so the result is what one batch of all contigs would give.
// Why the cuts are exact, the capacity rule and the bounds: genome_acc_plan.h.
#include "genome_acc_plan.h"
#include "genomes.h"
#include "position_road.h"
#include "device_common.h"

struct sylph_genome_acc {
    sylph_ctx* ctx = nullptr;
    uint32_t c = 0, k = 0;
    int seed_mode = 0, pseudotax = 0;
    uint64_t min_spacing = 0;
    sylph::DevBuf hash, contig, end;      // `cap` seeds each; the first n_seeds are valid, in (contig, position) order
    uint64_t cap = 0, n_seeds = 0, n_contigs = 0, n_bases = 0;
    bool finished = false;
};

namespace sylph {

namespace {

namespace plan = genome_acc_plan;

// per survivor of a push (position order): does the contig rule keep it, and if so its global contig number and the end position
// inside the contig.  flag has a scan sentinel behind it that the host has zeroed.
__global__ __launch_bounds__(256) void acc_annotate_kernel(const uint64_t* __restrict__ contig_off, uint64_t n_contigs,
                                                           const uint32_t* __restrict__ pos, uint32_t n, uint32_t bias, uint32_t k,
                                                           int avx2_compat, uint32_t contig0, uint32_t* __restrict__ flag,
                                                           uint32_t* __restrict__ o_contig, uint32_t* __restrict__ o_end) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t p = (uint64_t)pos[i] - bias;   // K1 ran from the 16 B aligned address `bias` bytes below the push
    uint32_t ok = 0, contig = 0, endpos = 0;
    if (pos[i] >= bias && p < contig_off[n_contigs]) {
        const uint64_t r = find_record(contig_off, n_contigs, p);
        const uint64_t start = contig_off[r], L = contig_off[r + 1] - start;
        if ((p - start) < n_hashed_kmers(L, k, avx2_compat, 1)) {   // contig rule: nothing below 2k (avx2_seeding.rs:160)
            ok = 1;
            contig = contig0 + (uint32_t)r;                          // this push's numbers continue the earlier pushes'
            endpos = (uint32_t)(p - start + k - 1);                  // index of the k-mer's last base (seeding.rs:205)
        }
    }
    flag[i] = ok;
    o_contig[i] = contig;
    o_end[i] = endpos;
}

// the valid survivors behind the `base` seeds accumulated so far, order kept; base + (valid survivors) <= capacity (host-checked)
__global__ __launch_bounds__(256) void acc_append_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ fpos,
                                                         const uint64_t* __restrict__ hash, const uint32_t* __restrict__ contig,
                                                         const uint32_t* __restrict__ endp, uint32_t n, uint32_t base,
                                                         uint64_t* __restrict__ a_hash, uint32_t* __restrict__ a_contig,
                                                         uint32_t* __restrict__ a_end) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const uint32_t j = base + fpos[i];
    a_hash[j] = hash[i];
    a_contig[j] = contig[i];
    a_end[j] = endp[i];
}

// what the finish's sort carries (idx[i] = i) and the genome of every seed (one genome: 0)
__global__ __launch_bounds__(256) void acc_iota_kernel(uint32_t n, uint32_t* __restrict__ idx, uint32_t* __restrict__ gid) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    idx[i] = i;
    gid[i] = 0;
}

void swap_bufs(DevBuf& a, DevBuf& b) { std::swap(a.p, b.p); std::swap(a.cap, b.cap); }

// room for `need` seeds by the plan's rule; the arrays change hands only when all three new ones are there
void acc_reserve(sylph_genome_acc* a, uint64_t need) {
    sylph_ctx* ctx = a->ctx;
    const uint64_t first = ctx->genome_acc_first_capacity ? ctx->genome_acc_first_capacity : plan::FIRST_CAPACITY;
    const uint64_t cap = plan::capacity_for(a->cap, need, first);
    if (cap == a->cap) return;
    DevBuf h(ctx), c(ctx), e(ctx);
    h.alloc((size_t)cap * 8);
    c.alloc((size_t)cap * 4);
    e.alloc((size_t)cap * 4);
    if (a->n_seeds) {
        SY_HIP(hipMemcpyAsync(h.p, a->hash.p, (size_t)a->n_seeds * 8, hipMemcpyDeviceToDevice, ctx->stream));
        SY_HIP(hipMemcpyAsync(c.p, a->contig.p, (size_t)a->n_seeds * 4, hipMemcpyDeviceToDevice, ctx->stream));
        SY_HIP(hipMemcpyAsync(e.p, a->end.p, (size_t)a->n_seeds * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
    swap_bufs(a->hash, h);      // the old arrays go back to the pool behind the copies (stream order)
    swap_bufs(a->contig, c);
    swap_bufs(a->end, e);
    a->cap = cap;
}

void acc_push(sylph_genome_acc* a, const uint8_t* bases, const uint64_t* contig_off, uint64_t n_contigs, int mem) {
    sylph_ctx* ctx = a->ctx;
    SY_REQUIRE(!a->finished, "sylph_genome_acc_push after sylph_genome_acc_finish");
    SY_REQUIRE(mem == SYLPH_MEM_HOST || mem == SYLPH_MEM_DEVICE, "bad mem kind %d", mem);
    SY_REQUIRE(contig_off && contig_off[0] == 0, "bad contig offsets");
    for (uint64_t i = 0; i < n_contigs; i++) SY_REQUIRE(contig_off[i] <= contig_off[i + 1], "contig offsets must not decrease");
    const uint64_t n_bases = contig_off[n_contigs];
    SY_REQUIRE(plan::push_fits(n_bases, 0), "push larger than 2^32-1 bases: split it at a contig boundary");
    SY_REQUIRE(bases || n_bases == 0, "null bases");
    SY_REQUIRE(plan::contigs_fit(a->n_contigs, n_contigs), "more than 2^32-1 contigs in one genome");
    if (n_bases == 0) { a->n_contigs += n_contigs; return; }

    DeviceGuard dg(ctx->device);
    DevBuf d_bases(ctx), d_off(ctx);
    const uint8_t* db = bases;
    if (mem == SYLPH_MEM_HOST) {
        d_bases.reserve(n_bases + 64);
        ctx->h2d(d_bases.p, bases, n_bases);
        db = d_bases.as<uint8_t>();
    }
    d_off.reserve((n_contigs + 1) * 8);
    ctx->h2d(d_off.p, contig_off, (n_contigs + 1) * 8);
    ctx->counters.reserve(64);
    const uint32_t bias = (uint32_t)((uintptr_t)db & 15);   // a caller's device pointer need not be 16 B aligned
    SY_REQUIRE(plan::push_fits(n_bases, bias), "push larger than 2^32-1 bases: split it at a contig boundary");
    const PosSeeds seeds = seeds_sorted_by_pos(ctx, db - bias, n_bases + bias, a->c, a->k, ctx->counters.as<uint32_t>());
    const uint32_t n = seeds.n;
    uint32_t n_valid = 0;
    if (n) {
        const size_t n1 = (size_t)n + 1;
        DevBuf b_flag(ctx), b_fpos(ctx), b_contig(ctx), b_end(ctx);
        b_flag.reserve(n1 * 4); b_fpos.reserve(n1 * 4);
        b_contig.reserve((size_t)n * 4); b_end.reserve((size_t)n * 4);
        {
            ScopedKernelTimer t(ctx, "annotate");
            SY_HIP(hipMemsetAsync(b_flag.as<uint32_t>() + n, 0, 4, ctx->stream));   // scan sentinel
            hipLaunchKernelGGL(acc_annotate_kernel, dim3(grid_for64(n)), dim3(256), 0, ctx->stream, d_off.as<uint64_t>(), n_contigs,
                               seeds.pos, n, bias, a->k, a->seed_mode == SYLPH_SEED_AVX2_COMPAT, (uint32_t)a->n_contigs,
                               b_flag.as<uint32_t>(), b_contig.as<uint32_t>(), b_end.as<uint32_t>());
            SY_HIP(hipGetLastError());
        }
        exclusive_sum_u32(ctx, b_flag.as<uint32_t>(), b_fpos.as<uint32_t>(), n1);
        ctx->read_back(&n_valid, b_fpos.as<uint32_t>() + n, 4);
        SY_REQUIRE(n_valid <= n, "internal: inconsistent seed count");
        SY_REQUIRE(plan::seeds_fit(a->n_seeds, n_valid), "more than 2^32-2 seeds in one genome: raise c");
        if (n_valid) {
            acc_reserve(a, a->n_seeds + n_valid);
            ScopedKernelTimer t(ctx, "annotate");
            hipLaunchKernelGGL(acc_append_kernel, dim3(grid_for64(n)), dim3(256), 0, ctx->stream, b_flag.as<uint32_t>(),
                               b_fpos.as<uint32_t>(), seeds.hash, b_contig.as<uint32_t>(), b_end.as<uint32_t>(), n, (uint32_t)a->n_seeds,
                               a->hash.as<uint64_t>(), a->contig.as<uint32_t>(), a->end.as<uint32_t>());
            SY_HIP(hipGetLastError());
        }
    }
    a->n_seeds += n_valid;
    a->n_contigs += n_contigs;
    a->n_bases += n_bases;
}

void acc_finish(sylph_genome_acc* a, uint64_t** out_kmers, uint64_t* n_kmers, uint64_t** out_tracked, uint64_t* n_tracked) {
    sylph_ctx* ctx = a->ctx;
    SY_REQUIRE(!a->finished, "sylph_genome_acc_finish called twice");
    *out_kmers = nullptr;
    *n_kmers = 0;
    if (out_tracked) *out_tracked = nullptr;
    if (n_tracked) *n_tracked = 0;
    uint64_t koff[2] = {0, 0}, toff[2] = {0, 0};
    uint64_t *hk = nullptr, *ht = nullptr;
    if (a->n_seeds == 0) {
        hk = (uint64_t*)malloc(8);
        ht = (uint64_t*)malloc(8);
        if (!hk || !ht) { free(hk); free(ht); throw std::bad_alloc(); }
    } else {
        DeviceGuard dg(ctx->device);
        const uint32_t n = (uint32_t)a->n_seeds;   // <= MAX_SEEDS
        DevBuf b_idx(ctx), b_gid(ctx);
        b_idx.reserve((size_t)n * 4);
        b_gid.reserve((size_t)n * 4);
        hipLaunchKernelGGL(acc_iota_kernel, dim3(grid_for64(n)), dim3(256), 0, ctx->stream, n, b_idx.as<uint32_t>(), b_gid.as<uint32_t>());
        SY_HIP(hipGetLastError());
        // every accumulated seed is valid: its hash is its sort key
        filter_annotated_genomes(ctx, AnnotatedSeeds{a->hash.as<uint64_t>(), a->hash.as<uint64_t>(), a->contig.as<uint32_t>(),
                                                     a->end.as<uint32_t>(), b_gid.as<uint32_t>(), b_idx.as<uint32_t>(), n},
                                 1, a->min_spacing, a->pseudotax, &hk, koff, &ht, toff);
    }
    a->finished = true;
    a->hash.release(); a->contig.release(); a->end.release();
    a->cap = 0;
    *out_kmers = hk;
    *n_kmers = koff[1];
    if (out_tracked) *out_tracked = ht; else free(ht);
    if (n_tracked) *n_tracked = a->pseudotax ? toff[1] : 0;
}

}  // namespace

}  // namespace sylph

using namespace sylph;

extern "C" {

int sylph_genome_acc_create(sylph_ctx* ctx, uint32_t c, uint32_t k, int seed_mode, uint64_t min_spacing, int pseudotax,
                            sylph_genome_acc** out) {
    return guarded([&] {
        SY_REQUIRE(ctx && out, "null argument");
        *out = nullptr;
        SY_REQUIRE(c >= 1, "c must be >= 1");
        SY_REQUIRE(seed_mode == SYLPH_SEED_SCALAR || seed_mode == SYLPH_SEED_AVX2_COMPAT, "bad seed_mode %d", seed_mode);
        SY_REQUIRE(k == 21 || k == 31, "k must be 21 or 31 (avx2_seeding.rs:46-52)");
        sylph_genome_acc* a = new sylph_genome_acc;
        a->ctx = ctx;
        a->c = c; a->k = k; a->seed_mode = seed_mode; a->min_spacing = min_spacing; a->pseudotax = pseudotax ? 1 : 0;
        a->hash.ctx = a->contig.ctx = a->end.ctx = ctx;
        ctx->refs++;                          // sylph_genome_acc_destroy gives it back
        *out = a;
    });
}

int sylph_genome_acc_push(sylph_genome_acc* a, const uint8_t* bases, const uint64_t* contig_off, uint64_t n_contigs, int mem) {
    return guarded([&] {
        SY_REQUIRE(a, "null argument");
        std::lock_guard<std::mutex> lock(a->ctx->mu);
        acc_push(a, bases, contig_off, n_contigs, mem);
    });
}

int sylph_genome_acc_counts(const sylph_genome_acc* a, uint64_t* n_contigs, uint64_t* n_bases, uint64_t* n_seeds) {
    return guarded([&] {
        SY_REQUIRE(a, "null argument");
        std::lock_guard<std::mutex> lock(a->ctx->mu);
        if (n_contigs) *n_contigs = a->n_contigs;
        if (n_bases) *n_bases = a->n_bases;
        if (n_seeds) *n_seeds = a->n_seeds;
    });
}

int sylph_genome_acc_finish(sylph_genome_acc* a, uint64_t** out_kmers, uint64_t* n_kmers, uint64_t** out_tracked, uint64_t* n_tracked) {
    return guarded([&] {
        SY_REQUIRE(a && out_kmers && n_kmers, "null argument");
        std::lock_guard<std::mutex> lock(a->ctx->mu);
        acc_finish(a, out_kmers, n_kmers, out_tracked, n_tracked);
    });
}

void sylph_genome_acc_destroy(sylph_genome_acc* a) {
    if (!a) return;
    sylph_ctx* ctx = a->ctx;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        a->hash.release(); a->contig.release(); a->end.release();   // to the pool: reuse is stream-ordered behind the kernels that read them
        delete a;
    }
    ctx_unref(ctx);
}

}  // extern "C"
