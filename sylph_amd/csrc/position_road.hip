// position_road.hip — everything that seeds by flat position and annotates afterwards, on gfx950.
//
//   K1 seeds (seeds.hip) -> survivors sorted by flat position (seeds_sorted_by_pos: ordered slots + scan, else the unordered kernel +
//   radix sort) -> K2 annotate: record lookup, boundary / AVX2-tail validation and, for reads, the locality markers.
//
// Takes the read batches the short-read kernel (reads.hip) declines or is not asked for (sketch.hip process_batch), every genome
// (genomes.hip; sylph_seeds_positions here) and the single-sequence entry sylph_seeds.
#include <algorithm>

#include "common.h"
#include "device_common.h"
#include "position_road.h"
#include "seeds.h"

namespace sylph {
namespace {

// 32 consecutive bases starting at p (any alignment) -> (even-position 16-mer, odd-position 16-mer), each base a
// 2-bit BYTE_TO_SEQ code, first base most significant (the order pair_kmer[_single] builds them in,
// sketch.rs:636-653,:668-685).  Two unaligned 16-byte loads instead of 32 byte loads.
__device__ __forceinline__ void marker_halves(const uint8_t* __restrict__ p, uint32_t& even, uint32_t& odd) {
    uint32_t e = 0, o = 0;
    uint64_t xs[4];
    __builtin_memcpy(&xs[0], p, 16);
    __builtin_memcpy(&xs[2], p + 16, 16);
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const uint64_t x = xs[w];
        uint32_t bad = 0;
        uint32_t lo = codes4_fast((uint32_t)x, bad), hi = codes4_fast((uint32_t)(x >> 32), bad);
        if (bad) { lo = codes4_exact((uint32_t)x); hi = codes4_exact((uint32_t)(x >> 32)); }
        // byte lanes b0..b3 of lo, b4..b7 of hi hold bases 8w..8w+7
        const uint32_t ev = ((lo & 3u) << 6) | (((lo >> 16) & 3u) << 4) | ((hi & 3u) << 2) | ((hi >> 16) & 3u);
        const uint32_t od = (((lo >> 8) & 3u) << 6) | (((lo >> 24) & 3u) << 4) | (((hi >> 8) & 3u) << 2) | ((hi >> 24) & 3u);
        e = (e << 8) | ev;
        o = (o << 8) | od;
    }
    even = e;
    odd = o;
}

// Coarse record index of a batch: coarse[t] = record containing flat base t * 2^COARSE_SHIFT (the last record for
// positions at or beyond the end).  One thread per entry, all binary searches in flight at once — so the annotate
// kernel's workgroups need ONE dependent load to bound their record window instead of a 23-step search each
// (that chain of L2/HBM round trips was half of the kernel's time).
constexpr int COARSE_SHIFT = 14;
__global__ __launch_bounds__(256) void coarse_index_kernel(const uint64_t* __restrict__ off, uint64_t n_rec, uint32_t n_entries,
                                                           uint32_t* __restrict__ coarse) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_entries) return;
    const uint64_t total = off[n_rec];
    uint64_t p = (uint64_t)t << COARSE_SHIFT;
    if (total == 0) { coarse[t] = 0; return; }
    if (p >= total) p = total - 1;
    coarse[t] = (uint32_t)find_record(off, n_rec, p);
}

// ---- K2: annotate survivors of one batch (already sorted by flat position) ---------------------------------
// Validates that the k-mer lies inside one record and among the k-mers the reference hashes, finds the record,
// and computes the dedup markers.  Invalid survivors get hash = ~0 (sorts last, dropped in finish()).
// Survivors arrive sorted by position, so a workgroup's 256 survivors span a short run of records: two lanes bound
// it through the coarse index (first and last survivor), the run's offsets are staged in LDS and every lane searches
// only inside that run.
template <bool LIGHT>   // LIGHT: validity only — o_hash, no markers, no OccRec (marker-less single-end batches)
__global__ __launch_bounds__(256) void annotate_reads_kernel(
    const uint8_t* __restrict__ bases, const uint64_t* __restrict__ off, uint64_t n_rec, const uint32_t* __restrict__ pos, const uint64_t* __restrict__ hash,
    uint32_t n, uint32_t pos_bias, uint32_t k, int avx2_compat, int paired, int want_markers, uint64_t rec_base, const uint32_t* __restrict__ coarse,
    uint64_t* __restrict__ o_hash, OccRec* __restrict__ o_rec) {
    constexpr uint32_t WIN = 1024;           // record offsets staged in LDS (8 KiB)
    __shared__ uint64_t s_lo, s_hi;
    __shared__ uint64_t s_off[WIN + 2];
    const uint32_t first = blockIdx.x * blockDim.x;
    const uint32_t i = first + threadIdx.x;
    const uint64_t total = off[n_rec];
    if (threadIdx.x == 0 || threadIdx.x == 64) {
        const uint32_t j = threadIdx.x == 0 ? first : min(n, first + blockDim.x) - 1;
        uint64_t p = pos[j] >= pos_bias ? pos[j] - pos_bias : 0;   // positions are relative to the 16 B-aligned load base
        if (total && p >= total) p = total - 1;
        // the record of p lies in [coarse[t], coarse[t + 1]]: bound the window with those instead of searching for it
        const uint64_t t = p >> COARSE_SHIFT;
        if (threadIdx.x == 0) s_lo = total ? coarse[t] : 0; else s_hi = (total ? coarse[t + 1] : 0) + 1;
    }
    __syncthreads();
    // stage off[s_lo .. s_hi + 1] (the run of records this workgroup's survivors fall into, +1 for the mate lookup)
    const uint64_t w_lo = s_lo & ~1ull;      // even, so a pair's three offsets are inside the window too
    const uint64_t w_n = min(s_hi + 2, n_rec + 1) - w_lo;
    const bool in_lds = w_n <= WIN + 2;
    if (in_lds)
        for (uint32_t t = threadIdx.x; t < w_n; t += blockDim.x) s_off[t] = off[w_lo + t];
    __syncthreads();
    const bool live = i < n && pos[i] >= pos_bias;
    const uint64_t p = live ? pos[i] - pos_bias : ~0ull;
    uint64_t h = live ? hash[i] : 0, rid = 0, m0 = 0, m1 = 0;
    bool valid = false;
    if (p < total) {
        // record search + the (up to five) offsets needed, from LDS when the run fits (the usual case) — kept as two
        // separate code paths so that the LDS one compiles to ds_read, not to flat loads through a selected pointer
        uint64_t r, start, L, s1 = 0, s2 = 0, e2 = 0;
        auto locate = [&](auto OFF) {
            uint64_t lo = s_lo, hi = s_hi;   // off[lo] <= p < off[hi]
            while (hi - lo > 1) {
                const uint64_t mid = (lo + hi) >> 1;
                if (OFF(mid) <= p) lo = mid; else hi = mid;
            }
            r = lo;
            start = OFF(r);
            L = OFF(r + 1) - start;
            if (paired) { const uint64_t r1 = r & ~1ull; s1 = OFF(r1); s2 = OFF(r1 + 1); e2 = OFF(r1 + 2); }
        };
        if (in_lds) locate([&](uint64_t q) -> uint64_t { return s_off[q - w_lo]; });
        else locate([&](uint64_t q) -> uint64_t { return off[q]; });
        valid = (p - start) < n_hashed_kmers(L, k, avx2_compat, 0);
        if (valid) {
            rid = rec_base + r;
            if (!LIGHT && want_markers) {
                const uint8_t* a = nullptr;
                const uint8_t* b = nullptr;
                if (!paired) {
                    // pair_kmer_single, sketch.rs:625-656; caller passes None above 400 bp (sketch.rs:922-927)
                    if (L >= 66 && L <= 400) { a = bases + start; b = a + L / 2; }
                } else {
                    // pair_kmer, sketch.rs:659-688: both mates >= 33 bp
                    if (s2 - s1 >= 33 && e2 - s2 >= 33) { a = bases + s1; b = bases + s2; }
                }
                if (a) {
                    uint32_t f, g, rr, t;
                    marker_halves(a, f, g);    // f: bases 0,2,..,30   g: bases 1,3,..,31
                    marker_halves(b, rr, t);
                    m0 = (uint64_t)f | ((uint64_t)rr << 32);
                    m1 = (uint64_t)g | ((uint64_t)t << 32);
                    rid |= RID_MARKER_BIT;
                    if (paired)
                        rid |= min(emission_rank((uint32_t)(p - start), (uint32_t)n_hashed_kmers(L, k, avx2_compat, 0), avx2_compat), RID_RANK_MAX)
                               << RID_RANK_SHIFT;
                }
            }
        }
    }
    if (i < n) {
        const uint64_t hv = valid ? h : INVALID_HASH;
        o_hash[i] = hv;
        if constexpr (!LIGHT) o_rec[i] = OccRec{hv, rid, m0, m1};
    }
    // (no counter of valid survivors here: one atomic per wavefront on a single word runs at ~88 atomics/us and was
    //  the whole 0.9 ms of this kernel; finish() finds the count by binary search in the hash-sorted array instead)
}

// Genome flavour: (contig, end position, hash), validated with the positions-variant rules
// (avx2_seeding.rs:160: nothing for contigs shorter than 2k).
__global__ __launch_bounds__(256) void annotate_contigs_kernel(const uint64_t* __restrict__ off, uint64_t n_contigs, const uint32_t* __restrict__ pos,
                                                               const uint64_t* __restrict__ hash, uint32_t n, uint32_t k, int avx2_compat,
                                                               uint32_t* __restrict__ o_contig, uint64_t* __restrict__ o_pos, uint64_t* __restrict__ o_hash) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t p = pos[i];
    uint64_t h = INVALID_HASH, endpos = 0;
    uint32_t contig = 0;
    if (p < off[n_contigs]) {
        const uint64_t r = find_record(off, n_contigs, p);
        const uint64_t start = off[r], L = off[r + 1] - start;
        if ((p - start) < n_hashed_kmers(L, k, avx2_compat, 1)) {
            h = hash[i];
            contig = (uint32_t)r;
            endpos = p - start + k - 1;   // index of the k-mer's last base (seeding.rs:205)
        }
    }
    o_contig[i] = contig;
    o_pos[i] = endpos;
    o_hash[i] = h;
}

}  // namespace

// Runs K1 with capacity retry; returns the survivors sorted by flat position.  Scratch slots: sylph_ctx::scratch (common.h).
PosSeeds seeds_sorted_by_pos(sylph_ctx* ctx, const uint8_t* d_bases, uint64_t n_bases, uint32_t c, uint32_t k, uint32_t* d_count) {
    SY_REQUIRE(n_bases < (1ull << 32), "a batch may hold at most 2^32-1 bases (got %llu)", (unsigned long long)n_bases);
    const PosSeeds none{nullptr, nullptr, 0};
    if (n_bases == 0) return none;
    DevBuf &b_pos = ctx->scratch[2], &b_hash = ctx->scratch[3];   // the result
    if (ctx->seeds_mode != 1) {
        // ordered K1: per-tile slots in position order, then scan + gather (no radix sort, no atomics)
        HostPhase ph(ctx, "push: seeds (ordered slots)");
        const uint32_t n_tiles = seeds_n_tiles(n_bases), slot_cap = seeds_slot_capacity(c);
        DevBuf &b_sh = ctx->scratch[0], &b_sp = ctx->scratch[1], &b_tc = ctx->scratch[4];
        b_sh.reserve((size_t)n_tiles * slot_cap * 8);
        b_sp.reserve((size_t)n_tiles * slot_cap * 4);
        // [tile_count (n_tiles+1) | tile_off (n_tiles+1) | spill_slot_of_tile (n_tiles) | SpillState]
        b_tc.reserve(((size_t)n_tiles + 1) * 4 * 3 + sizeof(SpillState) + 16);
        uint32_t* tile_count = b_tc.as<uint32_t>();
        uint32_t* tile_off = tile_count + (n_tiles + 1);
        uint32_t* spill_slot = tile_off + (n_tiles + 1);
        SpillState* d_spill = reinterpret_cast<SpillState*>(spill_slot + n_tiles + 1);
        SY_HIP(hipMemsetAsync(tile_count + n_tiles, 0, 4, ctx->stream));   // scan sentinel
        SY_HIP(hipMemsetAsync(d_spill, 0, 4, ctx->stream));                // n_tiles of the spill list
        launch_seeds_slots(ctx, d_bases, (uint32_t)n_bases, c, k, slot_cap, b_sh.as<uint64_t>(), b_sp.as<uint32_t>(), tile_count, d_spill, nullptr, 0, nullptr);
        exclusive_sum_u32(ctx, tile_count, tile_off, (size_t)n_tiles + 1);
        uint32_t res[2] = {0, 0};   // total survivors, tiles that overflowed their slots
        SY_HIP(hipMemcpyAsync(ctx->pinned, tile_off + n_tiles, 4, hipMemcpyDeviceToHost, ctx->stream));
        SY_HIP(hipMemcpyAsync((uint8_t*)ctx->pinned + 4, d_spill, 4, hipMemcpyDeviceToHost, ctx->stream));
        SY_HIP(hipStreamSynchronize(ctx->stream));
        memcpy(res, ctx->pinned, 8);
        if (!ctx->pending.empty()) profile_collect(ctx);
        if (res[1] <= SPILL_MAX_TILES) {
            if (res[0] == 0) return none;
            uint64_t* xh = nullptr;   // the spill regions, if any: [hashes | positions]
            uint32_t* xp = nullptr;
            if (res[1]) {   // a few tiles (low-complexity reads, repeats) are redone with room for every position
                DevBuf& b_x = ctx->scratch[7];
                const size_t tb = seeds_tile_bases();
                b_x.reserve((size_t)res[1] * tb * 12);
                xh = b_x.as<uint64_t>();
                xp = reinterpret_cast<uint32_t*>(xh + (size_t)res[1] * tb);
                ScopedKernelTimer ts(ctx, "seeds_spill");   // (family of its own so that tests can see this path was taken)
                launch_seeds_slots(ctx, d_bases, (uint32_t)n_bases, c, k, slot_cap, xh, xp, tile_count, d_spill, d_spill->tiles, res[1], spill_slot);
            }
            b_pos.reserve((size_t)res[0] * 4);
            b_hash.reserve((size_t)res[0] * 8);
            launch_compact_slots(ctx, b_sh.as<uint64_t>(), b_sp.as<uint32_t>(), tile_count, tile_off, n_tiles, slot_cap, xh, xp, spill_slot,
                                 b_pos.as<uint32_t>(), b_hash.as<uint64_t>());
            return PosSeeds{b_pos.as<uint32_t>(), b_hash.as<uint64_t>(), res[0]};
        }
        // more overflowing tiles than spill regions (a batch dominated by repeats): redo it with the unordered kernel
    }
    uint64_t cap = n_bases / c + n_bases / (4ull * c) + 65536;
    if (cap > n_bases) cap = n_bases;
    uint32_t n = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        HostPhase ph(ctx, "push: seeds kernel");
        ctx->scratch[0].reserve(cap * 8);   // hash (unsorted)
        ctx->scratch[1].reserve(cap * 4);   // pos (unsorted)
        static const bool slowlog = getenv("SYLPH_HIP_SLOWLOG") != nullptr;
        const double t0 = slowlog ? HostPhase::now() : 0;
        SY_HIP(hipMemsetAsync(d_count, 0, 4, ctx->stream));
        const double t1 = slowlog ? HostPhase::now() : 0;
        if (slowlog && t1 - t0 > 3.0) fprintf(stderr, "[sylph_hip] slow memset issue %.3f ms\n", t1 - t0);
        launch_seeds(ctx, d_bases, (uint32_t)n_bases, c, k, ctx->scratch[0].as<uint64_t>(), ctx->scratch[1].as<uint32_t>(), (uint32_t)cap, d_count);
        ctx->read_back(&n, d_count, 4);
        if (n <= cap) break;
        cap = n;                            // the counter kept counting: exact size for the retry
        SY_REQUIRE(attempt == 0, "seed buffer overflow persisted");
    }
    if (n == 0) return none;
    HostPhase ph(ctx, "push: sort by position");
    b_pos.reserve((size_t)n * 4);
    b_hash.reserve((size_t)n * 8);
    sort_pairs_u32_u64(ctx, ctx->scratch[1].as<uint32_t>(), b_pos.as<uint32_t>(), ctx->scratch[0].as<uint64_t>(), b_hash.as<uint64_t>(), n, 0,
                       std::max(1, bit_length(n_bases)));
    return PosSeeds{b_pos.as<uint32_t>(), b_hash.as<uint64_t>(), n};
}

void annotate_reads(sylph_sketch* sk, const uint8_t* d_bases, const uint64_t* d_off, uint64_t n_records, uint64_t n_bases, uint32_t bias,
                    const PosSeeds& s, bool plain) {
    sylph_ctx* ctx = sk->ctx;
    const uint32_t n_coarse = (uint32_t)(n_bases >> COARSE_SHIFT) + 2;
    DevBuf& b_coarse = ctx->scratch[5];
    b_coarse.reserve((size_t)n_coarse * 4);
    ScopedKernelTimer t(ctx, "annotate");
    hipLaunchKernelGGL(coarse_index_kernel, dim3(grid_for64(n_coarse)), dim3(256), 0, ctx->stream, d_off, n_records, n_coarse, b_coarse.as<uint32_t>());
    auto annotate = [&](auto kernel, int want_markers, OccRec* o_rec) {
        hipLaunchKernelGGL(kernel, dim3(grid_for64(s.n)), dim3(256), 0, ctx->stream, d_bases, d_off, n_records, s.pos, s.hash, s.n, bias, sk->k, sk->avx2_compat,
                           sk->paired, want_markers, sk->rec_base, b_coarse.as<uint32_t>(), sk->hash.as<uint64_t>() + sk->n_occ, o_rec);
    };
    if (plain) annotate(annotate_reads_kernel<true>, 0, nullptr);
    else annotate(annotate_reads_kernel<false>, sk->no_dedup ? 0 : 1, sk->recs.as<OccRec>() + sk->n_occ);
    SY_HIP(hipGetLastError());
}

// ---- genome side -------------------------------------------------------------------------------------------

struct ContigSeeds { std::vector<uint32_t> contig; std::vector<uint64_t> pos, hash; };

static void seeds_positions_impl(sylph_ctx* ctx, const uint8_t* bases, const uint64_t* contig_off, uint64_t n_contigs, uint32_t c, uint32_t k, int seed_mode, ContigSeeds& out) {
    SY_REQUIRE(c >= 1, "c must be >= 1");
    SY_REQUIRE(seed_mode == SYLPH_SEED_SCALAR || seed_mode == SYLPH_SEED_AVX2_COMPAT, "bad seed_mode %d", seed_mode);
    SY_REQUIRE(k == 21 || k == 31, "k must be 21 or 31 (avx2_seeding.rs:46-52)");
    if (n_contigs == 0) return;
    SY_REQUIRE(contig_off && contig_off[0] == 0, "bad contig offsets");
    SY_REQUIRE(bases || contig_off[n_contigs] == 0, "null bases");
    SY_REQUIRE(n_contigs < (1ull << 32), "too many contigs");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard dg(ctx->device);
    const uint64_t n_bases = contig_off[n_contigs];
    SY_REQUIRE(n_bases < (1ull << 32), "genome larger than 2^32-1 bases: split by contig");
    DevBuf d_bases(ctx), d_off(ctx);
    d_bases.reserve(n_bases + 64);
    d_off.reserve((n_contigs + 1) * 8);
    ctx->h2d(d_bases.p, bases, n_bases);
    ctx->h2d(d_off.p, contig_off, (n_contigs + 1) * 8);
    ctx->counters.reserve(64);
    const PosSeeds s = seeds_sorted_by_pos(ctx, d_bases.as<uint8_t>(), n_bases, c, k, ctx->counters.as<uint32_t>());
    const uint32_t n = s.n;
    if (!n) return;
    DevBuf o_contig(ctx), o_pos(ctx), o_hash(ctx);
    o_contig.reserve((size_t)n * 4);
    o_pos.reserve((size_t)n * 8);
    o_hash.reserve((size_t)n * 8);
    {
        ScopedKernelTimer t(ctx, "annotate");
        hipLaunchKernelGGL(annotate_contigs_kernel, dim3(grid_for64(n)), dim3(256), 0, ctx->stream, d_off.as<uint64_t>(), n_contigs, s.pos, s.hash, n, k,
                           seed_mode == SYLPH_SEED_AVX2_COMPAT, o_contig.as<uint32_t>(), o_pos.as<uint64_t>(), o_hash.as<uint64_t>());
        SY_HIP(hipGetLastError());
    }
    std::vector<uint32_t> hc(n);
    std::vector<uint64_t> hp(n), hh(n);
    ctx->d2h(hc.data(), o_contig.p, (size_t)n * 4);
    ctx->d2h(hp.data(), o_pos.p, (size_t)n * 8);
    ctx->d2h(hh.data(), o_hash.p, (size_t)n * 8);
    out.contig.reserve(n); out.pos.reserve(n); out.hash.reserve(n);
    for (uint32_t i = 0; i < n; i++) {
        if (hh[i] == INVALID_HASH) continue;   // straddled a contig boundary / AVX2 tail / short contig
        out.contig.push_back(hc[i]); out.pos.push_back(hp[i]); out.hash.push_back(hh[i]);
    }
}

template <class T>
static T* to_malloc(const std::vector<T>& v) {
    T* p = (T*)malloc(std::max<size_t>(1, v.size()) * sizeof(T));
    if (!p) throw std::bad_alloc();
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

}  // namespace sylph

using namespace sylph;

extern "C" {

int sylph_seeds_positions(sylph_ctx* ctx, const uint8_t* bases, const uint64_t* contig_off, uint64_t n_contigs, uint32_t c,
                          uint32_t k, int seed_mode, uint32_t** out_contig, uint64_t** out_pos, uint64_t** out_hash,
                          uint64_t* out_n) {
    return guarded([&] {
        SY_REQUIRE(ctx && out_contig && out_pos && out_hash && out_n, "null argument");
        ContigSeeds s;
        seeds_positions_impl(ctx, bases, contig_off, n_contigs, c, k, seed_mode, s);
        *out_contig = to_malloc(s.contig);
        *out_pos = to_malloc(s.pos);
        *out_hash = to_malloc(s.hash);
        *out_n = s.hash.size();
    });
}

int sylph_seeds(sylph_ctx* ctx, const uint8_t* bases, uint64_t len, uint32_t c, uint32_t k, int seed_mode,
                uint64_t** out_hashes, uint64_t* out_n) {
    return guarded([&] {
        SY_REQUIRE(ctx && out_hashes && out_n, "null argument");
        // one record; the read rule for short sequences (k+1, avx2_seeding.rs:42) differs from the contig rule
        // (2k, :160), so run the read flavour through a throw-away session-less path
        SY_REQUIRE(c >= 1, "c must be >= 1");
        SY_REQUIRE(k == 21 || k == 31, "k must be 21 or 31 (avx2_seeding.rs:46-52)");
        SY_REQUIRE(seed_mode == SYLPH_SEED_SCALAR || seed_mode == SYLPH_SEED_AVX2_COMPAT, "bad seed_mode %d", seed_mode);
        std::vector<uint64_t> res;
        if (len) {
            SY_REQUIRE(bases, "null bases");
            SY_REQUIRE(len < (1ull << 32), "sequence longer than 2^32-1 bases");
            std::lock_guard<std::mutex> lock(ctx->mu);
            DeviceGuard dg(ctx->device);
            DevBuf d_bases(ctx);
            d_bases.reserve(len + 64);
            ctx->h2d(d_bases.p, bases, len);
            ctx->counters.reserve(64);
            const PosSeeds s = seeds_sorted_by_pos(ctx, d_bases.as<uint8_t>(), len, c, k, ctx->counters.as<uint32_t>());
            if (const uint32_t n = s.n) {
                std::vector<uint32_t> hp(n);
                std::vector<uint64_t> hh(n);
                ctx->d2h(hp.data(), s.pos, (size_t)n * 4);
                ctx->d2h(hh.data(), s.hash, (size_t)n * 8);
                const uint64_t nk = n_hashed_kmers(len, k, seed_mode == SYLPH_SEED_AVX2_COMPAT, 0);
                for (uint32_t i = 0; i < n; i++)
                    if (hp[i] < nk) res.push_back(hh[i]);
            }
        }
        *out_hashes = to_malloc(res);
        *out_n = res.size();
    });
}

}  // extern "C"
