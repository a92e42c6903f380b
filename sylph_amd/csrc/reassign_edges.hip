// reassign_edges.hip — the reassignment log of `profile --log-reassignments` (contain.rs:432-456): for every passing genome, how
// many of its genome_kmers the winner table hands to which other passing genome.  The reference walks every passing genome's k-mers
// through the hash map its winner_table built; here the winner table exists only as the resident line indexes + rank_of / ani
// (contain_index.h winner_of, the search reassign_kernel makes per sample k-mer), so the caller's copy of the passing genomes'
// k-mers is run through it:
//   edge_winner_kernel   flat over all query k-mers, one per lane: the winner's rank (or ~0) into a u32 array parallel to the query
//   edge_count_kernel    one workgroup per (loser, window of winner ranks): counts the loser's slice of that array in LDS and
//                        appends the counts that reach min_count to a bounded edge list
// and the few edges are sorted on the host.  The arithmetic of the second launch is reassign_edges_plan.h.  Unmeasured so far:
// the window size (reassign_edges_plan.h WINDOW_DEFAULT) is a guess.
#include <memory>

#include "contain_index.h"
#include "reassign_edges_plan.h"
#include "device_common.h"

namespace sylph {
namespace {

static_assert(sizeof(edge_plan::Edge) == sizeof(sylph_reassign_edge) && offsetof(edge_plan::Edge, winner) == offsetof(sylph_reassign_edge, winner) &&
              offsetof(edge_plan::Edge, loser) == offsetof(sylph_reassign_edge, loser) && offsetof(edge_plan::Edge, count) == offsetof(sylph_reassign_edge, count),
              "the plan's Edge is the ABI's sylph_reassign_edge");

constexpr int WINNER_TPB = 256;
constexpr uint32_t WINNER_GRID = 1024;

// winner[i] = rank of the passing genome that owns query k-mer i, or ~0 when no passing genome holds it.  Persistent workgroups
// striding over 256-k-mer chunks, like reassign_kernel: the load balance does not depend on the genomes' sizes.
__global__ __launch_bounds__(WINNER_TPB) void edge_winner_kernel(const uint64_t* __restrict__ q_kmers, uint32_t n_q, LineView kept, LineView tracked,
                                                                 int have_tracked, const uint32_t* __restrict__ rank,
                                                                 const double* __restrict__ ani, uint32_t* __restrict__ winner) {
    const uint32_t n_chunks = (n_q + WINNER_TPB - 1) / WINNER_TPB;
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t i = chunk * WINNER_TPB + threadIdx.x;
        const bool live = i < n_q;
        const uint64_t km = live ? q_kmers[i] : 0;
        uint32_t n_kept;
        const uint32_t w = winner_of<false>(kept, tracked, have_tracked, km, live, rank, ani, n_kept);
        if (live) winner[i] = w;
    }
}

// Work item blockIdx.x (edge_plan::work_item): the loser losers[loser_slot], whose k-mers are the entries [off[loser], off[loser + 1])
// of the winner array, and the winner ranks [window_base, window_base + window_len).  cnt[w - window_base] += 1 for every entry
// in the window that is not the loser itself (LDS atomics without return); then the window is scanned in ascending order, tile
// by tile, and the counts that reach min_count go to edges[] from ONE reservation on *cursor.  A workgroup whose reservation
// passes `cap` writes what fits; the host sees cursor > cap and launches again with room for all.
__global__ __launch_bounds__(edge_plan::COUNT_TPB) void edge_count_kernel(const uint32_t* __restrict__ winner, const uint64_t* __restrict__ off,
                                                                          const uint32_t* __restrict__ losers, uint32_t n_passing, uint32_t window,
                                                                          uint32_t min_count, edge_plan::Edge* __restrict__ edges, uint32_t cap,
                                                                          uint32_t* __restrict__ cursor) {
    using namespace edge_plan;
    __shared__ uint32_t cnt[WINDOW_MAX];
    __shared__ uint32_t wave_totals[COUNT_WAVES];
    __shared__ uint32_t n_reported, reservation;
    const WorkItem it = work_item(blockIdx.x, n_passing, window);
    const uint32_t loser = losers[it.loser_slot];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t t = threadIdx.x; t < it.window_len; t += COUNT_TPB) cnt[t] = 0;
    if (threadIdx.x == 0) n_reported = 0;
    __syncthreads();
    for (uint64_t i = off[loser] + threadIdx.x, hi = off[loser + 1]; i < hi; i += COUNT_TPB) {
        const uint32_t w = winner[i];
        if (counts_in_window(w, loser, it.window_base, it.window_len)) atomicAdd(&cnt[w - it.window_base], 1u);
    }
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t t = threadIdx.x; t < it.window_len; t += COUNT_TPB) mine += reported(cnt[t], min_count) ? 1u : 0u;
    if (mine) atomicAdd(&n_reported, mine);
    __syncthreads();
    const uint32_t total = n_reported;
    if (total == 0) return;                                  // uniform: every lane read the same word
    if (threadIdx.x == 0) reservation = atomicAdd(cursor, total);
    uint32_t before = 0;                                     // reported entries of the tiles scanned so far
    for (uint32_t t0 = 0; t0 < it.window_len; t0 += COUNT_TPB) {
        const uint32_t t = t0 + threadIdx.x;
        const uint32_t c = t < it.window_len ? cnt[t] : 0u;
        const bool rep = t < it.window_len && reported(c, min_count);
        const unsigned long long ballot = __ballot(rep);
        if (lane == 0) wave_totals[wave] = (uint32_t)__popcll(ballot);
        __syncthreads();                                     // (the first one also publishes the reservation)
        uint32_t wt[COUNT_WAVES];
#pragma unroll
        for (uint32_t w = 0; w < COUNT_WAVES; w++) wt[w] = wave_totals[w];
        if (rep) {
            const uint32_t slot = reservation + before + slot_in_tile(wt, wave, below_lane(ballot, lane));
            if (slot < cap) edges[slot] = Edge{it.window_base + t, loser, c};
        }
        before += tile_total(wt);
        __syncthreads();                                     // everyone has read wave_totals before the next tile writes them
    }
}

}  // namespace
}  // namespace sylph

using namespace sylph;

extern "C" int sylph_db_reassign_edges(sylph_db* db, const uint64_t* genome_kmers, const uint64_t* kmer_off, int mem, const uint32_t* passing_gids,
                                       const double* passing_ani, uint32_t n_passing, uint32_t min_count, sylph_reassign_edge** out_edges,
                                       uint64_t* out_n) {
    return guarded([&] {
        SY_REQUIRE(db && kmer_off && out_edges && out_n, "null argument");
        *out_edges = nullptr;
        *out_n = 0;
        SY_REQUIRE(mem == SYLPH_MEM_HOST || mem == SYLPH_MEM_DEVICE, "bad mem kind %d", mem);
        SY_REQUIRE(db->world == 1, "this database is one shard of %u: the reassignment log needs the whole index", db->world);
        SY_REQUIRE(n_passing == 0 || (passing_gids && passing_ani), "null passing list");
        SY_REQUIRE(n_passing < 0xFFFFFFFFu, "too many passing genomes");
        for (uint32_t r = 0; r < n_passing; r++) SY_REQUIRE(kmer_off[r] <= kmer_off[r + 1], "kmer_off decreases at rank %u", r);
        const uint64_t n_q = kmer_off[n_passing] - kmer_off[0];
        SY_REQUIRE(n_q < (1ull << 32), "more than 2^32-1 k-mers in the passing genomes");
        SY_REQUIRE(n_q == 0 || genome_kmers, "null genome_kmers");
        sylph_ctx* ctx = db->ctx;
        std::lock_guard<std::mutex> lock(ctx->mu);
        DeviceGuard dg(ctx->device);
        const uint64_t G = db->n_genomes;
        std::vector<uint32_t> rank(std::max<uint64_t>(1, G), 0xFFFFFFFFu);
        for (uint32_t r = 0; r < n_passing; r++) {
            SY_REQUIRE(passing_gids[r] < G, "passing genome id %u out of range", passing_gids[r]);
            SY_REQUIRE(rank[passing_gids[r]] == 0xFFFFFFFFu, "genome %u listed twice", passing_gids[r]);
            rank[passing_gids[r]] = r;
        }
        if (n_passing < 2 || n_q == 0 || !db->kept.n_postings) return;   // nobody to lose to, nothing to look up
        const uint32_t window = std::min<uint32_t>(std::max<uint32_t>(1, ctx->reassign_edge_window), edge_plan::WINDOW_MAX);
        // offsets from 0 (the caller's may start anywhere), the losers with k-mers, the work list's size
        std::vector<uint64_t> off(n_passing + 1);
        for (uint32_t r = 0; r <= n_passing; r++) off[r] = kmer_off[r] - kmer_off[0];
        std::vector<uint32_t> losers(n_passing);
        const uint32_t n_losers = edge_plan::work_losers(off.data(), n_passing, losers.data());
        const uint64_t n_items = edge_plan::n_work_items(n_losers, n_passing, window);
        SY_REQUIRE(n_items < (1ull << 31), "too many (genome, window) items for the reassignment log: raise reassign_edge_window");
        // the winner table's two arrays (the database's own: the next reassignment pass uploads its own again); everything else is
        // this call's scratch — the result block and the query buffers of the probe entry points are not touched
        db->rank_of.reserve(rank.size() * 4);
        db->ani.reserve((size_t)n_passing * 8);
        ctx->h2d(db->rank_of.p, rank.data(), rank.size() * 4);
        ctx->h2d(db->ani.p, passing_ani, (size_t)n_passing * 8);
        DevBuf d_q(ctx), d_winner(ctx), d_off(ctx), d_losers(ctx), d_edges(ctx), d_cursor(ctx);
        const uint64_t* d_k = genome_kmers + kmer_off[0];
        if (mem == SYLPH_MEM_HOST) {
            d_q.reserve(n_q * 8);
            ctx->h2d(d_q.p, genome_kmers + kmer_off[0], n_q * 8);
            d_k = d_q.as<uint64_t>();
        }
        d_winner.reserve(n_q * 4);
        d_off.reserve(off.size() * 8);
        d_losers.reserve((size_t)n_losers * 4);
        d_cursor.reserve(4);
        ctx->h2d(d_off.p, off.data(), off.size() * 8);
        ctx->h2d(d_losers.p, losers.data(), (size_t)n_losers * 4);
        {
            ScopedKernelTimer t(ctx, "edge_winner");
            hipLaunchKernelGGL(edge_winner_kernel, dim3(std::min<uint32_t>(grid_for64(n_q, WINNER_TPB), WINNER_GRID)), dim3(WINNER_TPB), 0, ctx->stream, d_k,
                               (uint32_t)n_q, db->kept.view(), db->tracked.view(), db->tracked.n_postings ? 1 : 0, db->rank_of.as<uint32_t>(),
                               db->ani.as<double>(), d_winner.as<uint32_t>());
            SY_HIP(hipGetLastError());
        }
        uint64_t cap = edge_plan::first_capacity(edge_plan::edge_bound(off.data(), n_passing, min_count), n_passing);
        uint32_t n_edges = 0;
        for (int attempt = 0; attempt < 2 && cap; attempt++) {
            SY_REQUIRE(cap < (1ull << 32), "more than 2^32-1 edges in the reassignment log");
            d_edges.reserve(cap * sizeof(edge_plan::Edge));
            SY_HIP(hipMemsetAsync(d_cursor.p, 0, 4, ctx->stream));
            {
                ScopedKernelTimer t(ctx, "edge_count");
                hipLaunchKernelGGL(edge_count_kernel, dim3((uint32_t)n_items), dim3(edge_plan::COUNT_TPB), 0, ctx->stream, d_winner.as<uint32_t>(),
                                   d_off.as<uint64_t>(), d_losers.as<uint32_t>(), n_passing, window, min_count, d_edges.as<edge_plan::Edge>(), (uint32_t)cap,
                                   d_cursor.as<uint32_t>());
                SY_HIP(hipGetLastError());
            }
            ctx->read_back(&n_edges, d_cursor.p, 4);
            const uint64_t again = edge_plan::retry_capacity(n_edges, cap);
            if (!again) break;
            SY_REQUIRE(attempt == 0, "edge list overflow persisted");
            cap = again;
        }
        if (!ctx->pending.empty()) profile_collect(ctx);
        if (!cap || !n_edges) return;
        edge_plan::Edge* h = (edge_plan::Edge*)malloc((size_t)n_edges * sizeof(edge_plan::Edge));
        if (!h) throw std::bad_alloc();
        std::unique_ptr<edge_plan::Edge, decltype(&free)> hold(h, &free);
        ctx->d2h(h, d_edges.p, (size_t)n_edges * sizeof(edge_plan::Edge));
        *out_n = edge_plan::sort_and_merge(h, n_edges);
        *out_edges = reinterpret_cast<sylph_reassign_edge*>(hold.release());
    });
}
