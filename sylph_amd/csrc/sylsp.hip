// sylsp.hip — a pre-sketched sample's table on the device: the packed 12-byte entries of a .sylsp file in, k-mers and counts as
// two arrays out (sylph_table_from_entries).  The reference rebuilds a hash map from the file (types.rs:117-129) and the host
// road here copies, sorts and deduplicates 1.9 M pairs on one thread (read_sylsp); on the device the file's bytes travel as they
// are and one kernel unpacks them — and finds out on the way whether the keys ascend strictly, which is the case for every file
// this project writes: then the unpacked arrays ARE the table.  Otherwise: stable radix sort, last-of-run flags, scan, compaction.
// The arithmetic (tile window, lane's dwords, order rule, keep rule) is sylsp_plan.h, tested on the CPU.
#include <memory>

#include "sylsp_table.h"
#include "sylsp_plan.h"

using namespace sylph;
namespace sp = sylph::sylsp_plan;

namespace {

// result[0]: 1 when some entry breaks the order; result[1]: entries of the table (n here; the compaction kernel's total on the
// general road) — the two travel back in one read.
// One workgroup = one tile: the lanes load the tile's 16-byte-aligned window (coalesced 16-byte loads; the window may reach up to
// 12 bytes in front of and behind the tile: the neighbouring tiles' dwords, or the stream's margins) into LDS, then every lane
// takes its entry's three dwords from there.  Bounded by the arguments: no loop, no wait on another workgroup.
__global__ __launch_bounds__(sp::TILE) void sylsp_unpack_kernel(const uint32_t* __restrict__ base, uint32_t n, uint32_t phase,
                                                                uint64_t* __restrict__ kmers, uint32_t* __restrict__ counts,
                                                                uint32_t* __restrict__ result) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[sp::LDS_DWORDS];
    const uint32_t tile = blockIdx.x, lane = threadIdx.x;
    const sp::TileWindow w = sp::tile_window(tile, n, phase);
    if (lane < w.n_vecs) {
        const uint4 v = *reinterpret_cast<const uint4*>(base + (w.first_dword + 4 * (int64_t)lane));
        *reinterpret_cast<uint4*>(&lds[4 * lane]) = v;
    }
    __syncthreads();
    bool breaks = false;
    if (lane < sp::tile_entries(tile, n)) {
        const uint32_t at = sp::lane_lds_dword(lane, phase);
        const sp::Entry e = sp::entry_from_words(lds[at], lds[at + 1], lds[at + 2]);
        const uint32_t i = tile * sp::TILE + lane;
        kmers[i] = e.kmer;
        counts[i] = e.count;
        uint64_t prev = 0;
        if (lane) {
            prev = sp::key_from_words(lds[at - sp::ENTRY_DWORDS], lds[at - sp::ENTRY_DWORDS + 1]);
        } else if (i) {                          // the previous tile's last entry, from the input
            const uint64_t d = sp::prev_key_dword(i);
            prev = sp::key_from_words(base[d], base[d + 1]);
        }
        breaks = sp::breaks_order(i, prev, e.kmer);
        if (i == 0) result[1] = n;
    }
    // one atomic per wavefront at the most, and none once the bit is seen set: 30,000 wavefronts of a shuffled 1.9 M table ORing
    // into the one word made this kernel 0.34 ms; with the read in front 0.05 - 0.11 ms (ascending: 0.011; profiles/sylsp_pipeline.txt)
    if (__any(breaks) && (lane & 63u) == 0 && __hip_atomic_load(&result[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicOr(&result[0], 1u);
}

__global__ __launch_bounds__(256) void sylsp_last_of_run_kernel(const uint64_t* __restrict__ sorted, uint32_t n, uint32_t* __restrict__ keep) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    keep[i] = sp::last_of_run(i, n, sorted[i], i + 1 < n ? sorted[i + 1] : 0) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void sylsp_compact_kernel(const uint64_t* __restrict__ sorted, const uint32_t* __restrict__ sorted_counts,
                                                            const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos, uint32_t n,
                                                            uint64_t* __restrict__ kmers, uint32_t* __restrict__ counts, uint32_t* __restrict__ result) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (keep[i]) {                               // pos[i] <= i < n: inside the arrays of n entries
        kmers[pos[i]] = sorted[i];
        counts[pos[i]] = sorted_counts[i];
    }
    if (i == n - 1) result[1] = pos[i] + keep[i];
}

struct TableDeleter { void operator()(sylph_table* t) const { sylph_table_destroy(t); } };

}  // namespace

sylph_table* sylph::table_from_entries_impl(sylph_ctx* ctx, const void* entries, uint64_t n, int mem) {
    SY_REQUIRE(ctx, "null ctx");
    SY_REQUIRE(n < sp::MAX_ENTRIES, "sylph_table_from_entries: %llu entries, the limit is 2^31 - 1", (unsigned long long)n);
    SY_REQUIRE(entries || n == 0, "null entries");
    SY_REQUIRE(mem == SYLPH_MEM_HOST || mem == SYLPH_MEM_HOST_PINNED || mem == SYLPH_MEM_DEVICE, "bad mem %d", mem);
    SY_REQUIRE(mem != SYLPH_MEM_DEVICE || n == 0 || ((uintptr_t)entries & 3u) == 0, "sylph_table_from_entries: device entries must be 4-byte aligned");
    std::unique_ptr<sylph_table, TableDeleter> t(new sylph_table());      // (declared before the lock: its deleter takes ctx->mu itself)
    t->ctx = t->kmers.ctx = t->counts.ctx = ctx;
    ctx->refs++;                                 // sylph_table_destroy gives it back
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard dg(ctx->device);
    // every buffer of BOTH roads before anything is copied or launched: no room -> SYLPH_ERR_NOMEM with nothing touched.  (The sort
    // road's four come out of the context's pool and go back at the end of the call: an ascending table pays two pool look-ups for
    // them.  Only rocPRIM's own temporary storage, sized by rocPRIM inside the sort, is found when the order flag asks for it.)
    DevBuf staged(ctx), result(ctx), sorted(ctx), sorted_counts(ctx), keep(ctx), pos(ctx);
    t->kmers.alloc(n * 8 + 64);
    t->counts.alloc(n * 4 + 64);
    result.alloc(64);
    if (n && mem != SYLPH_MEM_DEVICE) staged.alloc(n * sp::ENTRY_BYTES + 2 * sp::MARGIN_BYTES);
    if (n > 1) {
        sorted.alloc(n * 8);
        sorted_counts.alloc(n * 4);
        keep.alloc(n * 4);
        pos.alloc(n * 4);
    }
    if (n == 0) return t.release();
    const uint32_t* base = (const uint32_t*)entries;
    if (mem != SYLPH_MEM_DEVICE) {               // host entries at any alignment: copied behind a margin, 16-byte aligned (phase 0)
        ctx->h2d(staged.as<char>() + sp::MARGIN_BYTES, entries, n * sp::ENTRY_BYTES);
        base = (const uint32_t*)(staged.as<char>() + sp::MARGIN_BYTES);
    }
    SY_HIP(hipMemsetAsync(result.p, 0, 8, ctx->stream));
    {
        ScopedKernelTimer timer(ctx, "sylsp");
        hipLaunchKernelGGL(sylsp_unpack_kernel, dim3(sp::n_tiles(n)), dim3(sp::TILE), 0, ctx->stream, base, (uint32_t)n, sp::base_phase((uint64_t)(uintptr_t)base),
                           t->kmers.as<uint64_t>(), t->counts.as<uint32_t>(), result.as<uint32_t>());
        SY_HIP(hipGetLastError());
    }
    uint32_t back[2] = {0, 0};
    ctx->read_back(back, result.p, 8);
    if (back[0]) {                               // the general road: stable sort by all 64 key bits, keep the last of every run
        sort_pairs_u64_u32(ctx, t->kmers.as<uint64_t>(), sorted.as<uint64_t>(), t->counts.as<uint32_t>(), sorted_counts.as<uint32_t>(), n, 0, 64);
        const uint32_t grid = grid_for64(n);
        {
            ScopedKernelTimer timer(ctx, "sylsp_dedup");
            hipLaunchKernelGGL(sylsp_last_of_run_kernel, dim3(grid), dim3(256), 0, ctx->stream, sorted.as<uint64_t>(), (uint32_t)n, keep.as<uint32_t>());
            SY_HIP(hipGetLastError());
            exclusive_sum_u32(ctx, keep.as<uint32_t>(), pos.as<uint32_t>(), n);
            hipLaunchKernelGGL(sylsp_compact_kernel, dim3(grid), dim3(256), 0, ctx->stream, sorted.as<uint64_t>(), sorted_counts.as<uint32_t>(),
                               keep.as<uint32_t>(), pos.as<uint32_t>(), (uint32_t)n, t->kmers.as<uint64_t>(), t->counts.as<uint32_t>(), result.as<uint32_t>());
            SY_HIP(hipGetLastError());
        }
        ctx->read_back(back, result.p, 8);
        t->was_ascending = 0;
    }
    t->n = back[1];
    return t.release();
}

extern "C" {

int sylph_table_from_entries(sylph_ctx* ctx, const void* entries, uint64_t n_entries, int mem, sylph_table** out) {
    return guarded([&] {
        SY_REQUIRE(out, "null argument");
        *out = nullptr;
        *out = table_from_entries_impl(ctx, entries, n_entries, mem);
    });
}

int sylph_table_view(const sylph_table* t, const uint64_t** dev_kmers, const uint32_t** dev_counts, uint64_t* n, int* was_ascending) {
    return guarded([&] {
        SY_REQUIRE(t, "null argument");
        if (dev_kmers) *dev_kmers = t->kmers.as<uint64_t>();
        if (dev_counts) *dev_counts = t->counts.as<uint32_t>();
        if (n) *n = t->n;
        if (was_ascending) *was_ascending = t->was_ascending;
    });
}

void sylph_table_destroy(sylph_table* t) {
    if (!t) return;
    sylph_ctx* ctx = t->ctx;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        t->kmers.release();                      // (back to the context's pool: everything that read them ran on, or was waited for by, its stream)
        t->counts.release();
    }
    delete t;
    ctx_unref(ctx);
}

}  // extern "C"
