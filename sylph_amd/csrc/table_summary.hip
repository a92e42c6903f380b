// table_summary.hip — K15: the integers --estimate-unknown reads off a sample's table (contain.rs:901-951 get_kmer_identity's two
// walks, :392-408's total), counted where the table lies.  table_summary_plan.h holds the arithmetic and the proof; this file is the
// three passes of a rung as kernels and the ladder queued on the context's stream without a host round trip: a later rung's kernels
// read the earlier rungs' verdicts from device memory and return at once.  The common case is three launches that work, three per
// further rung that do not, and one read-back of 160 bytes.
//
//   pass 1, pass 3   one lane per chunk, 64 chunks per workgroup of one wavefront.  The counts come in coalesced runs of TILE entries
//                    per chunk through an LDS tile (8.25 KB); a lane then walks its own row of the tile: LDS read, compare, add —
//                    four independent chains in pass 1 (a lower and an upper state for either parity), one in pass 3.  The sums
//                    leave a workgroup through a wave reduction and one atomic each.
//   pass 2           a single wavefront: the lanes load 64 chunk records at a time, every lane then goes through them in order (the
//                    control flow is uniform) and lane c keeps chunk c's start; an open chunk is walked again by the whole wavefront,
//                    64 coalesced counts per load, handed round by lane broadcasts.
#include <algorithm>

#include "common.h"
#include "device_common.h"

#include "table_summary.h"

namespace sylph {
namespace {

using namespace table_summary_plan;
static_assert(sizeof(Summary) == sizeof(sylph_table_summary_t) && sizeof(Summary) == 48, "the ABI's summary is the plan's");
static_assert(DECLINED == SYLPH_TABLE_SUMMARY_DECLINED && DECLINED_LADDER == SYLPH_TABLE_SUMMARY_DECLINED_LADDER &&
              DECLINED_SUM == SYLPH_TABLE_SUMMARY_DECLINED_SUM && DECLINED_SIZE == SYLPH_TABLE_SUMMARY_DECLINED_SIZE, "the ABI's flags are the plan's");
static_assert(GROUP == 64, "one wavefront per workgroup: the tile's barriers are a wavefront's own");

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t x) {
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    // 64 low halves sum to less than 2^38: two 32-bit sums of their 16-bit halves, and one of the high halves (mod 2^32, as the u64 is)
    const uint64_t a = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_sum(lo & 0xFFFFu), 63);
    const uint64_t b = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_sum(lo >> 16), 63);
    const uint64_t c = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_sum(hi), 63);
    return a + (b << 16) + (c << 32);
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_sum(x), 63); }

// lane `from`'s x, `from` the same in every lane: one v_readlane_b32
__device__ __forceinline__ uint32_t lane_value(uint32_t x, uint32_t from) { return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)from); }

// records[chunk] for every chunk of rung `rung`, and the table's three sums into states[rung]
__global__ __launch_bounds__(GROUP) void table_pass1_kernel(const uint32_t* __restrict__ counts, uint64_t n, const Ladder ladder, uint32_t rung,
                                                            RungState* __restrict__ states, ChunkRecord* __restrict__ records) {
    __shared__ uint32_t tile[TILE_WORDS];
    if (answered_before(states, ladder, rung)) return;
    const uint32_t cap = ladder.rung[rung].cap, chunk = ladder.rung[rung].chunk;
    const uint32_t lane = threadIdx.x, group = blockIdx.x, n_rounds = n_rounds_of(chunk);
    Walk1 w = walk1_begin(cap);
    Tally tally{0, 0, 0};
    for (uint32_t round = 0; round < n_rounds; round++) {
        stage_tile(counts, n, chunk, group, round, lane, tile, &tally);
        __syncthreads();
        walk1_tile(w, tile, lane, cap);
        __syncthreads();
    }
    const uint64_t c = (uint64_t)group * GROUP + lane;
    if (c < n_chunks_of(n, chunk)) records[c] = walk1_end(w);
    const uint64_t total = wave_sum_u64(tally.total);
    const uint32_t ones = wave_sum_u32(tally.num_1s), not_ones = wave_sum_u32(tally.num_not1s);
    if (lane == 0) {
        RungState* st = states + rung;
        atomicAdd((unsigned long long*)&st->total_counts, (unsigned long long)total);
        atomicAdd(&st->num_1s, ones);
        atomicAdd(&st->num_not1s, not_ones);
    }
}

// starts[chunk] for every chunk, and the rung's steps, open chunks and give-up: ONE wavefront
__global__ __launch_bounds__(GROUP) void table_pass2_kernel(const uint32_t* __restrict__ counts, uint64_t n, const Ladder ladder, uint32_t rung,
                                                            RungState* __restrict__ states, const ChunkRecord* __restrict__ records,
                                                            uint32_t* __restrict__ starts) {
    if (answered_before(states, ladder, rung)) return;
    const uint32_t cap = ladder.rung[rung].cap, chunk = ladder.rung[rung].chunk, lane = threadIdx.x;
    const uint64_t n_chunks = n_chunks_of(n, chunk);
    Pass2 p = pass2_begin();
    for (uint64_t base = 0; base < n_chunks; base += GROUP) {
        const uint64_t mine = base + lane;
        const ChunkRecord r = mine < n_chunks ? records[mine] : ChunkRecord{0, {OPEN, OPEN}};
        const uint32_t here = n_chunks - base < GROUP ? (uint32_t)(n_chunks - base) : GROUP;
        uint32_t my_start = 0;
        for (uint32_t c = 0; c < here; c++) {                        // (uniform: every lane walks the same records)
            const ChunkRecord rc{lane_value(r.steps, c), {lane_value(r.end[0], c), lane_value(r.end[1], c)}};
            const uint32_t start = pass2_chunk(p, rc, ladder.max_open, [&](uint32_t m) {
                const uint64_t lo = (base + c) * chunk, hi = lo + chunk < n ? lo + chunk : n;
                for (uint64_t at = lo; at < hi; at += GROUP) {
                    const uint32_t v = at + lane < hi ? counts[at + lane] : 0u;
                    for (uint32_t j = 0; j < GROUP; j++) m = rewalk_step(m, lane_value(v, j), cap);
                }
                return m;
            });
            if (c == lane) my_start = start;
        }
        if (mine < n_chunks) starts[mine] = my_start;
    }
    if (lane == 0) {
        RungState* st = states + rung;
        st->steps = (uint32_t)p.steps;
        st->open = p.open;
        st->gave_up = p.gave_up;
    }
}

// the sum of the states and their maximum into states[rung]
__global__ __launch_bounds__(GROUP) void table_pass3_kernel(const uint32_t* __restrict__ counts, uint64_t n, const Ladder ladder, uint32_t rung,
                                                            RungState* __restrict__ states, const uint32_t* __restrict__ starts) {
    __shared__ uint32_t tile[TILE_WORDS];
    if (answered_before(states, ladder, rung) || states[rung].gave_up) return;
    const uint32_t cap = ladder.rung[rung].cap, chunk = ladder.rung[rung].chunk;
    const uint32_t lane = threadIdx.x, group = blockIdx.x, n_rounds = n_rounds_of(chunk);
    const uint64_t c = (uint64_t)group * GROUP + lane;
    Walk3 w{0, c < n_chunks_of(n, chunk) ? starts[c] : 0u, 0};
    for (uint32_t round = 0; round < n_rounds; round++) {
        stage_tile(counts, n, chunk, group, round, lane, tile, nullptr);
        __syncthreads();
        walk3_tile(w, tile, lane, cap);
        __syncthreads();
    }
    const uint64_t sum = wave_sum_u64(w.sum);
    const uint32_t top = wave_max_u32(w.max);
    if (lane == 0) {
        RungState* st = states + rung;
        atomicAdd((unsigned long long*)&st->median_sum, (unsigned long long)sum);
        atomicMax(&st->max_state, top);
    }
}

}  // namespace

table_summary_plan::Ladder table_summary_ladder(const sylph_ctx* ctx) {
    Ladder l = default_ladder();
    struct Numbers { uint32_t n = 0, v[MAX_RUNGS] = {0, 0, 0, 0}; };
    auto from_env = [](const char* name) {
        Numbers x;
        const char* e = getenv(name);
        const int n = e ? parse_rung_numbers(e, x.v) : 0;
        SY_REQUIRE(n >= 0, "%s must be up to four numbers in [1, 2^30], comma-separated", name);
        x.n = (uint32_t)n;
        return x;
    };
    static const Numbers env_caps = from_env("SYLPH_HIP_TABLE_SUMMARY_CAPS"), env_chunks = from_env("SYLPH_HIP_TABLE_SUMMARY_CHUNK");
    Numbers caps = env_caps, chunks = env_chunks;
    if (ctx->table_summary_n_caps) { caps.n = ctx->table_summary_n_caps; memcpy(caps.v, ctx->table_summary_caps, sizeof(caps.v)); }
    if (ctx->table_summary_n_chunks) { chunks.n = ctx->table_summary_n_chunks; memcpy(chunks.v, ctx->table_summary_chunks, sizeof(chunks.v)); }
    if (caps.n) {
        l.n_rungs = caps.n;
        for (uint32_t r = 0; r < MAX_RUNGS; r++) l.rung[r].cap = r < caps.n ? caps.v[r] : 0;
    }
    // a chunk given alone holds for every rung; without one, a rung of caps given alone takes 16 entries per unit of its cap
    for (uint32_t r = 0; r < l.n_rungs; r++) {
        if (chunks.n) l.rung[r].chunk = chunks.v[r < chunks.n ? r : chunks.n - 1];
        else if (caps.n) l.rung[r].chunk = l.rung[r].cap <= (1u << 26) ? l.rung[r].cap * 16u : 1u << 30;
    }
    l.max_open = ctx->table_summary_max_open;
    return l;
}

// Device counts in, the summary out (table_summary.h); the caller holds ctx->mu.  Queues every rung on ctx->stream and reads the
// rungs' states back: one synchronisation.
void table_summary_device(sylph_ctx* ctx, const uint32_t* counts, uint64_t n, table_summary_plan::Summary& out) {
    const Ladder ladder = table_summary_ladder(ctx);
    SY_REQUIRE(ladder_ok(ladder), "table_summary: the caps must ascend within [%u, %u], with a chunk of at least one entry each", CAP_MIN, CAP_MAX);
    RungState states[MAX_RUNGS] = {};
    if (n == 0 || n >= MAX_ENTRIES) { out = finish(states, ladder, n); return; }
    uint64_t most_chunks = 0;
    for (uint32_t r = 0; r < ladder.n_rungs; r++) most_chunks = std::max(most_chunks, n_chunks_of(n, ladder.rung[r].chunk));
    // scratch: the rungs' states, then one rung's records and starts (a rung is done with them before the next one's kernels run)
    DevBuf work(ctx);
    const size_t a_states = 0, a_records = a_states + sizeof(states), a_starts = a_records + (size_t)most_chunks * sizeof(ChunkRecord),
                 a_end = a_starts + (size_t)most_chunks * 4;
    work.reserve(a_end);
    char* w = work.as<char>();
    RungState* d_states = (RungState*)(w + a_states);
    ChunkRecord* records = (ChunkRecord*)(w + a_records);
    uint32_t* starts = (uint32_t*)(w + a_starts);
    {
        ScopedKernelTimer t(ctx, "table_summary");
        SY_HIP(hipMemsetAsync(d_states, 0, sizeof(states), ctx->stream));
        for (uint32_t r = 0; r < ladder.n_rungs; r++) {
            const uint32_t grid = n_groups_of(n, ladder.rung[r].chunk);
            hipLaunchKernelGGL(table_pass1_kernel, dim3(grid), dim3(GROUP), 0, ctx->stream, counts, n, ladder, r, d_states, records);
            hipLaunchKernelGGL(table_pass2_kernel, dim3(1), dim3(GROUP), 0, ctx->stream, counts, n, ladder, r, d_states, (const ChunkRecord*)records, starts);
            hipLaunchKernelGGL(table_pass3_kernel, dim3(grid), dim3(GROUP), 0, ctx->stream, counts, n, ladder, r, d_states, (const uint32_t*)starts);
            SY_HIP(hipGetLastError());
        }
    }
    ctx->read_back(states, d_states, sizeof(states));
    out = finish(states, ladder, n);
}

}  // namespace sylph

using namespace sylph;

extern "C" {

int sylph_table_summary(sylph_ctx* ctx, const uint32_t* counts, uint64_t n, int mem, sylph_table_summary_t* out) {
    return guarded([&] {
        SY_REQUIRE(ctx && out, "null argument");
        memset(out, 0, sizeof(*out));
        SY_REQUIRE(counts || n == 0, "null argument");
        SY_REQUIRE(mem == SYLPH_MEM_HOST || mem == SYLPH_MEM_DEVICE || mem == SYLPH_MEM_HOST_PINNED, "bad mem");
        SY_REQUIRE(mem != SYLPH_MEM_DEVICE || (uintptr_t)counts % 4 == 0, "sylph_table_summary: device counts not aligned to their width");
        std::lock_guard<std::mutex> lock(ctx->mu);
        DeviceGuard dg(ctx->device);
        DevBuf d_counts(ctx);
        const uint32_t* dc = counts;
        if (mem != SYLPH_MEM_DEVICE && n && n < table_summary_plan::MAX_ENTRIES) {
            d_counts.reserve((size_t)n * 4);
            ctx->h2d(d_counts.p, counts, (size_t)n * 4);
            dc = d_counts.as<uint32_t>();
        }
        table_summary_plan::Summary s;
        table_summary_device(ctx, dc, n, s);
        memcpy(out, &s, sizeof(s));
    });
}

}  // extern "C"
