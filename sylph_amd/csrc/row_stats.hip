// row_stats.hip — the integer half of the statistics head (contain.rs:657-690) on the device: every non-empty coverage row of a
// result block reduced to the few integers stats_head reads off it (row_stats_plan.h RowSummary), the rows that cannot reach the
// ANI cut dropped (surely_rejected: conservative, in the index domain), and the CANDIDATES gathered in ascending row order — their
// summaries, their coverage values side by side at the width they came in, and the offsets of each candidate's values.  The exact
// decision, in f64, stays with the host (host/inference.cpp stats_head_from_summary): what comes back are counts.
//
// One wavefront per row, four rows per workgroup, no LDS: a row is ascending, so its runs are found by a compare with the left
// neighbour and a ballot, and the mode by a wave maximum over (run length, value).  Nearly every row is a handful of values — one
// chunk; a present genome's row is thousands — a loop over 64-value chunks that carries the open run.  The split is
// row_stats_plan.h's, lane by lane.  A second launch, behind two exclusive sums over the rows, copies what the candidates keep.
#include <algorithm>

#include "common.h"
#include "device_common.h"

#include "row_stats.h"

namespace sylph {
namespace {

using namespace row_stats_plan;
static_assert(sizeof(Filter) == sizeof(sylph_row_filter) && sizeof(Filter) == 152, "the ABI's filter is the plan's");
static_assert(sizeof(RowSummary) == sizeof(sylph_row_summary) && sizeof(RowSummary) == 36, "the ABI's summary is the plan's");
static_assert(CUT_ENTRIES == SYLPH_ROW_CUT_ENTRIES && CUT_NONE == SYLPH_ROW_CUT_NONE && CHUNK == 64, "the ABI's table is the plan's");

constexpr int ROWS_TPB = 256, ROWS_WAVES = ROWS_TPB / 64;

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_sum(x), 63); }

// summaries[row], flag[row] (1 = candidate) and cand_len[row] (its values, 0 for a row that is dropped) for every row; the genome of
// row r has row_kmers[r % kmers_period] k-mers (a result block holds the rows of several samples, one after the other)
template <class T>
__global__ __launch_bounds__(ROWS_TPB) void row_stats_kernel(const T* __restrict__ covs, const uint64_t* __restrict__ cov_off,
                                                             const uint32_t* __restrict__ row_kmers, uint32_t kmers_period, uint32_t n_rows, const Filter f,
                                                             RowSummary* __restrict__ summaries, uint32_t* __restrict__ flag,
                                                             uint64_t* __restrict__ cand_len) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * ROWS_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= n_rows) return;                                               // (the whole wavefront)
    const uint64_t lo = cov_off[row];
    const uint32_t len = (uint32_t)(cov_off[row + 1] - lo);                  // (the host entry refuses rows of 2^32 values)
    if (len == 0) {
        if (lane == 0) { flag[row] = 0u; cand_len[row] = 0ull; }
        return;
    }
    const T* __restrict__ r = covs + lo;
    const uint32_t median = (uint32_t)r[len / 2];
    const uint32_t limit = keep_limit(median, f.cut);
    Carry c = carry_begin();
    uint32_t v = 0;
    bool kept = false;                                                       // (of the last chunk walked: next_count of a short row)
    for (uint64_t base = 0;; base += CHUNK) {
        const uint64_t i = base + lane;
        v = i < len ? (uint32_t)r[i] : 0u;
        // the kept lanes are the chunk's prefix up to the first value beyond the limit, whatever lies behind it
        const uint64_t within = __ballot(lane_kept(i, len, v, limit));
        const uint32_t n_kept = ~within ? (uint32_t)__ffsll((long long)~within) - 1u : CHUNK;
        kept = lane < n_kept;
        const uint32_t left = (uint32_t)__shfl_up((int)v, 1);
        const uint64_t starts = __ballot(lane_starts_run(lane, kept, v, left));
        const bool more = chunk_has_more(n_kept, base, len);
        close_stale_run(c, n_kept, (uint32_t)__builtin_amdgcn_readfirstlane((int)v));
        const uint32_t run_len = kept ? run_len_up_to(lane, starts, v, c) : 0u;
        const bool closes = lane_closes_run(lane, n_kept, starts, more);
        const uint32_t bid_len = closes ? run_len : 0u;
        const uint32_t n_closed = (uint32_t)__popcll(__ballot(closes));
        const uint32_t best_len = wave_max_u32(bid_len);
        const uint32_t best_value = wave_max_u32(closes && bid_len == best_len ? v : 0u);
        const uint32_t chunk_sum = wave_sum_u32(kept ? v : 0u);
        const int last = n_kept ? (int)n_kept - 1 : 0;
        fold_chunk(c, n_kept, chunk_sum, n_closed, best_len, best_value, more, (uint32_t)__shfl((int)v, last), (uint32_t)__shfl((int)run_len, last));
        if (!more) break;
    }
    uint32_t next_count;
    if (len <= CHUNK) next_count = (uint32_t)__popcll(__ballot(kept && c.mode != 0xFFFFFFFFu && v == c.mode + 1u));
    else next_count = next_count_by_search([&](uint32_t i) { return (uint32_t)r[i]; }, c.keep, c.mode);
    RowSummary s = summary_of_carry(c, len, median, next_count);
    s.row = row;
    const bool candidate = !surely_rejected(s, len, row_kmers[row % kmers_period], f);
    if (lane == 0) {
        if (candidate) summaries[row] = s;
        flag[row] = candidate ? 1u : 0u;
        cand_len[row] = candidate ? (uint64_t)len : 0ull;
    }
}

// candidate j = the j-th flagged row: its summary to out_rows[j], its values to out_covs[out_off[j] ..); the wavefront of the last row
// also leaves the totals (totals[0] = candidates, totals[1] = their values) and closes out_off
template <class T>
__global__ __launch_bounds__(ROWS_TPB) void row_gather_kernel(const T* __restrict__ covs, const uint64_t* __restrict__ cov_off, uint32_t n_rows,
                                                              const RowSummary* __restrict__ summaries, const uint32_t* __restrict__ flag,
                                                              const uint32_t* __restrict__ flag_pos, const uint64_t* __restrict__ cand_len,
                                                              const uint64_t* __restrict__ len_pos, RowSummary* __restrict__ out_rows,
                                                              uint64_t* __restrict__ out_off, T* __restrict__ out_covs, uint64_t* __restrict__ totals) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * ROWS_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= n_rows) return;
    const uint32_t pos = flag_pos[row];
    const uint64_t at = len_pos[row];
    if (row == n_rows - 1 && lane == 0) {
        const uint64_t n = (uint64_t)pos + flag[row], n_vals = at + cand_len[row];
        totals[0] = n;
        totals[1] = n_vals;
        out_off[n] = n_vals;
    }
    if (!flag[row]) return;
    const uint64_t lo = cov_off[row];
    const uint32_t len = (uint32_t)(cov_off[row + 1] - lo);
    if (lane == 0) { out_rows[pos] = summaries[row]; out_off[pos] = at; }
    for (uint32_t i = lane; i < len; i += 64u) out_covs[at + i] = covs[lo + i];
}

// sample_off[s] = cov_off[s * period], s = 0 .. n_samples: where the values of every sample of a result block begin
__global__ __launch_bounds__(64) void sample_offsets_kernel(const uint64_t* __restrict__ cov_off, uint32_t period, uint32_t n_samples, uint64_t* __restrict__ sample_off) {
    const uint32_t s = blockIdx.x * 64u + threadIdx.x;
    if (s <= n_samples) sample_off[s] = cov_off[(uint64_t)s * period];
}

template <class T>
void launch_row_stats(sylph_ctx* ctx, const void* covs, const uint64_t* cov_off, const uint32_t* row_kmers, uint32_t kmers_period, uint32_t n_rows, const Filter& f,
                      RowSummary* summaries, uint32_t* flag, uint32_t* flag_pos, uint64_t* cand_len, uint64_t* len_pos, RowStatsResult& out,
                      uint64_t* totals) {
    const uint32_t grid = (n_rows + ROWS_WAVES - 1) / ROWS_WAVES;
    hipLaunchKernelGGL(row_stats_kernel<T>, dim3(grid), dim3(ROWS_TPB), 0, ctx->stream, (const T*)covs, cov_off, row_kmers, kmers_period, n_rows, f, summaries, flag,
                       cand_len);
    exclusive_sum_u32(ctx, flag, flag_pos, n_rows);
    exclusive_sum_u64(ctx, cand_len, len_pos, n_rows);
    hipLaunchKernelGGL(row_gather_kernel<T>, dim3(grid), dim3(ROWS_TPB), 0, ctx->stream, (const T*)covs, cov_off, n_rows, summaries, flag, flag_pos,
                       cand_len, len_pos, out.rows.as<RowSummary>(), out.cov_off.as<uint64_t>(), out.covs.as<T>(), totals);
    SY_HIP(hipGetLastError());
}

}  // namespace

// Device arrays in, device arrays out (row_stats.h); the caller holds ctx->mu.  max_vals: an upper bound of the values of all rows
// (what a gather of every row would take); kmers_period: entries of row_kmers, row r reads entry r % kmers_period.  Queues everything on ctx->stream and reads the two totals back: one synchronisation.
void row_stats_device(sylph_ctx* ctx, const void* covs, uint32_t width, const uint64_t* cov_off, const uint32_t* row_kmers, uint32_t kmers_period,
                      uint32_t n_rows, uint64_t max_vals, const row_stats_plan::Filter& f, RowStatsResult& out) {
    out.n = 0;
    out.n_vals = 0;
    out.cov_off.reserve(((size_t)n_rows + 1) * 8);
    if (!n_rows) {
        SY_HIP(hipMemsetAsync(out.cov_off.p, 0, 8, ctx->stream));
        return;
    }
    out.rows.reserve((size_t)n_rows * sizeof(RowSummary));
    out.n_samples = n_rows / kmers_period;
    out.sample_off.reserve(((size_t)out.n_samples + 1) * 8);
    out.covs.reserve((size_t)max_vals * width + 16);
    // scratch: the rows' summaries, flags and lengths with their exclusive sums, and the two totals
    DevBuf work(ctx);
    const size_t a_sum = 0, a_len = a_sum + (((size_t)n_rows * sizeof(RowSummary) + 7) & ~(size_t)7), a_lpos = a_len + (size_t)n_rows * 8,
                 a_tot = a_lpos + (size_t)n_rows * 8, a_flag = a_tot + 16, a_fpos = a_flag + (size_t)n_rows * 4, a_end = a_fpos + (size_t)n_rows * 4;
    work.reserve(a_end);
    char* w = work.as<char>();
    uint64_t* totals = (uint64_t*)(w + a_tot);
    {
        ScopedKernelTimer t(ctx, "row_stats");
        auto go = [&](auto tag) {
            using T = decltype(tag);
            launch_row_stats<T>(ctx, covs, cov_off, row_kmers, kmers_period, n_rows, f, (RowSummary*)(w + a_sum), (uint32_t*)(w + a_flag), (uint32_t*)(w + a_fpos),
                                (uint64_t*)(w + a_len), (uint64_t*)(w + a_lpos), out, totals);
        };
        if (width == 4) go(uint32_t{});
        else if (width == 2) go(uint16_t{});
        else go(uint8_t{});
        hipLaunchKernelGGL(sample_offsets_kernel, dim3(out.n_samples / 64 + 1), dim3(64), 0, ctx->stream, cov_off, kmers_period, out.n_samples,
                           out.sample_off.as<uint64_t>());
        SY_HIP(hipGetLastError());
    }
    uint64_t tot[2];
    ctx->read_back(tot, totals, 16);
    out.n = (uint32_t)tot[0];
    out.n_vals = tot[1];
}

}  // namespace sylph

using namespace sylph;

extern "C" {

int sylph_row_summaries(sylph_ctx* ctx, const void* covs, uint32_t cov_width, const uint64_t* cov_off, const uint32_t* row_kmers, uint32_t n_rows,
                        int mem, const sylph_row_filter* filter, sylph_row_summary** rows, uint32_t* n, uint64_t** row_cov_off, void** row_covs) {
    return guarded([&] {
        SY_REQUIRE(ctx, "null context");
        SY_REQUIRE(rows && n && row_cov_off && row_covs, "null argument");
        *rows = nullptr; *n = 0; *row_cov_off = nullptr; *row_covs = nullptr;
        SY_REQUIRE(filter, "sylph_row_summaries: null filter");
        SY_REQUIRE(filter->struct_size == sizeof(sylph_row_filter), "sylph_row_summaries: filter of %u bytes, this library's has %zu", filter->struct_size,
                   sizeof(sylph_row_filter));
        SY_REQUIRE(cov_width == 1 || cov_width == 2 || cov_width == 4, "sylph_row_summaries: coverage values of %u bytes", cov_width);
        SY_REQUIRE(mem == SYLPH_MEM_HOST || mem == SYLPH_MEM_DEVICE || mem == SYLPH_MEM_HOST_PINNED, "bad mem");
        SY_REQUIRE(cov_off && (row_kmers || !n_rows), "null argument");
        for (uint32_t i = 0; i < n_rows; i++) {
            SY_REQUIRE(cov_off[i] <= cov_off[i + 1], "sylph_row_summaries: cov_off decreases at row %u", i);
            const uint64_t len = cov_off[i + 1] - cov_off[i];
            SY_REQUIRE(len <= row_kmers[i], "sylph_row_summaries: row %u has %llu values, its genome %u k-mers", i, (unsigned long long)len, row_kmers[i]);
        }
        const uint64_t first = cov_off[0], n_vals = cov_off[n_rows] - first;
        SY_REQUIRE(covs || n_vals == 0, "null argument");
        const bool device_covs = mem == SYLPH_MEM_DEVICE;
        SY_REQUIRE(!device_covs || (uintptr_t)covs % cov_width == 0, "sylph_row_summaries: device values not aligned to their width");
        Filter f;
        memcpy(&f, filter, sizeof(f));
        std::lock_guard<std::mutex> lock(ctx->mu);
        DeviceGuard dg(ctx->device);
        // host values travel from the first row's to the last row's, and the offsets count from there
        std::vector<uint64_t> off(cov_off, cov_off + n_rows + 1);
        if (!device_covs) for (auto& o : off) o -= first;
        DevBuf d_off(ctx), d_kmers(ctx), d_covs(ctx);
        d_off.reserve(off.size() * 8);
        ctx->h2d(d_off.p, off.data(), off.size() * 8);
        d_kmers.reserve((size_t)n_rows * 4 + 4);
        ctx->h2d(d_kmers.p, row_kmers, (size_t)n_rows * 4);
        const void* cv = covs;
        if (!device_covs) {
            d_covs.reserve((size_t)n_vals * cov_width + 16);
            ctx->h2d(d_covs.p, (const uint8_t*)covs + first * cov_width, (size_t)n_vals * cov_width);
            cv = d_covs.p;
        }
        RowStatsResult res(ctx);
        row_stats_device(ctx, cv, cov_width, d_off.as<uint64_t>(), d_kmers.as<uint32_t>(), n_rows, n_rows, n_vals, f, res);
        auto* h_off = (uint64_t*)malloc(((size_t)res.n + 1) * 8);
        auto* h_rows = res.n ? (sylph_row_summary*)malloc((size_t)res.n * sizeof(sylph_row_summary)) : nullptr;
        void* h_covs = res.n_vals ? malloc((size_t)res.n_vals * cov_width) : nullptr;
        if (!h_off || (res.n && !h_rows) || (res.n_vals && !h_covs)) { free(h_off); free(h_rows); free(h_covs); throw std::bad_alloc(); }
        try {
            ctx->d2h(h_off, res.cov_off.p, ((size_t)res.n + 1) * 8);
            if (res.n) ctx->d2h(h_rows, res.rows.p, (size_t)res.n * sizeof(sylph_row_summary));
            if (res.n_vals) ctx->d2h(h_covs, res.covs.p, (size_t)res.n_vals * cov_width);
        } catch (...) { free(h_off); free(h_rows); free(h_covs); throw; }
        *rows = h_rows; *n = res.n; *row_cov_off = h_off; *row_covs = h_covs;
    });
}

}  // extern "C"
