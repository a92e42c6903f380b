// row_stats.h — the device-to-device entry of row_stats.hip, for the callers inside the library
#pragma once
#include "common.h"

#include "row_stats_plan.h"

namespace sylph {

// the candidates of one call, in device memory: rows[0 .. n), cov_off[0 .. n] and covs[0 .. n_vals) at the width that came in; and
// sample_off[s] = the input's cov_off[s * kmers_period], s = 0 .. n_samples = n_rows / kmers_period (n_rows != 0)
struct RowStatsResult {
    DevBuf rows, cov_off, covs, sample_off;
    uint32_t n = 0, n_samples = 0;
    uint64_t n_vals = 0;
    explicit RowStatsResult(sylph_ctx* ctx) : rows(ctx), cov_off(ctx), covs(ctx), sample_off(ctx) {}
};
void row_stats_device(sylph_ctx* ctx, const void* covs, uint32_t width, const uint64_t* cov_off, const uint32_t* row_kmers, uint32_t kmers_period,
                      uint32_t n_rows, uint64_t max_vals, const row_stats_plan::Filter& f, RowStatsResult& out);

}  // namespace sylph
