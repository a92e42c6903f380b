// table_summary.h — the device-to-summary entry of table_summary.hip, for the callers inside the library
#pragma once
#include "common.h"

#include "table_summary_plan.h"

namespace sylph {

// "c0,c1,.." -> vals[0 .. n): up to four numbers in [1, 2^30]; -1: anything else.  "" gives 0
inline int parse_rung_numbers(const char* value, uint32_t* vals) {
    int n = 0;
    for (const char* at = value; *at;) {
        char* end = nullptr;
        const unsigned long long v = strtoull(at, &end, 10);
        if (end == at || (*end != ',' && *end) || n >= (int)table_summary_plan::MAX_RUNGS || v < 1 || v > (1ull << 30)) return -1;
        vals[n++] = (uint32_t)v;
        at = *end ? end + 1 : end;
    }
    return n;
}
// the ladder the context's options ask for ("table_summary_caps" / "table_summary_chunk" / "table_summary_max_open"), else the
// environment's (SYLPH_HIP_TABLE_SUMMARY_CAPS / SYLPH_HIP_TABLE_SUMMARY_CHUNK, same spelling: for whole commands), else the default
table_summary_plan::Ladder table_summary_ladder(const sylph_ctx* ctx);
// counts[0 .. n) in device memory -> the summary (declined: see its flags); the caller holds ctx->mu
void table_summary_device(sylph_ctx* ctx, const uint32_t* counts, uint64_t n, table_summary_plan::Summary& out);

}  // namespace sylph
