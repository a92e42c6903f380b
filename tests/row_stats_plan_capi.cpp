// C entry points over sylph_amd/csrc/row_stats_plan.h for tests/test_row_stats_plan.py (ctypes) and tests/row_stats_sanitize_main.cpp:
// the sequential summary, the conservative reject, and rs_replay — one wavefront of row_stats.hip replayed on the host, chunk by chunk
// and lane by lane, with the very functions the kernel calls; what is a ballot, a shuffle or a wave reduction on the device is a
// loop over the 64 lanes here.  Every load of the replay is checked against the row's length.
#include <cstdint>
#include <cstring>

#include "../sylph_amd/csrc/row_stats_plan.h"

using namespace sylph::row_stats_plan;

namespace {

template <class T>
RowSummary replay_row(const T* r, uint32_t len, const uint32_t* cut, int* err) {
    auto load = [&](uint64_t i) -> uint32_t {
        if (i >= len) { *err = 1; return 0; }
        return (uint32_t)r[i];
    };
    const uint32_t median = load(len / 2);
    const uint32_t limit = keep_limit(median, cut);
    Carry c = carry_begin();
    uint32_t v[CHUNK];
    bool kept[CHUNK];
    for (uint64_t base = 0;; base += CHUNK) {
        uint64_t within = 0;
        for (uint32_t lane = 0; lane < CHUNK; lane++) {
            const uint64_t i = base + lane;
            v[lane] = i < len ? load(i) : 0u;
            if (lane_kept(i, len, v[lane], limit)) within |= 1ull << lane;
        }
        const uint32_t n_kept = ~within ? (uint32_t)__builtin_ctzll(~within) : CHUNK;
        uint64_t starts = 0;
        for (uint32_t lane = 0; lane < CHUNK; lane++) {
            kept[lane] = lane < n_kept;
            if (lane_starts_run(lane, kept[lane], v[lane], lane ? v[lane - 1] : v[0])) starts |= 1ull << lane;
        }
        const bool more = chunk_has_more(n_kept, base, len);
        close_stale_run(c, n_kept, v[0]);
        uint32_t run_len[CHUNK], bid_len[CHUNK], n_closed = 0, best_len = 0, best_value = 0, chunk_sum = 0;
        bool closes[CHUNK];
        for (uint32_t lane = 0; lane < CHUNK; lane++) {
            run_len[lane] = kept[lane] ? run_len_up_to(lane, starts, v[lane], c) : 0u;
            closes[lane] = lane_closes_run(lane, n_kept, starts, more);
            bid_len[lane] = closes[lane] ? run_len[lane] : 0u;
            n_closed += closes[lane];
            if (bid_len[lane] > best_len) best_len = bid_len[lane];
            chunk_sum += kept[lane] ? v[lane] : 0u;
        }
        for (uint32_t lane = 0; lane < CHUNK; lane++) {
            const uint32_t cand = closes[lane] && bid_len[lane] == best_len ? v[lane] : 0u;
            if (cand > best_value) best_value = cand;
        }
        const uint32_t last = n_kept ? n_kept - 1 : 0;
        fold_chunk(c, n_kept, chunk_sum, n_closed, best_len, best_value, more, v[last], run_len[last]);
        if (!more) break;
    }
    uint32_t next_count = 0;
    if (len <= CHUNK) {
        for (uint32_t lane = 0; lane < CHUNK; lane++) next_count += kept[lane] && c.mode != 0xFFFFFFFFu && v[lane] == c.mode + 1u;
    } else {
        next_count = next_count_by_search([&](uint32_t i) { return load(i); }, c.keep, c.mode);
    }
    return summary_of_carry(c, len, median, next_count);
}

template <class F>
int by_width(uint32_t width, F&& f) {
    if (width == 4) f((const uint32_t*)nullptr);
    else if (width == 2) f((const uint16_t*)nullptr);
    else if (width == 1) f((const uint8_t*)nullptr);
    else return -1;
    return 0;
}

}  // namespace

extern "C" {

void rs_constants(uint32_t* out) {
    out[0] = CUT_ENTRIES; out[1] = CUT_NONE; out[2] = CHUNK; out[3] = MEDIAN_LAMBDA_MAX; out[4] = SAMPLE_SIZE_CUTOFF;
    out[5] = (uint32_t)sizeof(Filter); out[6] = (uint32_t)sizeof(RowSummary);
}
uint32_t rs_keep_limit(uint32_t median, const uint32_t* cut) { return keep_limit(median, cut); }
// out: the nine words of a RowSummary (row = 0)
int rs_summarise(const void* row, uint32_t width, uint32_t len, const uint32_t* cut, uint32_t* out) {
    return by_width(width, [&](auto* tag) {
        const RowSummary s = summarise_row((decltype(tag))row, len, cut);
        memcpy(out, &s, sizeof(s));
    });
}
// -> 0, or 1 when a load left the row
int rs_replay(const void* row, uint32_t width, uint32_t len, const uint32_t* cut, uint32_t* out) {
    int err = 0;
    if (by_width(width, [&](auto* tag) {
            const RowSummary s = replay_row((decltype(tag))row, len, cut, &err);
            memcpy(out, &s, sizeof(s));
        }))
        return -1;
    return err;
}
// the table from a pass matrix: pass[m * stride + x] != 0 <=> poisson_cdf(m, x) < CUTOFF_PVALUE, x < stride (beyond: fails)
void rs_cut_table(const uint8_t* pass, uint32_t stride, uint32_t* cut) {
    build_cut_table([&](uint32_t m, uint32_t x) { return x < stride && pass[(uint64_t)m * stride + x] != 0; }, cut);
}
int rs_surely_rejected(const uint32_t* summary, uint32_t contain_count, uint64_t n_genome_kmers, const void* filter) {
    RowSummary s;
    Filter f;
    memcpy(&s, summary, sizeof(s));
    memcpy(&f, filter, sizeof(f));
    return surely_rejected(s, contain_count, n_genome_kmers, f);
}
// many rows at once (the soundness test): summaries of 9 words each
void rs_surely_rejected_n(const uint32_t* summaries, const uint64_t* n_genome_kmers, uint64_t n, const void* filter, uint8_t* out) {
    Filter f;
    memcpy(&f, filter, sizeof(f));
    for (uint64_t i = 0; i < n; i++) {
        RowSummary s;
        memcpy(&s, summaries + 9 * i, sizeof(s));
        out[i] = surely_rejected(s, s.contain_count, n_genome_kmers[i], f);
    }
}

}  // extern "C"
