// C entry points over sylph_amd/csrc/table_summary_plan.h for tests/test_table_summary_plan.py and tests/table_summary_sanitize_main.cpp:
// the header the kernels include, compiled with the host compiler.
#include <vector>

#include "../sylph_amd/csrc/table_summary_plan.h"

using namespace sylph::table_summary_plan;

namespace {
bool make_ladder(const uint32_t* caps, const uint32_t* chunks, uint32_t n_rungs, uint32_t max_open, Ladder& l) {
    l = Ladder{n_rungs, max_open, {}};
    if (n_rungs > MAX_RUNGS) return false;
    for (uint32_t r = 0; r < n_rungs; r++) l.rung[r] = Rung{caps[r], chunks[r]};
    return ladder_ok(l);
}
}  // namespace

extern "C" {

// MAX_RUNGS, GROUP, TILE, sizeof(Summary), sizeof(RungState), sizeof(ChunkRecord), the flags, the default ladder
void ts_constants(uint32_t* out) {
    const Ladder d = default_ladder();
    uint32_t i = 0;
    out[i++] = MAX_RUNGS; out[i++] = GROUP; out[i++] = TILE; out[i++] = sizeof(Summary); out[i++] = sizeof(RungState); out[i++] = sizeof(ChunkRecord);
    out[i++] = DECLINED; out[i++] = DECLINED_LADDER; out[i++] = DECLINED_SUM; out[i++] = DECLINED_SIZE;
    out[i++] = d.n_rungs; out[i++] = d.max_open;
    for (uint32_t r = 0; r < MAX_RUNGS; r++) { out[i++] = d.rung[r].cap; out[i++] = d.rung[r].chunk; }
}
uint32_t ts_step(uint32_t m, uint32_t x) { return step(m, x); }
int ts_ladder_ok(const uint32_t* caps, const uint32_t* chunks, uint32_t n_rungs, uint32_t max_open) {
    Ladder l;
    return make_ladder(caps, chunks, n_rungs, max_open, l) ? 1 : 0;
}
void ts_walk(const uint32_t* counts, uint64_t n, Summary* out) { *out = summarise_walk(counts, n); }
// the sequential model of the device's passes; -1: a ladder the library would refuse
int ts_model(const uint32_t* counts, uint64_t n, const uint32_t* caps, const uint32_t* chunks, uint32_t n_rungs, uint32_t max_open, Summary* out) {
    Ladder l;
    if (!make_ladder(caps, chunks, n_rungs, max_open, l)) return -1;
    std::vector<ChunkRecord> records;     // sized exactly: an index behind the chunks is a sanitizer report
    std::vector<uint32_t> starts;
    *out = summarise_model(counts, n, l, [&](uint64_t n_chunks, ChunkRecord** r, uint32_t** s) {
        records.assign(n_chunks, ChunkRecord{0, {0, 0}});
        records.shrink_to_fit();
        starts.assign(n_chunks, 0);
        starts.shrink_to_fit();
        *r = records.data();
        *s = starts.data();
    });
    return 0;
}
// the verdict over forged rung states (states: n_rungs x RungState)
int ts_finish(const RungState* states, const uint32_t* caps, const uint32_t* chunks, uint32_t n_rungs, uint64_t n, Summary* out) {
    Ladder l;
    if (!make_ladder(caps, chunks, n_rungs, 0, l)) return -1;
    *out = finish(states, l, n);
    return 0;
}

// The three lemmas by brute force: every count vector over {0 .. max_count} of length 0 .. max_len, every pair of same-parity start
// states a <= b <= max_start, every cap 2 .. max_cap.  out: cases walked, then the violations of parity, order, shrink rule,
// stay-equal, clamp bound, clamp identity, and no-wrap.
void ts_lemmas(uint32_t max_count, uint32_t max_len, uint32_t max_start, uint32_t max_cap, uint64_t* out) {
    for (int i = 0; i < 8; i++) out[i] = 0;
    std::vector<uint32_t> v;
    for (uint32_t len = 0; len <= max_len; len++) {
        v.assign(len, 0);
        for (;;) {
            out[0]++;
            {   // parity, and the walk never wraps below zero
                uint32_t m = 0, i = 0;
                for (uint32_t x : v) {
                    if (!is_step(x)) continue;
                    if (m == 0 && !(x > m)) out[7]++;
                    m = step(m, x);
                    i++;
                    if ((m & 1u) != (i & 1u)) out[1]++;
                }
            }
            for (uint32_t a = 0; a <= max_start; a++) {
                for (uint32_t b = a; b <= max_start; b += 2) {
                    uint32_t p = a, q = b;
                    for (uint32_t x : v) {
                        if (!is_step(x)) continue;
                        const uint32_t d = q - p;
                        const bool between = p < x && x <= q;
                        p = step(p, x);
                        q = step(q, x);
                        if (p > q) { out[2]++; break; }
                        if (q - p != (between ? d - 2 : d)) out[3]++;
                        if (d == 0 && q != p) out[4]++;
                    }
                }
            }
            for (uint32_t cap = CAP_MIN; cap <= max_cap; cap++) {
                uint32_t m = 0, mc = 0;
                bool reached = false;
                std::vector<uint32_t> plain, clamp;
                for (uint32_t x : v) {
                    if (!is_step(x)) continue;
                    m = step(m, x);
                    mc = step(mc, clamped(x, cap));
                    plain.push_back(m);
                    clamp.push_back(mc);
                    if (mc > cap) out[5]++;
                    if (mc >= cap) reached = true;
                }
                if (!reached && plain != clamp) out[6]++;
                // and from the upper start of either parity the clamped walk stays at or below it
                for (uint32_t parity = 0; parity < 2; parity++) {
                    uint32_t u = upper_start(cap, parity);
                    const uint32_t top = u;
                    for (uint32_t x : v) {
                        if (!is_step(x)) continue;
                        u = step(u, clamped(x, cap));
                        if (u > top) out[5]++;
                    }
                }
            }
            uint32_t at = 0;                      // the next vector
            while (at < len && v[at] == max_count) v[at++] = 0;
            if (at == len) break;
            v[at]++;
        }
    }
}

}  // extern "C"
