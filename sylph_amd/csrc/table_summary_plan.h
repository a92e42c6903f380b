// table_summary_plan.h — the arithmetic of K15, the sample table's summary for --estimate-unknown (contain.rs:901-951
// get_kmer_identity, :392-408 estimate_covered_bases), HIP-free: table_summary.hip's kernels call the bodies below lane by lane, the
// host compiles the same header, and tests/test_table_summary_plan.py drives it through tests/table_summary_plan_capi.cpp.
//
// What the host reads off a table are three walks over its counts, in the table's order (ascending k-mers):
//   the running "continuous median":  x_1 .. x_S = the counts > 1;  m_0 = 0,  m_i = m_{i-1} + 1 if x_i > m_{i-1} else m_{i-1} - 1;
//                                     mov_avg_median = (sum of the m_i) / (1 + S)
//   the multiplicity-1 share:         num_1s = #(count == 1), num_not1s = the u32 WRAPPING sum of the counts != 1
//   the total:                        total_counts = the u64 sum of all counts
// Five integers and a maximum (Summary); the f64 decision stays with the host.  The sums are reductions; the median is a sequential
// +-1 walk, and runs exactly in parallel on three facts (each proven by brute force in the CPU test):
//   PARITY       m_i = i (mod 2): every step changes the state by one.  (m never wraps: a state of 0 or 1 meets x >= 2 and goes up.)
//   COALESCENCE  two walks of the same parity, a <= b, stay ordered under a step, and b' - a' is b - a or b - a - 2 — it shrinks
//                exactly when a < x <= b; once equal they stay equal.  So if the walks from a lower and an upper bound of a chunk's
//                start state meet inside the chunk, the chunk's end state does not depend on its start: the chunk is CLOSED.
//   CLAMP        with x' = min(x, C): as long as the walk over x' stays below C it IS the walk over x (m < C gives
//                (min(x, C) > m) <=> (x > m)), and it never exceeds C.  So C — or C + 1, for the parity — bounds every chunk's
//                start state from above, the parity's minimum (0 or 1) from below, and a rare count of 10^5 costs nothing.
// The plan, per RUNG (a cap C with its chunk length L) of a short ladder:
//   pass 1   every chunk of L entries walks FOUR states over the clamped counts, a lower and an upper one for either parity of the
//            steps before it (the parity is not known yet; four independent chains also fill the latency of one), and records its
//            steps and, per parity, its end state if the two met, else OPEN.  The same pass reduces the three sums.
//   pass 2   one walker goes through the records in order: a closed chunk hands on its constant end state, a chunk without a step
//            its start, an open chunk is walked again from its now known start.  More than max_open open chunks: the rung gives up.
//            It leaves every chunk's start state.
//   pass 3   every chunk walks again from its true start and sums the states and their maximum.
//   verdict  the rung answers iff it did not give up and max_state < C (then the clamped walk was the walk).  Else the next rung.
// After the last rung, or with a sum of 2^53 or more (the host's f64 additions of integers are exact below that, so (double)
// median_sum / n equals its running f64 sum bit for bit — not above), or a table of 2^31 entries or more, the summary DECLINES:
// the caller walks the counts on the host.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SY_TSUM_HD __host__ __device__ __forceinline__
#define SY_TSUM_UNROLL _Pragma("unroll")
#define SY_TSUM_NOUNROLL _Pragma("nounroll")
#else
#define SY_TSUM_HD inline
#define SY_TSUM_UNROLL
#define SY_TSUM_NOUNROLL
#endif

namespace sylph {
namespace table_summary_plan {

// ---- the summary (include/sylph_hip.h sylph_table_summary_t is this, field for field) ----
constexpr uint32_t DECLINED = 1u;              // flags: the summary declined (the bits below say why); the walk's fields are 0
constexpr uint32_t DECLINED_LADDER = 2u;       //   no rung of the ladder answered
constexpr uint32_t DECLINED_SUM = 4u;          //   median_sum reached 2^53
constexpr uint32_t DECLINED_SIZE = 8u;         //   2^31 entries or more: nothing was counted
struct Summary {
    uint64_t median_sum;       // sum of m_1 .. m_S
    uint64_t total_counts;
    uint32_t steps;            // S
    uint32_t num_1s;
    uint32_t num_not1s;        // wraps, as the host's uint32_t does
    uint32_t max_state;        // the largest m_i
    uint32_t flags;
    uint32_t rung;             // the rung that answered (n_rungs: none did)
    uint32_t open_chunks;      // chunks pass 2 walked again on that rung
    uint32_t reserved;
};
constexpr uint64_t SUM_LIMIT = 1ull << 53;
constexpr uint64_t MAX_ENTRIES = 1ull << 31;

// ---- the ladder ----
// Defaults.  Real tables hold many counts of 1 (error k-mers), which are no steps, and the two walks of a chunk meet after about C
// steps plus the climb to the equilibrium: the first rung's cap is small so that a shallow metagenome closes its chunks with one
// step in fifty entries, and the deeper rungs take 16 entries per unit of cap.  Simulated on the CPU (tests/test_table_summary_plan.py
// test_default_ladder_on_simulated_tables: 400,000 entries, log-normal Poisson depths, 1 in 5,000 entries set to 5*10^4 .. 2*10^6):
// states near 3 and 9 answer on rung 0, near 400 on rung 1, with no open chunk.  No GPU time decided any of them.
constexpr uint32_t MAX_RUNGS = 4;
struct Rung { uint32_t cap, chunk; };
struct Ladder { uint32_t n_rungs; uint32_t max_open; Rung rung[MAX_RUNGS]; };
constexpr uint32_t MAX_OPEN_DEFAULT = 64;
constexpr uint32_t CAP_MIN = 2, CAP_MAX = 1u << 30;         // (x' = min(x, C) must keep x' >= 2 a step; C + 1 must not wrap)
SY_TSUM_HD Ladder default_ladder() { return Ladder{3, MAX_OPEN_DEFAULT, {{64, 4096}, {1024, 16384}, {16384, 262144}, {0, 0}}}; }
SY_TSUM_HD bool ladder_ok(const Ladder& l) {
    if (l.n_rungs < 1 || l.n_rungs > MAX_RUNGS) return false;
    for (uint32_t r = 0; r < l.n_rungs; r++) {
        if (l.rung[r].cap < CAP_MIN || l.rung[r].cap > CAP_MAX || l.rung[r].chunk < 1) return false;
        if (r && l.rung[r].cap <= l.rung[r - 1].cap) return false;
    }
    return true;
}

// ---- the step ----
SY_TSUM_HD uint32_t step(uint32_t m, uint32_t x) { return x > m ? m + 1u : m - 1u; }     // (x >= 2: m never goes below 1 again)
SY_TSUM_HD bool is_step(uint32_t count) { return count > 1u; }
SY_TSUM_HD uint32_t clamped(uint32_t x, uint32_t cap) { return x < cap ? x : cap; }
SY_TSUM_HD uint32_t lower_start(uint32_t parity) { return parity; }                                  // 0 or 1
SY_TSUM_HD uint32_t upper_start(uint32_t cap, uint32_t parity) { return cap + ((cap ^ parity) & 1u); }   // C or C + 1

// the three sums
struct Tally { uint64_t total; uint32_t num_1s, num_not1s; };
SY_TSUM_HD void tally_add(Tally& t, uint32_t count) {
    if (count == 1u) t.num_1s += 1u; else t.num_not1s += count;
    t.total += count;
}

// ---- chunk geometry: a workgroup of GROUP lanes takes GROUP consecutive chunks, one per lane, and stages TILE entries of each per
// round through a tile of GROUP x (TILE + 1) words (the odd pitch keeps the lanes' reads off each other's banks): the loads are
// coalesced runs of TILE entries, a lane's chain is a read of its own row, a compare and an add ----
constexpr uint32_t GROUP = 64, TILE = 32, TILE_PITCH = TILE + 1, TILE_WORDS = GROUP * TILE_PITCH;
SY_TSUM_HD uint64_t n_chunks_of(uint64_t n, uint32_t chunk) { return (n + chunk - 1) / chunk; }
SY_TSUM_HD uint32_t n_groups_of(uint64_t n, uint32_t chunk) { return (uint32_t)((n_chunks_of(n, chunk) + GROUP - 1) / GROUP); }
SY_TSUM_HD uint32_t n_rounds_of(uint32_t chunk) { return (chunk + TILE - 1) / TILE; }
// What lane `lane` brings into the tile in round `round` of group `group`: TILE_WORDS / GROUP words; an entry behind its chunk or
// behind the table is a 0 — no step, and nothing to any sum.  tally: null in pass 3.
// STAGE_BATCH of a lane's loads are issued before the first of them is used: TILE / STAGE_BATCH memory latencies per round, not TILE
// (all TILE at once cost the kernels over 200 VGPRs for the addresses; eight keep them small).
constexpr uint32_t STAGE_BATCH = 8;
static_assert(TILE % STAGE_BATCH == 0 && GROUP % TILE == 0, "a lane stays in one column of the tile, in whole batches");
SY_TSUM_HD void stage_tile(const uint32_t* counts, uint64_t n, uint32_t chunk, uint32_t group, uint32_t round, uint32_t lane, uint32_t* tile, Tally* tally) {
    const uint32_t t = lane % TILE;                                  // (GROUP * TILE words by GROUP lanes: TILE each, all in column t)
    const uint64_t in_chunk = (uint64_t)round * TILE + t;
    SY_TSUM_NOUNROLL
    for (uint32_t first = 0; first < TILE; first += STAGE_BATCH) {
        uint32_t x[STAGE_BATCH];
        SY_TSUM_UNROLL
        for (uint32_t i = 0; i < STAGE_BATCH; i++) {
            const uint32_t c = (lane + (first + i) * GROUP) / TILE;
            const uint64_t pos = ((uint64_t)group * GROUP + c) * chunk + in_chunk;
            x[i] = (in_chunk < chunk && pos < n) ? counts[pos] : 0u;
        }
        SY_TSUM_UNROLL
        for (uint32_t i = 0; i < STAGE_BATCH; i++) {
            const uint32_t c = (lane + (first + i) * GROUP) / TILE;
            tile[c * TILE_PITCH + t] = x[i];
            if (tally) tally_add(*tally, x[i]);
        }
    }
}

// ---- pass 1 ----
constexpr uint32_t OPEN = 0xFFFFFFFFu;
struct ChunkRecord { uint32_t steps; uint32_t end[2]; };   // end[p]: the end state after an even / odd number of steps before the chunk, or OPEN
struct Walk1 { uint32_t lo[2], hi[2], steps; };
SY_TSUM_HD Walk1 walk1_begin(uint32_t cap) { return Walk1{{lower_start(0), lower_start(1)}, {upper_start(cap, 0), upper_start(cap, 1)}, 0}; }
SY_TSUM_HD void walk1_step(Walk1& w, uint32_t count, uint32_t cap) {
    if (!is_step(count)) return;
    const uint32_t x = clamped(count, cap);
    w.lo[0] = step(w.lo[0], x); w.hi[0] = step(w.hi[0], x);
    w.lo[1] = step(w.lo[1], x); w.hi[1] = step(w.hi[1], x);
    w.steps += 1u;
}
SY_TSUM_HD void walk1_tile(Walk1& w, const uint32_t* tile, uint32_t lane, uint32_t cap) {
    for (uint32_t t = 0; t < TILE; t++) walk1_step(w, tile[lane * TILE_PITCH + t], cap);
}
SY_TSUM_HD ChunkRecord walk1_end(const Walk1& w) {
    return ChunkRecord{w.steps, {w.lo[0] == w.hi[0] ? w.lo[0] : OPEN, w.lo[1] == w.hi[1] ? w.lo[1] : OPEN}};
}

// ---- pass 2: in chunk order.  rewalk(start) -> the chunk's end state, walked over the clamped counts from `start` ----
struct Pass2 { uint64_t steps; uint32_t state, open, gave_up; };
SY_TSUM_HD Pass2 pass2_begin() { return Pass2{0, 0, 0, 0}; }
// returns the chunk's start state; after a give-up the walker's state means nothing
template <class Rewalk>
SY_TSUM_HD uint32_t pass2_chunk(Pass2& s, const ChunkRecord& r, uint32_t max_open, Rewalk&& rewalk) {
    const uint32_t start = s.state;
    if (r.steps != 0u && !s.gave_up) {
        const uint32_t end = r.end[s.steps & 1u];
        if (end != OPEN) s.state = end;
        else if (s.open >= max_open) s.gave_up = 1u;
        else { s.open += 1u; s.state = rewalk(start); }
    }
    s.steps += r.steps;
    return start;
}
SY_TSUM_HD uint32_t rewalk_step(uint32_t m, uint32_t count, uint32_t cap) { return is_step(count) ? step(m, clamped(count, cap)) : m; }

// ---- pass 3 ----
struct Walk3 { uint64_t sum; uint32_t state, max; };
SY_TSUM_HD void walk3_step(Walk3& w, uint32_t count, uint32_t cap) {
    if (!is_step(count)) return;
    w.state = step(w.state, clamped(count, cap));
    w.sum += w.state;
    if (w.state > w.max) w.max = w.state;
}
SY_TSUM_HD void walk3_tile(Walk3& w, const uint32_t* tile, uint32_t lane, uint32_t cap) {
    for (uint32_t t = 0; t < TILE; t++) walk3_step(w, tile[lane * TILE_PITCH + t], cap);
}

// ---- the verdict.  RungState: what a rung's three passes leave (all zero before them) ----
struct RungState {
    uint64_t median_sum, total_counts;
    uint32_t steps, num_1s, num_not1s, max_state, gave_up, open;
};
SY_TSUM_HD bool rung_answers(const RungState& s, uint32_t cap) { return !s.gave_up && s.max_state < cap; }
// a later rung's kernels return at once when an earlier one answered: no host round trip between the rungs
SY_TSUM_HD bool answered_before(const RungState* states, const Ladder& l, uint32_t rung) {
    for (uint32_t r = 0; r < rung; r++)
        if (rung_answers(states[r], l.rung[r].cap)) return true;
    return false;
}
SY_TSUM_HD Summary declined(Summary s, uint32_t why, uint32_t n_rungs) {
    s.median_sum = 0; s.max_state = 0; s.open_chunks = 0;
    s.flags = DECLINED | why;
    s.rung = n_rungs;
    return s;
}
// states[0 .. n_rungs) of a table of n entries -> the summary
SY_TSUM_HD Summary finish(const RungState* states, const Ladder& l, uint64_t n) {
    Summary s{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (n >= MAX_ENTRIES) return declined(s, DECLINED_SIZE, l.n_rungs);
    if (n == 0) return s;
    // (every rung that ran counted the same sums: the first always runs)
    s.total_counts = states[0].total_counts; s.steps = states[0].steps; s.num_1s = states[0].num_1s; s.num_not1s = states[0].num_not1s;
    for (uint32_t r = 0; r < l.n_rungs; r++) {
        if (!rung_answers(states[r], l.rung[r].cap)) continue;
        if (states[r].median_sum >= SUM_LIMIT) return declined(s, DECLINED_SUM, l.n_rungs);
        s.median_sum = states[r].median_sum; s.max_state = states[r].max_state; s.open_chunks = states[r].open; s.rung = r;
        return s;
    }
    return declined(s, DECLINED_LADDER, l.n_rungs);
}

// ---- the sequential model of one rung, through the very bodies the kernels call (group by group, round by round, lane by lane):
// what the CPU tests compare with the plain walk.  records / starts: n_chunks_of(n, chunk) entries of scratch ----
inline void rung_model(const uint32_t* counts, uint64_t n, const Ladder& l, uint32_t r, ChunkRecord* records, uint32_t* starts, RungState& st) {
    const uint32_t cap = l.rung[r].cap, chunk = l.rung[r].chunk;
    const uint64_t n_chunks = n_chunks_of(n, chunk);
    const uint32_t n_groups = n_groups_of(n, chunk), n_rounds = n_rounds_of(chunk);
    uint32_t tile[TILE_WORDS];
    Tally tally{0, 0, 0};
    for (uint32_t g = 0; g < n_groups; g++) {                        // pass 1
        Walk1 w[GROUP];
        for (uint32_t lane = 0; lane < GROUP; lane++) w[lane] = walk1_begin(cap);
        for (uint32_t round = 0; round < n_rounds; round++) {
            for (uint32_t lane = 0; lane < GROUP; lane++) stage_tile(counts, n, chunk, g, round, lane, tile, &tally);
            for (uint32_t lane = 0; lane < GROUP; lane++) walk1_tile(w[lane], tile, lane, cap);
        }
        for (uint32_t lane = 0; lane < GROUP; lane++)
            if ((uint64_t)g * GROUP + lane < n_chunks) records[(uint64_t)g * GROUP + lane] = walk1_end(w[lane]);
    }
    st.total_counts = tally.total; st.num_1s = tally.num_1s; st.num_not1s = tally.num_not1s;
    Pass2 p = pass2_begin();                                         // pass 2
    for (uint64_t c = 0; c < n_chunks; c++) {                        // (to the end even after a give-up: the steps are a sum the host reads)
        starts[c] = pass2_chunk(p, records[c], l.max_open, [&](uint32_t m) {
            const uint64_t lo = c * chunk, hi = lo + chunk < n ? lo + chunk : n;
            for (uint64_t i = lo; i < hi; i++) m = rewalk_step(m, counts[i], cap);
            return m;
        });
    }
    st.steps = (uint32_t)p.steps; st.gave_up = p.gave_up; st.open = p.open;
    if (p.gave_up) return;
    for (uint32_t g = 0; g < n_groups; g++) {                        // pass 3
        Walk3 w[GROUP];
        for (uint32_t lane = 0; lane < GROUP; lane++) {
            const uint64_t c = (uint64_t)g * GROUP + lane;
            w[lane] = Walk3{0, c < n_chunks ? starts[c] : 0u, 0};
        }
        for (uint32_t round = 0; round < n_rounds; round++) {
            for (uint32_t lane = 0; lane < GROUP; lane++) stage_tile(counts, n, chunk, g, round, lane, tile, nullptr);
            for (uint32_t lane = 0; lane < GROUP; lane++) walk3_tile(w[lane], tile, lane, cap);
        }
        for (uint32_t lane = 0; lane < GROUP; lane++) {
            st.median_sum += w[lane].sum;
            if (w[lane].max > st.max_state) st.max_state = w[lane].max;
        }
    }
}
// the whole ladder, as the device runs it: a rung runs only while none before it answered
template <class Scratch>
inline Summary summarise_model(const uint32_t* counts, uint64_t n, const Ladder& l, Scratch&& scratch) {
    RungState states[MAX_RUNGS] = {};
    if (n > 0 && n < MAX_ENTRIES) {
        for (uint32_t r = 0; r < l.n_rungs; r++) {
            if (answered_before(states, l, r)) break;
            const uint64_t n_chunks = n_chunks_of(n, l.rung[r].chunk);
            ChunkRecord* records = nullptr;
            uint32_t* starts = nullptr;
            scratch(n_chunks, &records, &starts);
            rung_model(counts, n, l, r, records, starts, states[r]);
        }
    }
    return finish(states, l, n);
}

// the plain walk: the definition (and the host's road), in integers
inline Summary summarise_walk(const uint32_t* counts, uint64_t n) {
    Summary s{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t m = 0;
    Tally t{0, 0, 0};
    for (uint64_t i = 0; i < n; i++) {
        tally_add(t, counts[i]);
        if (!is_step(counts[i])) continue;
        m = step(m, counts[i]);
        s.median_sum += m;
        s.steps += 1u;
        if (m > s.max_state) s.max_state = m;
    }
    s.total_counts = t.total; s.num_1s = t.num_1s; s.num_not1s = t.num_not1s;
    return s;
}

}  // namespace table_summary_plan
}  // namespace sylph
