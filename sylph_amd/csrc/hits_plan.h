// hits_plan.h — the plan of the hit finish (contain.hip finish_driver, hits.hip), host-compilable: the constants and the index
// arithmetic of the row assembly's kernels, the geometry of one assembly, the two capacity rules, the verdict on a hit list — which
// rows_sum_kernel writes into snap[2] and the host reaches from the same two numbers — and the state function that names the
// driver's next step and records what every step leaves clean or dirty.  hits.hip and contain.hip include this header;
// tests/test_hits_plan.py compiles it with g++ (tests/hits_plan_capi.cpp) and walks every sequence of answers.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SY_HITS_HD __host__ __device__ __forceinline__
#else
#define SY_HITS_HD inline
#endif

namespace sylph {
namespace hits_plan {

constexpr int ROWS_TPB = 256, ROWS_PER_THREAD = 8, ROWS_TILE = ROWS_TPB * ROWS_PER_THREAD;
constexpr uint32_t SMALL_ROW = 64;            // rows up to one wavefront of values are ranked by shuffles
constexpr uint32_t MAX_VALUE_LDS = 4096;      // rows_sort_kernel's histogram: values below this
// stretch hash: the hits of a workgroup's stretch of the list in an LDS table of HIT_SLOTS (row, count) entries (open addressing);
// a stretch with more distinct rows than the table may hold sends the surplus hits straight to the global counters
#ifndef SYLPH_HIT_SLOTS_LOG2
#define SYLPH_HIT_SLOTS_LOG2 12
#endif
constexpr uint32_t HIT_SLOTS = 1u << SYLPH_HIT_SLOTS_LOG2, HIT_SLOTS_FULL = HIT_SLOTS * 3 / 4;
constexpr uint32_t STRETCH_ROUND = 256;       // a workgroup takes its stretch in rounds of 256 hits, one per thread
// Whether the table still takes new rows is decided between two rounds, for the whole workgroup: a round adds at most
// STRETCH_ROUND rows to a table that was below HIT_SLOTS_FULL before it, so a claim always finds a free slot
static_assert(HIT_SLOTS_FULL + STRETCH_ROUND <= HIT_SLOTS, "SYLPH_HIT_SLOTS_LOG2 too small: a round of 256 hits could fill the stretch table");

SY_HITS_HD uint32_t hash_row(uint32_t row) { return (row * 2654435761u) >> (32 - SYLPH_HIT_SLOTS_LOG2); }   // top bits
// where the counter of a row lives: a bijection of [0, 2^m) (an odd multiplier) that sends neighbouring rows to different cache lines
SY_HITS_HD uint32_t rc_at(uint32_t row, uint32_t rc_mask) { return (row * 0x9E3779B1u) & rc_mask; }
// the stretch of workgroup `block` of `grid`: whole multiples of 256 hits.  Written so that nothing wraps up to n = 2^32 - 1:
// block * per < n + 256 * grid - n / grid stays below 2^32 for every grid geometry() hands out (n / grid outweighs 256 * grid long
// before n comes near the top), and the end is taken from what is left of the list, not from lo + per.
SY_HITS_HD void stretch_of(uint32_t n, uint32_t grid, uint32_t block, uint32_t& lo, uint32_t& hi) {
    const uint32_t per = (n / grid + (n % grid != 0 ? 1u : 0u) + (STRETCH_ROUND - 1)) & ~(STRETCH_ROUND - 1);
    const uint32_t at = block * per;
    lo = at < n ? at : n;
    hi = lo + (per < n - lo ? per : n - lo);
}

// One row assembly: R rows, a hit array of `cap` entries, about n_guess hits (device-known sizes: half the array; else the number).
// row_meta = [tile_sum n_tiles | snap 4 | lists: 2 lengths, then list_cap rows] in words.  The two row lists grow towards each other
// from both ends of the list_cap entries: every listed row has a hit of its own among at most max(cap, 1) and is one of R rows, so
// small + long rows <= list_cap and they never meet.
struct Geometry {
    bool taken;                       // false: no row assembly for this many rows (none, or 2^31 and more); nothing else is set
    uint32_t R, R2, rc_mask;          // counters: a power of two (rc_at is a bijection of [0, R2))
    uint32_t n_tiles, list_cap, hit_grid;
    size_t rc_bytes, meta_bytes;
    uint32_t tile_sum_at, snap_at, lists_at;   // word offsets inside row_meta
};
inline Geometry geometry(uint64_t n_rows, uint64_t cap, uint64_t n_guess) {
    Geometry g{};
    if (n_rows == 0 || n_rows >= (1ull << 31)) return g;
    g.taken = true;
    g.R = (uint32_t)n_rows;
    g.R2 = 1024;
    while (g.R2 < g.R) g.R2 <<= 1;
    g.rc_mask = g.R2 - 1;
    g.n_tiles = (g.R + ROWS_TILE - 1) / ROWS_TILE;
    const uint64_t room = cap > 1 ? cap : 1;
    g.list_cap = (uint32_t)(g.R < room ? g.R : room);
    g.rc_bytes = (size_t)g.R2 * 4;
    g.meta_bytes = ((size_t)g.n_tiles + 4 + 2 + g.list_cap) * 4 + 64;
    // a few dozen long stretches: the fewer workgroups, the fewer atomics per row counter (one per workgroup and distinct row)
    const uint64_t want = n_guess / 6144;
    g.hit_grid = (uint32_t)(want < 16 ? 16 : want > 768 ? 768 : want);
    g.tile_sum_at = 0;
    g.snap_at = g.n_tiles;
    g.lists_at = g.n_tiles + 4;
    return g;
}

// the hit array of a first launch over `total` sample k-mers, and the limit of any launch
inline uint64_t first_capacity(uint64_t total) { return 2 * total > (1ull << 20) ? 2 * total : (1ull << 20); }
inline bool fits(uint64_t cap) { return cap < (1ull << 32); }

// What becomes of a hit list of n_counted hits (as counted: a probe that overflowed counted more than it stored), the largest of
// them max_count, in an array of cap entries.  Overflow first: whatever else is true of such a list, it is not all there.
enum class Verdict { Regrow, Sorted, Rows };
SY_HITS_HD Verdict verdict(uint32_t n_counted, uint32_t max_count, uint32_t cap) {
    if (n_counted > cap) return Verdict::Regrow;
    return max_count >= MAX_VALUE_LDS ? Verdict::Sorted : Verdict::Rows;
}

// ---- the driver's steps --------------------------------------------------------------------------------------------------------
// Device: the assembly is queued behind the probe and takes the list's sizes from the two words the probe counted into, which the host
// reads while it runs; Host: the sizes are known to the host before the assembly — given, or read behind a probe it waited for.
enum class Sizes { Device, Host };
enum class Step {
    Probe,         // the caller's launch with a hit array of first_capacity (-> counts into the two words)
    Assemble,      // launch_row_assembly: five kernels
    ReadWords,     // wait for the two words; the answer is verdict() of them
    RegrowProbe,   // the launch once more, with room for every hit the first one counted
    Sorted,        // finish_hits_sorted, which copies out itself: the end
    CopyOut,       // the assembled block: the end
    Done,          // (finish = false) the hit list is all there: the end
    Fail,          // "hit buffer overflow persisted": the end
};
constexpr uint32_t MAX_PROBES = 2;

struct State {
    bool to_probe;       // false: nothing to launch, the sizes are host-known from the start (`verdict` is set, `read` is true)
    Sizes sizes;
    bool force_sort;     // SYLPH_HIP_HIT_SORT
    bool rows_taken;     // Geometry::taken for the call's rows
    bool finish;         // false: the caller wants the hit list only (the sharded probe)
    uint32_t probes;
    bool assembled, read;
    Verdict verdict;
    // The record.  The row counters must be zero when an assembly starts, the two counter words when a probe does; a dirty flag
    // makes the launcher clear them first.  Which step leaves what:
    //   a probe              counts into the two words, and nothing behind it zeroes them ...
    //   an assembly, Rows    ... but rows_sort_kernel, when it was handed the device words.  The scan zeroes the counters of the
    //                        non-empty rows (they become cursors), the per-row sort zeroes its row's again: clean
    //   behind snap[2]       the scatter and the sort return at once: the words stay, and the counters count as dirty (the scan
    //                        has in fact zeroed them; the flag is kept as it always was, and with it the dispatches of a call)
    //   host-known sizes     the words are not handed over and stay as they are
    bool rc_dirty, cnt_dirty;
};

inline bool row_road(const State& s) { return !s.force_sort && s.rows_taken; }
inline bool behind_probe(const State& s) { return s.sizes == Sizes::Device && row_road(s); }

// The order and the number of launches are what they always were: the row road behind a probe does not wait for the words before
// it assembles, every other road does; an overflowed list is probed once more and never a third time; a forced sort and a row
// space the assembly does not take never assemble.  Ends: every step but the last moves probes, assembled or read forwards, and
// only RegrowProbe takes the latter two back, once.
inline Step next(const State& s) {
    if (s.to_probe && s.probes == 0) return Step::Probe;
    if (!s.read) return behind_probe(s) && !s.assembled ? Step::Assemble : Step::ReadWords;
    if (s.verdict == Verdict::Regrow) return s.to_probe && s.probes < MAX_PROBES ? Step::RegrowProbe : Step::Fail;
    if (!s.finish) return Step::Done;
    if (!row_road(s) || s.verdict == Verdict::Sorted) return Step::Sorted;
    return s.assembled ? Step::CopyOut : Step::Assemble;
}

// the state behind a completed step (answer: of ReadWords)
inline State after(State s, Step step, Verdict answer = Verdict::Rows) {
    switch (step) {
    case Step::Probe:
    case Step::RegrowProbe:
        s.probes++;
        s.read = s.assembled = false;
        s.cnt_dirty = true;
        break;
    case Step::Assemble:
        s.assembled = true;
        s.rc_dirty = false;                  // (behind a probe: until the words say otherwise)
        break;
    case Step::ReadWords:
        s.read = true;
        s.verdict = answer;
        if (s.assembled) { if (answer == Verdict::Rows) s.cnt_dirty = false; else s.rc_dirty = true; }
        break;
    default:
        break;
    }
    return s;
}
// a step that threw half-way: nothing is known to be clean
inline State failed(State s) { s.rc_dirty = s.cnt_dirty = true; return s; }

// known: the verdict on host-known sizes (to_probe = false)
inline State start(bool to_probe, Sizes sizes, bool force_sort, bool rows_taken, bool finish, bool rc_dirty, bool cnt_dirty,
                   Verdict known = Verdict::Rows) {
    return State{to_probe, sizes, force_sort, rows_taken, finish, 0, false, !to_probe, known, rc_dirty, cnt_dirty};
}

}  // namespace hits_plan
}  // namespace sylph
