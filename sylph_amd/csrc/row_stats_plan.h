// row_stats_plan.h — the integer half of the statistics head (contain.rs:657-690, host/inference.cpp stats_head), free of HIP: what
// the head reads off one ascending coverage row before its first floating-point operation, the table behind the Poisson cut, the
// conservative reject in the index domain, and the work split of row_stats.hip — which lane takes which value and how an open run
// is carried from one 64-value chunk of a long row to the next.  row_stats.hip includes this header, the host's statistics
// (host/inference.cpp) summarise their rows through it, and tests/test_row_stats_plan.py compiles it with g++
// (tests/row_stats_plan_capi.cpp) and replays the kernel's split lane by lane against the sequential summary.
#pragma once
#include <math.h>

#include <cstdint>

#if defined(__HIPCC__)
#define SY_ROWS_HD __host__ __device__ __forceinline__
#else
#define SY_ROWS_HD inline
#endif

namespace sylph {
namespace row_stats_plan {

constexpr uint32_t CUT_ENTRIES = 30;             // the cut is looked up for a median below 30 (contain.rs:666)
constexpr uint32_t CUT_NONE = 0xFFFFFFFFu;       // poisson_cdf(m, m) fails the test already: nothing is cut at this median
constexpr uint32_t KEEP_ALL = 0xFFFFFFFFu;       // keep_limit: every value stays
constexpr uint32_t MEDIAN_LAMBDA_MAX = 2;        // MEDIAN_ANI_THRESHOLD (constants.rs): a larger median is "High", no lambda
constexpr uint32_t SAMPLE_SIZE_CUTOFF = 25;      // inference.rs:225
constexpr uint32_t CHUNK = 64;                   // values one wavefront takes per step: one per lane

// the layout of sylph_row_filter / sylph_row_summary (include/sylph_hip.h)
struct Filter {
    uint32_t struct_size, k;
    double reject_below, min_count_correct;
    uint32_t no_adj, reserved;
    uint32_t cut[CUT_ENTRIES];
};
struct RowSummary {
    uint32_t row, contain_count, median, keep, sum, n_distinct, mode, mode_count, next_count;
};

// ---- the table behind the Poisson cut ---------------------------------------------------------------------------------------
// contain.rs:666-675 walks the values from the median on and stops at the first whose cdf(median, value) reaches the cutoff; with a
// cdf that does not decrease in x (tests/test_row_stats_plan.py checks the host's for m = 1..29, x = 0..200) the values that stay
// are those <= cut[median].  pass(m, x) = poisson_cdf(m, x) < CUTOFF_PVALUE is the caller's: the table is never written down.
template <class Pass>
inline void build_cut_table(Pass pass, uint32_t* cut) {
    for (uint32_t m = 0; m < CUT_ENTRIES; m++) {
        if (!pass(m, m)) { cut[m] = CUT_NONE; continue; }
        uint32_t x = m;
        while (x < CUT_NONE - 1 && pass(m, x + 1)) x++;
        cut[m] = x;
    }
}
// the largest value the kept prefix may hold, KEEP_ALL for "no cut"
SY_ROWS_HD uint32_t keep_limit(uint32_t median, const uint32_t* cut) {
    if (median >= CUT_ENTRIES) return KEEP_ALL;
    const uint32_t c = cut[median];
    return (c == CUT_NONE || median > c) ? KEEP_ALL : c;
}

// ---- the summary of one row, sequentially (the definition; the host's stats_head runs this) -----------------------------------
// row: len >= 1 ascending values, all >= 1.  `row` and `contain_count` of the result are the caller's to fill.
template <class T>
inline RowSummary summarise_row(const T* row, uint32_t len, const uint32_t* cut) {
    RowSummary s{0, len, (uint32_t)row[len / 2], 0, 0, 0, 0, 0, 0};
    const uint32_t limit = keep_limit(s.median, cut);
    uint32_t prev_value = 0;                     // the value of the run before the one being counted
    bool prev_is_mode = false;
    for (uint32_t i = 0; i < len && (uint32_t)row[i] <= limit;) {
        const uint32_t v = (uint32_t)row[i];
        uint32_t j = i;
        while (j < len && (uint32_t)row[j] == v) { s.sum += v; j++; }
        const uint32_t c = j - i;
        if (s.n_distinct < 2) s.n_distinct++;
        if (prev_is_mode && v == prev_value + 1 && prev_value != 0xFFFFFFFFu) s.next_count = c;
        prev_is_mode = c >= s.mode_count;                                  // ascending: a tie goes to the larger value
        if (prev_is_mode) { s.mode = v; s.mode_count = c; s.next_count = 0; }
        prev_value = v;
        s.keep = j;
        i = j;
    }
    return s;
}

// ---- the conservative reject ------------------------------------------------------------------------------------------------------
// stats_head's branches (High above MEDIAN_LAMBDA_MAX; ratio_lambda with SAMPLE_SIZE_CUTOFF and min_count_correct; no_adj) up to the
// containment index, whose k-th root is the ANI the cut tests.  No pow: the caller moved the cut into the index domain
// (reject_below = min_ani^k (1 - 2^-30)).  true only for a row no rounding of pow, exp and the divisions could lift over min_ani.
SY_ROWS_HD bool lambda_of(const RowSummary& s, double min_count_correct, double* lambda) {
    if (s.median > MEDIAN_LAMBDA_MAX) return false;
    if (s.n_distinct == 1 || s.keep < SAMPLE_SIZE_CUTOFF || s.next_count == 0) return false;
    const double count_p1 = (double)s.next_count, count = (double)s.mode_count;
    if (count_p1 < min_count_correct || count < min_count_correct) return false;
    *lambda = count_p1 / count * (double)((uint64_t)s.mode + 1);
    return true;
}
SY_ROWS_HD bool surely_rejected(const RowSummary& s, uint32_t contain_count, uint64_t n_genome_kmers, const Filter& f) {
    if (!(f.reject_below > 0.)) return false;
    double lambda = 0.;
    if (f.no_adj || !lambda_of(s, f.min_count_correct, &lambda)) return (double)contain_count / (double)n_genome_kmers < f.reject_below;
    const uint64_t n_total = n_genome_kmers - contain_count + s.keep;
    const double index = (double)s.keep / (1. - exp(-lambda)) / (double)n_total;
    if (!(index >= 0.) || index > 1.7976931348623157e308) return false;      // NaN, negative, infinite: the host decides
    return index < f.reject_below;
}

// ---- the work split of row_stats.hip ------------------------------------------------------------------------------------------
// One wavefront per row.  It reads the median (row[len / 2], one load for all lanes) and with it the limit, then walks the row in
// chunks of CHUNK values, lane l holding value base + l.  The kept lanes of a chunk are a prefix of it (the row ascends): n_kept of
// them.  A lane starts a run when its left neighbour holds another value (lane 0 always does: the carry decides whether its run
// began in an earlier chunk); `starts` is the ballot of those lanes.  A lane ends a run when the next lane starts one or it is the
// last kept lane.  The run that ends at the last kept lane of a chunk stays OPEN when the chunk is full and the row goes on
// (`more`): its value and length travel in the carry, and the next chunk either continues it (its lane 0 holds the same value) or
// closes it before anything else.  Every closed run counts one distinct value and bids (length, value) for the mode; the largest
// bid wins, lexicographically, which is "ties go to the larger value".  The walk ends behind the first chunk that is not `more`.
// next_count is counted afterwards, when the mode is known: in a row of one chunk by a ballot over the values still in registers,
// in a longer one as the difference of two binary searches over the kept prefix (count_at_most).
struct Carry {
    uint32_t keep, sum, n_runs, mode, mode_count;   // over the closed runs so far
    uint32_t open_value, open_len;                   // the run left open by the previous chunk; open_len == 0: none
};
SY_ROWS_HD Carry carry_begin() { return Carry{0, 0, 0, 0, 0, 0, 0}; }
SY_ROWS_HD uint64_t low_lanes(uint32_t n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }
SY_ROWS_HD bool lane_kept(uint64_t index, uint64_t len, uint32_t value, uint32_t limit) { return index < len && value <= limit; }
SY_ROWS_HD bool lane_starts_run(uint32_t lane, bool kept, uint32_t value, uint32_t left_value) { return kept && (lane == 0 || value != left_value); }
SY_ROWS_HD bool chunk_has_more(uint32_t n_kept, uint64_t base, uint64_t len) { return n_kept == CHUNK && base + CHUNK < len; }
SY_ROWS_HD void bid(Carry& c, uint32_t run_len, uint32_t value) {
    if (run_len > c.mode_count || (run_len == c.mode_count && value >= c.mode)) { c.mode = value; c.mode_count = run_len; }
}
// before the lanes of a chunk look at the carry: an open run the chunk does not continue is closed
SY_ROWS_HD void close_stale_run(Carry& c, uint32_t n_kept, uint32_t first_value) {
    if (c.open_len && (n_kept == 0 || first_value != c.open_value)) {
        c.n_runs++;
        bid(c, c.open_len, c.open_value);
        c.open_len = 0;
    }
}
// length of the run `lane` belongs to, from its start up to and including the lane, the open run of the carry included (lane < n_kept)
SY_ROWS_HD uint32_t run_len_up_to(uint32_t lane, uint64_t starts, uint32_t value, const Carry& c) {
    const uint64_t below = starts & low_lanes(lane + 1);                     // bit 0 is always set
    const uint32_t start = 63u - (uint32_t)__builtin_clzll(below);
    uint32_t n = lane - start + 1;
    if (start == 0 && c.open_len && value == c.open_value) n += c.open_len;
    return n;
}
// does a run CLOSE at this lane?
SY_ROWS_HD bool lane_closes_run(uint32_t lane, uint32_t n_kept, uint64_t starts, bool more) {
    if (lane >= n_kept) return false;
    if (lane + 1 == n_kept) return !more;
    return ((starts >> (lane + 1)) & 1u) != 0;
}
// behind the lanes: the chunk's totals (n_closed runs closed, the best bid among them — best_len == 0: none) and the run left open
SY_ROWS_HD void fold_chunk(Carry& c, uint32_t n_kept, uint32_t chunk_sum, uint32_t n_closed, uint32_t best_len, uint32_t best_value, bool more,
                           uint32_t last_value, uint32_t last_run_len) {
    c.keep += n_kept;
    c.sum += chunk_sum;
    c.n_runs += n_closed;
    if (best_len) bid(c, best_len, best_value);
    c.open_len = more ? last_run_len : 0;
    c.open_value = more ? last_value : 0;
}
// number of the first n ascending values that are <= x
template <class Load>
SY_ROWS_HD uint32_t count_at_most(Load load, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (load(mid) <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
template <class Load>
SY_ROWS_HD uint32_t next_count_by_search(Load load, uint32_t keep, uint32_t mode) {
    if (mode == 0xFFFFFFFFu) return 0;
    return count_at_most(load, keep, mode + 1) - count_at_most(load, keep, mode);
}
SY_ROWS_HD RowSummary summary_of_carry(const Carry& c, uint32_t len, uint32_t median, uint32_t next_count) {
    return RowSummary{0, len, median, c.keep, c.sum, c.n_runs < 2 ? c.n_runs : 2u, c.mode, c.mode_count, next_count};
}

// ---- the gather ---------------------------------------------------------------------------------------------------------------
// Candidates keep their row order: candidate j of a launch is the j-th row whose flag is set, its values start at the sum of the
// lengths of the candidates before it (two exclusive sums over the rows), and the wavefront that summarised nothing for a row
// copies nothing for it.

}  // namespace row_stats_plan
}  // namespace sylph
