// inference.cpp — coverage-adjusted ANI statistics, kept on the host as the north_star prescribes (f64 throughout).
// Restates contain.rs:657-813 (statistics half of get_stats), :817-847 (ani_from_lambda), :849-898 (bootstrap_interval)
// and inference.rs:104-124,207-242 (mean, var, ratio_lambda).  Third-party arithmetic (statrs Poisson::cdf, fastrand) is
// restated from its published definition and is "parity unpinned" (DESIGN.md §2).
#include <algorithm>
#include <array>
#include <cmath>

#include "sylph_host.hpp"

namespace sylph_host {

// statrs 0.16.1 Poisson::cdf(x) = gamma_ur(x + 1, lambda): regularised upper incomplete gamma Q(a, x).
static double gamma_q(double a, double x) {
    if (x <= 0.0) return 1.0;
    const double gln = std::lgamma(a);
    if (x < a + 1.0) {
        double ap = a, sum = 1.0 / a, del = sum;
        for (int n = 0; n < 100000; n++) {
            ap += 1.0;
            del *= x / ap;
            sum += del;
            if (std::fabs(del) < std::fabs(sum) * 1e-17) break;
        }
        return 1.0 - sum * std::exp(-x + a * std::log(x) - gln);
    }
    const double tiny = 1e-300;
    double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
    for (int i = 1; i < 100000; i++) {
        const double an = -(double)i * ((double)i - a);
        b += 2.0;
        d = an * d + b;
        if (std::fabs(d) < tiny) d = tiny;
        c = b + an / c;
        if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) < 1e-16) break;
    }
    return std::exp(-x + a * std::log(x) - gln) * h;
}
double poisson_cdf(double lambda, uint64_t x) { return gamma_q((double)x + 1.0, lambda); }

// A histogram of coverage values -> what ratio_lambda and ani_from_lambda read off it (csrc/bootstrap_plan.h: the device counts the
// resamples of the bootstrap into the same five numbers)
using bootstrap_plan::Summary;
using row_stats_plan::RowSummary;
namespace {
// hist[v] = how often v occurs; one bin beyond the largest value, so that hist[mode + 1] is there
Summary summary_of(const std::vector<uint32_t>& hist) { return bootstrap_plan::summary_of_histogram(hist.data(), (uint32_t)hist.size()); }
Summary summary_of_values(const uint32_t* v, size_t n) {
    uint32_t top = 0;
    for (size_t i = 0; i < n; i++) top = std::max(top, v[i]);
    if (top < (1u << 16)) {
        std::vector<uint32_t> hist((size_t)top + 2, 0);
        for (size_t i = 0; i < n; i++) hist[v[i]]++;
        return summary_of(hist);
    }
    std::map<uint32_t, uint32_t> count_map;                                  // (values no histogram should be sized for)
    Summary s{0, 0, 0, 0, 0};
    for (size_t i = 0; i < n; i++) if (v[i]) count_map[v[i]]++;
    for (const auto& kv : count_map) {
        s.n_nonzero += kv.second;
        if (s.n_distinct < 2) s.n_distinct++;
        if (kv.second >= s.mode_count) { s.mode = kv.first; s.mode_count = kv.second; }
    }
    const auto it = s.mode_count ? count_map.find(s.mode + 1) : count_map.end();
    s.next_count = it == count_map.end() ? 0 : it->second;
    return s;
}
}  // namespace

// inference.rs:207-242
std::optional<double> lambda_from_summary(const Summary& s, double min_count_correct) {
    if (s.n_distinct == 1) return std::nullopt;                              // :221
    if (s.n_nonzero < SAMPLE_SIZE_CUTOFF) return std::nullopt;               // :225
    // :228-230: sort (count, value) descending and take the first = the mode, ties to the larger value
    if (s.next_count == 0) return std::nullopt;                              // :231
    const double count_p1 = (double)s.next_count, count = (double)s.mode_count;
    if (count_p1 < min_count_correct || count < min_count_correct) return std::nullopt;   // :236
    return count_p1 / count * (double)((uint64_t)s.mode + 1);                // :239
}
std::optional<double> ratio_lambda(const std::vector<uint32_t>& full_covs, double min_count_correct) {
    return lambda_from_summary(summary_of_values(full_covs.data(), full_covs.size()), min_count_correct);
}

// contain.rs:817-847
std::optional<double> ani_from_counts(std::optional<double> lambda, double k, size_t contain_count, size_t n_total) {
    if (!lambda) return std::nullopt;
    const double adj_index = (double)contain_count / (1. - std::exp(-*lambda)) / (double)n_total;
    const double ani = std::pow(adj_index, 1. / k);
    if (ani < 0. || std::isnan(ani)) return std::nullopt;
    return ani;
}
std::optional<double> ani_from_lambda(std::optional<double> lambda, double k, const std::vector<uint32_t>& full_cov) {
    if (!lambda) return std::nullopt;
    size_t contain_count = 0;
    for (uint32_t x : full_cov) if (x != 0) contain_count++;
    return ani_from_counts(lambda, k, contain_count, full_cov.size());
}

// fastrand 2.1.1 (third party): WyRand step + Lemire bounded integers; `fastrand::seed(7)` (contain.rs:854).  The step and the
// bounded integer are bootstrap_plan.h's; the loop that draws again after a rejection is the host's alone.
namespace {
struct WyRand {
    uint64_t s;
    uint64_t next() {
        s += bootstrap_plan::WY_ADD;
        return bootstrap_plan::wyrand_output(s);
    }
    uint64_t below(uint64_t n) {   // usize(..n)
        bool rejected;
        uint64_t hi = bootstrap_plan::bounded(next(), n, &rejected);
        while (rejected) hi = bootstrap_plan::bounded(next(), n, &rejected);
        return hi;
    }
};
}  // namespace

// contain.rs:849-898 (default estimator only), behind the resampling: lambda and ANI of every resample from its counts, the 5th and
// 95th percentile of those that have both
void finish_ci(const Summary* summaries, size_t iters, size_t n_total, double k, const ContainArgs& args, AniResult& out) {
    std::vector<double> res_ani, res_lambda;
    for (size_t it = 0; it < iters; it++) {
        const auto lambda = lambda_from_summary(summaries[it], args.min_count_correct);
        const auto ani = ani_from_counts(lambda, k, summaries[it].n_nonzero, n_total);
        if (ani && lambda && !std::isnan(*ani) && !std::isnan(*lambda)) { res_ani.push_back(*ani); res_lambda.push_back(*lambda); }
    }
    std::sort(res_ani.begin(), res_ani.end());
    std::sort(res_lambda.begin(), res_lambda.end());
    if (res_ani.size() < 50) return;
    const size_t suc = res_ani.size();
    out.ani_ci_lo = res_ani[suc * 5 / 100 - 1];
    out.ani_ci_hi = res_ani[suc * 95 / 100 - 1];
    out.lambda_ci_lo = res_lambda[suc * 5 / 100 - 1];
    out.lambda_ci_hi = res_lambda[suc * 95 / 100 - 1];
}

// the resampling on the host: one stream seeded with BOOTSTRAP_SEED, BOOTSTRAP_ITERS resamples of n_total draws each
void bootstrap_host(const uint32_t* kept, size_t keep, size_t n_total, double k, const ContainArgs& args, AniResult& out) {
    WyRand rng{BOOTSTRAP_SEED};
    uint32_t top = 0;
    for (size_t i = 0; i < keep; i++) top = std::max(top, kept[i]);
    std::vector<Summary> summaries(BOOTSTRAP_ITERS);
    if (top < (1u << 16)) {
        std::vector<uint32_t> hist((size_t)top + 2);
        for (auto& s : summaries) {
            std::fill(hist.begin(), hist.end(), 0u);
            for (size_t i = 0; i < n_total; i++) hist[bootstrap_plan::value_of_draw(rng.below(n_total), n_total, keep, kept)]++;
            s = summary_of(hist);
        }
    } else {
        std::vector<uint32_t> rand_vec(n_total);
        for (auto& s : summaries) {
            for (size_t i = 0; i < n_total; i++) rand_vec[i] = bootstrap_plan::value_of_draw(rng.below(n_total), n_total, keep, kept);
            s = summary_of_values(rand_vec.data(), n_total);
        }
    }
    finish_ci(summaries.data(), summaries.size(), n_total, k, args, out);
}

// The table behind the Poisson cut (contain.rs:666-675; csrc/row_stats_plan.h), from this file's own poisson_cdf, once
const uint32_t* row_cut_table() {
    static const std::array<uint32_t, row_stats_plan::CUT_ENTRIES> table = [] {
        std::array<uint32_t, row_stats_plan::CUT_ENTRIES> t{};
        row_stats_plan::build_cut_table([](uint32_t m, uint32_t x) { return poisson_cdf((double)m, x) < CUTOFF_PVALUE; }, t.data());
        return t;
    }();
    return table.data();
}
static_assert(row_stats_plan::SAMPLE_SIZE_CUTOFF == SAMPLE_SIZE_CUTOFF && (double)row_stats_plan::MEDIAN_LAMBDA_MAX == MEDIAN_ANI_THRESHOLD,
              "the plan's reject follows these constants");

// what the device needs to drop the rows that cannot pass the ANI cut of `args` (csrc/row_stats_plan.h surely_rejected)
sylph_row_filter row_filter_for(const ContainArgs& args, uint64_t k) {
    sylph_row_filter f{};
    f.struct_size = sizeof(f);
    f.k = (uint32_t)k;
    const double min_ani = args.minimum_ani ? *args.minimum_ani / 100. : (args.pseudotax ? MIN_ANI_P_DEF : MIN_ANI_DEF);
    f.reject_below = min_ani > 0. ? std::pow(min_ani, (double)k) * (1. - std::ldexp(1., -30)) : 0.;
    f.min_count_correct = args.min_count_correct;
    f.no_adj = args.no_adj ? 1 : 0;
    std::copy(row_cut_table(), row_cut_table() + row_stats_plan::CUT_ENTRIES, f.cut);
    return f;
}

// contain.rs:657-813 up to the decision about the confidence interval, from the integers a sorted row comes down to (:657-690;
// csrc/row_stats_plan.h RowSummary, counted here by stats_head or on the device by csrc/row_stats.hip): the f64 half
StatsHead stats_head_from_summary(const ContainArgs& args, const RowSummary& s, size_t n_genome_kmers, uint64_t k, std::optional<size_t> kmers_lost) {
    StatsHead h;
    if (s.contain_count == 0) return h;                                      // :654
    const size_t contain_count = s.contain_count;
    AniResult r;
    r.naive_ani = std::pow((double)contain_count / (double)n_genome_kmers, 1. / (double)k);   // :657-660
    const double median_cov = (double)s.median;                              // :663
    // full_covs (:679-684) = n_genome_kmers - contain_count zeros, then the values the Poisson cut (:666-675) keeps: a prefix of the sorted values
    const size_t keep = s.keep;
    const size_t n_total = n_genome_kmers - contain_count + keep;
    const double geq1_mean_cov = (double)s.sum / (double)contain_count;      // :690 (iter().sum::<u32>())
    Summary whole{0, 0, 0, 0, 0};                                            // of full_covs; read only where a lambda is estimated
    std::optional<double> test_lambda;
    if (median_cov > MEDIAN_ANI_THRESHOLD) r.lambda_status = AdjustStatus::High;   // :692-694
    else {
        whole = Summary{s.keep, s.n_distinct, s.mode, s.mode_count, s.next_count};
        test_lambda = lambda_from_summary(whole, args.min_count_correct);    // :695-713 (default estimator)
        r.lambda_status = test_lambda ? AdjustStatus::Lambda : AdjustStatus::Low;
        if (test_lambda) r.lambda = *test_lambda;
    }
    if (r.lambda_status == AdjustStatus::Lambda) r.final_est_cov = r.lambda;                    // :717-728
    else if (median_cov < MAX_MEDIAN_FOR_MEAN_FINAL_EST) r.final_est_cov = geq1_mean_cov;
    else r.final_est_cov = args.mean_coverage ? geq1_mean_cov : median_cov;
    std::optional<double> opt_lambda;                                        // :730-735
    if (r.lambda_status == AdjustStatus::Lambda) opt_lambda = r.final_est_cov;
    const auto opt_est_ani = ani_from_counts(opt_lambda, (double)k, whole.n_nonzero, n_total);   // :737
    r.final_est_ani = (!opt_lambda || !opt_est_ani || args.no_adj) ? r.naive_ani : *opt_est_ani;   // :739-744
    const double min_ani = args.minimum_ani ? *args.minimum_ani / 100. : (args.pseudotax ? MIN_ANI_P_DEF : MIN_ANI_DEF);
    if (r.final_est_ani < min_ani) {                                         // :746-764
        h.rejected = true;
        h.rejected_ani = r.final_est_ani;
        h.rejected_contain_count = contain_count;
        return h;
    }
    h.want_ci = !args.no_ci && opt_lambda;                                   // :766-773
    h.keep = keep;
    h.n_total = n_total;
    r.mean_cov = geq1_mean_cov;                                              // AniResult.mean_cov (:795)
    r.median_cov = median_cov;
    r.contain_count = contain_count;
    r.n_kmers = n_genome_kmers;
    r.kmers_lost = kmers_lost;
    h.result = r;
    return h;
}

// the same from the row: summarise it here (:661-690, the integer half), then the f64 half above
StatsHead stats_head(const ContainArgs& args, std::vector<uint32_t>& covs, size_t n_genome_kmers, uint64_t k, std::optional<size_t> kmers_lost) {
    if (covs.empty()) return StatsHead{};                                    // :654
    if (!std::is_sorted(covs.begin(), covs.end())) std::sort(covs.begin(), covs.end());   // :661 (already sorted when they come from the GPU)
    return stats_head_from_summary(args, row_stats_plan::summarise_row(covs.data(), (uint32_t)covs.size(), row_cut_table()), n_genome_kmers, k, kmers_lost);
}

// contain.rs:657-813
std::optional<AniResult> stats_from_covs(const ContainArgs& args, std::vector<uint32_t> covs, size_t n_genome_kmers, uint64_t k,
                                         std::optional<size_t> kmers_lost) {
    StatsHead h = stats_head(args, covs, n_genome_kmers, k, kmers_lost);
    if (h.result && h.want_ci) bootstrap_host(covs.data(), h.keep, h.n_total, (double)k, args, *h.result);
    return h.result;
}

}  // namespace sylph_host
