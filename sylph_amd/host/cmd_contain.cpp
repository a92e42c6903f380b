// cmd_contain.cpp — the `query` / `profile` command (contain.rs:115-351): the database made resident on the device, raw samples
// sketched and probed through the library's pipeline, the statistics on the containment results, the reference's TSV rows.
#include <cmath>
#include <cstring>

#include "host_internal.hpp"
#include "ordered_ahead.hpp"

namespace sylph_host {

namespace {

// contain.rs:18-94
void print_ani_result(const AniResult& r, const std::string& seq_name, const GenomeSketch& g, bool pseudotax, FILE* out,
                      bool debug_f64 = false) {
    if (debug_f64) {   // --debug-f64 (not in the reference): every float column as %.17g, unclamped, for 1e-6 parity checks
        auto opt = [](const std::optional<double>& v) { char b[40]; if (v) snprintf(b, sizeof(b), "%.17g", *v); else snprintf(b, sizeof(b), "NA"); return std::string(b); };
        fprintf(out, "%s\t%s\t", seq_name.c_str(), g.file_name.c_str());
        if (pseudotax) fprintf(out, "%.17g\t%.17g\t", *r.rel_abund, *r.seq_abund);
        fprintf(out, "%.17g\t%.17g\t%s-%s\t", r.final_est_ani * 100., r.final_est_cov, opt(r.ani_ci_lo).c_str(), opt(r.ani_ci_hi).c_str());
        if (r.lambda_status == AdjustStatus::Lambda) fprintf(out, "%.17g\t", r.lambda);
        else fprintf(out, "%s\t", r.lambda_status == AdjustStatus::High ? "HIGH" : "LOW");
        fprintf(out, "%s-%s\t%.17g\t%.17g\t%zu/%zu\t%.17g\t", opt(r.lambda_ci_lo).c_str(), opt(r.lambda_ci_hi).c_str(), r.median_cov,
                r.mean_cov, r.contain_count, r.n_kmers, r.naive_ani * 100.);
        if (pseudotax) fprintf(out, "%zu\t", *r.kmers_lost);
        fprintf(out, "%s\n", g.first_contig_name.c_str());
        return;
    }
    char final_ani[64];
    snprintf(final_ani, sizeof(final_ani), "%.2f", std::min(r.final_est_ani * 100., 100.));
    char lambda_print[64];
    if (r.lambda_status == AdjustStatus::Lambda) snprintf(lambda_print, sizeof(lambda_print), "%.3f", r.lambda);
    else snprintf(lambda_print, sizeof(lambda_print), "%s", r.lambda_status == AdjustStatus::High ? "HIGH" : "LOW");
    char ci_ani[64] = "NA-NA", ci_lambda[64] = "NA-NA";
    if (r.ani_ci_lo && r.ani_ci_hi) snprintf(ci_ani, sizeof(ci_ani), "%.2f-%.2f", *r.ani_ci_lo * 100., *r.ani_ci_hi * 100.);
    if (r.lambda_ci_lo && r.lambda_ci_hi) snprintf(ci_lambda, sizeof(ci_lambda), "%.2f-%.2f", *r.lambda_ci_lo, *r.lambda_ci_hi);
    if (!pseudotax) {
        fprintf(out, "%s\t%s\t%s\t%.3f\t%s\t%s\t%s\t%.0f\t%.3f\t%zu/%zu\t%.2f\t%s\n", seq_name.c_str(), g.file_name.c_str(),
                final_ani, r.final_est_cov, ci_ani, lambda_print, ci_lambda, r.median_cov, r.mean_cov, r.contain_count, r.n_kmers,
                r.naive_ani * 100., g.first_contig_name.c_str());
    } else {
        fprintf(out, "%s\t%s\t%.4f\t%.4f\t%s\t%.3f\t%s\t%s\t%s\t%.0f\t%.3f\t%zu/%zu\t%.2f\t%zu\t%s\n", seq_name.c_str(),
                g.file_name.c_str(), *r.rel_abund, *r.seq_abund, final_ani, r.final_est_cov, ci_ani, lambda_print, ci_lambda,
                r.median_cov, r.mean_cov, r.contain_count, r.n_kmers, r.naive_ani * 100., *r.kmers_lost,
                g.first_contig_name.c_str());
    }
}

void print_header(bool pseudotax, FILE* out, bool estimate_unknown) {         // contain.rs:461-480
    if (!pseudotax)
        fprintf(out, "Sample_file\tGenome_file\tAdjusted_ANI\tEff_cov\tANI_5-95_percentile\tEff_lambda\tLambda_5-95_percentile\t"
                     "Median_cov\tMean_cov_geq1\tContainment_ind\tNaive_ANI\tContig_name\n");
    else
        fprintf(out, "Sample_file\tGenome_file\tTaxonomic_abundance\tSequence_abundance\tAdjusted_ANI\t%s\tANI_5-95_percentile\t"
                     "Eff_lambda\tLambda_5-95_percentile\tMedian_cov\tMean_cov_geq1\tContainment_ind\tNaive_ANI\tkmers_reassigned\t"
                     "Contig_name\n", estimate_unknown ? "True_cov" : "Eff_cov");
}

}  // namespace

// --estimate-unknown (-u), contain.rs:901-951 get_kmer_identity: k-mer identity of the reads (identity ^ k) from the share of
// multiplicity-1 k-mers.  The estimate itself (eps) is a sum over the table.  The reference's "continuous median" of the counts
// above 1 is a walk over `kmer_counts.values()` in hashbrown's iteration order, which this host does not reproduce: here the
// walk goes over the table in ascending k-mer order (an arbitrary order with respect to the counts, as the hash map's is).
// It only decides whether a short-read sample counts as "depth < 3" and gets the fixed 99.5 % identity — a sample right at
// that limit may take the other branch than `sylph profile -u` does; -I (contain.rs:275) bypasses the walk altogether.
// The integer types are the reference's: `num_not1s` is a u32 that wraps in a release build.
//
// Two halves.  The walks over the counts (table_summary_host; on the device's road csrc/table_summary.hip counts the same integers
// where the table lies: unknown_from_device) and the decision in f64 (kmer_identity_from_summary): both roads go through the one tail.
UnknownSummary table_summary_host(const std::vector<uint32_t>& counts) {
    UnknownSummary s;
    uint32_t median = 0;
    double mov_avg_median = 0., n = 1.;
    for (const uint32_t count : counts) {
        if (count > 1) {
            if (count > median) median += 1; else median -= 1;
            mov_avg_median += (double)median;
            n += 1.;
        }
    }
    s.mov_avg_median = mov_avg_median / n;
    for (const uint32_t count : counts) {
        if (count == 1) s.num_1s += 1; else s.num_not1s += count;
    }
    for (const uint32_t count : counts) s.total_counts += count;     // contain.rs:392-408's own walk
    return s;
}
// median_sum < 2^53 (a summary at or above that declines): the f64 additions above are exact on the same integers, so the quotient
// is the host's, bit for bit; 1 + steps <= 2^31 is exact as well
UnknownSummary unknown_from_device(const sylph_table_summary_t& d) {
    UnknownSummary s;
    s.mov_avg_median = (double)d.median_sum / (1. + (double)d.steps);
    s.num_1s = (int32_t)d.num_1s;
    s.num_not1s = d.num_not1s;
    s.total_counts = d.total_counts;
    return s;
}
std::optional<double> get_kmer_identity(const SequencesSketch& S, bool estimate_unknown) {
    if (!estimate_unknown) return std::nullopt;
    return kmer_identity_from_summary(table_summary_host(S.counts), S.k, S.mean_read_length, S.file_name);
}
double kmer_identity_from_summary(const UnknownSummary& s, uint64_t k, double mean_read_length, const std::string& file_name) {
    const struct { const std::string& file_name; double mean_read_length; uint64_t k; } S{file_name, mean_read_length, k};
    const double mov_avg_median = s.mov_avg_median;
    const double eps = (double)s.num_not1s / ((double)s.num_not1s + (double)s.num_1s + 0.1);
    {   // which branch the walk chose, and how close the call was (the walk's order is this host's, not hashbrown's: see above).
        // The reference prints neither line: the first only under SYLPH_HIP_DEBUG, the warning only inside the 10 % band.
        const bool near_limit = S.mean_read_length < 400. && std::fabs(mov_avg_median - MED_KMER_FOR_ID_EST) <= 0.1 * MED_KMER_FOR_ID_EST;
        if (getenv("SYLPH_HIP_DEBUG")) {
            char num[160];
            snprintf(num, sizeof(num), " --estimate-unknown: running median of the counts above 1 = %.4f (limit %.1f, mean read length %.1f): ",
                     mov_avg_median, MED_KMER_FOR_ID_EST, S.mean_read_length);
            info(S.file_name + num + ((mov_avg_median < MED_KMER_FOR_ID_EST && S.mean_read_length < 400.) ? "fixed 99.5% read identity" : "read identity estimated from the table"));
        }
        if (near_limit)
            warn(S.file_name + ": the sample's depth is within 10% of the limit that switches --estimate-unknown between the fixed 99.5% read identity and "
                 "the estimated one; that decision depends on the order the table is walked in (ascending k-mers here, hash-map order in "
                 "sylph), so True_cov / Sequence_abundance may differ from `sylph profile -u` for this sample: pass -I to fix the identity");
    }
    if (mov_avg_median < MED_KMER_FOR_ID_EST && S.mean_read_length < 400.) {
        info(S.file_name + " short-read sample has high diversity compared to sequencing depth (approx. avg depth < 3). Using 99.5% as "
             "read accuracy estimate instead of automatic detection for --estimate-unknown.");
        return std::pow(0.995, (double)S.k);
    }
    return eps < 1. ? eps : 1.;
}

// contain.rs:377-390
void estimate_true_cov(std::vector<AniResult>& results, std::optional<double> kmer_id_opt, bool estimate_unknown, double read_length,
                       uint64_t k) {
    double multiplier = 1.;
    if (estimate_unknown) multiplier = read_length / (read_length - (double)k + 1.);
    if (estimate_unknown && kmer_id_opt)
        for (auto& r : results) r.final_est_cov = r.final_est_cov / *kmer_id_opt * multiplier;
}

// contain.rs:392-408: share of the sample's bases the profiled genomes account for
double estimate_covered_bases(const std::vector<AniResult>& results, const std::vector<GenomeSketch>& genomes, uint64_t c, uint64_t num_total_counts,
                              double read_length, uint64_t k) {
    const double multiplier = read_length / (read_length - (double)k + 1.);
    double num_covered_bases = 0.;
    for (const auto& r : results) num_covered_bases += (double)genomes[r.genome_index].gn_size * r.final_est_cov;
    const double num_tentative_bases = (double)(c * num_total_counts) * multiplier;
    if (num_tentative_bases == 0.) return 0.;
    return std::min(num_covered_bases / num_tentative_bases, 1.);
}

namespace {
struct UploadGuard { sylph_upload* u = nullptr; ~UploadGuard() { sylph_upload_destroy(u); } };
// The genomes' k-mers (tracked: their pseudotax_tracked_nonused_kmers) go from where they lie — the mapped .syldb files (views), or
// the vectors of genomes sketched in this run — through the library's page-locked upload chunks to the device, gathered by all
// parse threads: no per-genome vector, no flat host copy, the copy of one chunk travels while the next is gathered (round 4;
// rounds 1-3: 113,104 vectors + one 11 GB concatenation + a staged pageable copy).  off: the genomes' offsets in the flat array.
const uint64_t* upload_gathered(sylph_ctx* ctx, const std::vector<GenomeSketch>& genome_sketches, bool tracked, std::vector<uint64_t>& off,
                                UploadGuard& guard) {
    off.assign(1, 0);
    for (const auto& g : genome_sketches) off.push_back(off.back() + (tracked ? g.n_tracked() : g.n_kmers()));
    const uint64_t total = off.back() * 8;
    sylph_upload* up = nullptr;
    hip_check(sylph_upload_begin(ctx, total, 256ull << 20, &up), "sylph_upload_begin");
    guard.u = up;
    const unsigned T = std::max(1u, parse_threads());
    uint64_t at = 0;                                   // bytes of the flat array gathered so far
    size_t g0 = 0;                                     // first genome that still has bytes to give
    while (at < total) {
        void* chunk = nullptr;
        uint64_t cap = 0;
        hip_check(sylph_upload_chunk(up, &chunk, &cap), "sylph_upload_chunk");
        const uint64_t n = std::min<uint64_t>(cap & ~7ull, total - at);
        std::vector<std::thread> th;
        std::exception_ptr err;
        auto piece = [&](unsigned w) {
            const uint64_t b0 = at + n / T * w / 8 * 8, b1 = w + 1 == T ? at + n : at + n / T * (w + 1) / 8 * 8;
            size_t g = (size_t)(std::upper_bound(off.begin() + (long)g0, off.end(), b0 / 8) - off.begin()) - 1;   // genome holding byte b0
            for (uint64_t b = b0; b < b1;) {
                while (off[g + 1] * 8 <= b) g++;
                const GenomeSketch& gs = genome_sketches[g];
                const uint8_t* src = tracked ? gs.tracked_bytes() : gs.kmers_bytes();
                const uint64_t in_g = b - off[g] * 8, len = std::min<uint64_t>(off[g + 1] * 8 - b, b1 - b);
                memcpy((uint8_t*)chunk + (b - at), src + in_g, len);
                b += len;
            }
        };
        for (unsigned w = 1; w < T; w++) th.emplace_back(piece, w);
        piece(0);
        for (auto& t : th) t.join();
        hip_check(sylph_upload_commit(up, n), "sylph_upload_commit");
        at += n;
        while (g0 + 1 < off.size() && off[g0 + 1] * 8 <= at) g0++;
    }
    const void* dev = nullptr;
    hip_check(sylph_upload_finish(up, &dev), "sylph_upload_finish");
    return (const uint64_t*)dev;
}
// an offsets array travels the same way (a few hundred KB)
const uint64_t* upload_offsets(sylph_ctx* ctx, const std::vector<uint64_t>& off, UploadGuard& guard) {
    hip_check(sylph_upload_begin(ctx, off.size() * 8, 1u << 20, &guard.u), "sylph_upload_begin");
    for (size_t i = 0; i < off.size();) {
        void* chunk = nullptr;
        uint64_t cap = 0;
        hip_check(sylph_upload_chunk(guard.u, &chunk, &cap), "sylph_upload_chunk");
        const size_t m = std::min<size_t>(off.size() - i, cap / 8);
        memcpy(chunk, off.data() + i, m * 8);
        hip_check(sylph_upload_commit(guard.u, m * 8), "sylph_upload_commit");
        i += m;
    }
    const void* dev = nullptr;
    hip_check(sylph_upload_finish(guard.u, &dev), "sylph_upload_finish");
    return (const uint64_t*)dev;
}

// --log-reassignments, contain.rs:432-456: the passing genomes by index, then how many k-mers of which genome the winner table
// hands to which other one.  The device holds the winner table (resident indexes + the passing list); the host gathers its copy
// of the passing genomes' k-mers — out of the mapping, which is unaligned: memcpy — into one buffer, in the order of `stats`, and
// sylph_db_reassign_edges counts.  The reference prints an edge when its count is above 10, in its hash map's order; here the
// edges come sorted by (loser, winner).  The block is ONE write.
void log_reassignment_edges(const std::vector<GenomeSketch>& genome_sketches, const std::vector<AniResult>& stats, const std::vector<uint32_t>& pg,
                            const std::vector<double>& pa, uint64_t threads, sylph_db* rdb) {
    std::vector<uint64_t> off(stats.size() + 1, 0);
    for (size_t i = 0; i < stats.size(); i++) off[i + 1] = off[i] + genome_sketches[stats[i].genome_index].n_kmers();
    std::vector<uint64_t> kmers(off.back());
    parallel_for(stats.size(), threads, [&](size_t i) {
        const GenomeSketch& g = genome_sketches[stats[i].genome_index];
        if (g.n_kmers()) memcpy(kmers.data() + off[i], g.kmers_bytes(), g.n_kmers() * 8);
    });
    sylph_reassign_edge* edges = nullptr;
    uint64_t n_edges = 0;
    hip_check(sylph_db_reassign_edges(rdb, kmers.data(), off.data(), SYLPH_MEM_HOST, pg.data(), pa.data(), (uint32_t)pg.size(), 11, &edges, &n_edges),
              "sylph_db_reassign_edges");
    std::vector<std::string> lines{"------------- Logging k-mer reassignments -----------------"};
    for (size_t i = 0; i < stats.size(); i++) {
        const GenomeSketch& g = genome_sketches[stats[i].genome_index];
        lines.push_back("Index\t" + std::to_string(i) + "\t" + g.file_name + "\t" + g.first_contig_name);
    }
    for (uint64_t e = 0; e < n_edges; e++)
        lines.push_back(std::to_string(edges[e].winner) + "->" + std::to_string(edges[e].loser) + "\t" + std::to_string(edges[e].count) + "\tkmers reassigned");
    sylph_free(edges);
    info_block(lines);
}

// ---- one sample's results -> statistics -> (profile: reassignment pass) -> TSV rows.  The first pass's rows come as FirstPass,
// the sample's table where it lies as SampleTable; S carries the metadata, and the counts on the host when -u needs them.
struct ReportTo {   // what every sample's report shares
    const ContainCmdArgs& args;
    const std::vector<GenomeSketch>& genome_sketches;   // the database, in the order of its device-side index
    FILE* out;
    sylph_ctx* ctx;                                     // the command's own context: the genomes' confidence intervals are resampled on it
};
// The road of the first pass's statistics head.  Host: every row with a hit is walked on this thread (stats_head).  Device: the
// pipeline summarises the rows on the device and hands over the candidates only (sylph_pipeline_set_row_filter; csrc/row_stats.hip),
// the f64 half runs here on their summaries (stats_head_from_summary) — same output, bit for bit.  SYLPH_HIP_STATS_DEVICE = 0 | 1 |
// only (only: a sample that cannot take the device's road is an Error).  The project's ship rule decides the default: on only where
// whole `profile` and `query` commands beat the parent commit's binary by more than both spreads — profiles/row_stats.txt holds the
// record: 2.0x and 2.4x over 64 sketches against 20,000 genomes, so unset means 1.
enum class StatsRoute { Host, Device, DeviceOnly };
constexpr StatsRoute STATS_ROUTE_DEFAULT = StatsRoute::Device;
StatsRoute stats_route() {
    const char* e = getenv("SYLPH_HIP_STATS_DEVICE");
    if (!e || !*e) return STATS_ROUTE_DEFAULT;
    if (!strcmp(e, "0")) return StatsRoute::Host;
    if (!strcmp(e, "1")) return StatsRoute::Device;
    if (!strcmp(e, "only")) return StatsRoute::DeviceOnly;
    throw Error{1, std::string("SYLPH_HIP_STATS_DEVICE must be 0, 1 or only, not ") + e};
}
// The road of --estimate-unknown's walks over a sample's counts.  Host: the pipeline copies every table to the host (want_table) and
// this thread walks the counts (table_summary_host).  Device: the pipeline's profile thread counts the walks' integers where the table
// lies (the option "table_summary"; csrc/table_summary.hip) and nothing of the table travels; a summary that declines brings the
// counts along and they are walked here.  SYLPH_HIP_UNKNOWN_DEVICE = 0 | 1 | only (only: a declined summary is an Error).  Same
// output, bit for bit.  The project's ship rule decides the default — on only where whole `profile -u` and `query -u` commands beat
// the parent commit's binary by more than both spreads: in profiles/table_summary.txt's record the device's road was faster in every
// pair (1.08x and 1.18x over 64 sketches), `profile -u` beyond the spreads and `query -u` not, so unset means 0.
enum class UnknownRoute { Host, Device, DeviceOnly };
constexpr UnknownRoute UNKNOWN_ROUTE_DEFAULT = UnknownRoute::Host;
UnknownRoute unknown_route() {
    const char* e = getenv("SYLPH_HIP_UNKNOWN_DEVICE");
    if (!e || !*e) return UNKNOWN_ROUTE_DEFAULT;
    if (!strcmp(e, "0")) return UnknownRoute::Host;
    if (!strcmp(e, "1")) return UnknownRoute::Device;
    if (!strcmp(e, "only")) return UnknownRoute::DeviceOnly;
    throw Error{1, std::string("SYLPH_HIP_UNKNOWN_DEVICE must be 0, 1 or only, not ") + e};
}
// the candidates of a sample (sylph_pipeline_rows_of_last)
struct Candidates {
    const sylph_row_summary* rows = nullptr;
    uint32_t n = 0;
    const uint64_t* off = nullptr;
    const void* covs = nullptr;
    uint32_t width = 0;
};
// SYLPH_HIP_FEED_TRACE: one line per sample — the road of its first statistics pass and what it walked.  The device's road brings
// only the candidates to the host: the number of rows with hits stays on the device.
void trace_stats_road(const std::string& sample, const char* road, size_t rows_with_hits, bool hits_known, size_t candidates) {
    if (!FeedLaps::on()) return;
    if (hits_known) fprintf(stderr, "[sylph_hip feed] stats %s: road %s, %zu rows with hits, %zu candidates\n", sample.c_str(), road, rows_with_hits, candidates);
    else fprintf(stderr, "[sylph_hip feed] stats %s: road %s, %zu candidates\n", sample.c_str(), road, candidates);
}

// The first pass's rows: the whole view of the probe (`cc / coff / covs`, values `width` bytes each), or — `cand` set, the rest
// null — the device's road: the candidates alone, summarised there.
struct FirstPass {
    const uint32_t* cc = nullptr;
    const uint64_t* coff = nullptr;
    const void* covs = nullptr;
    uint32_t width = 0;
    const Candidates* cand = nullptr;
};
// The sample's table where it lies (tmem: SYLPH_MEM_*), for the reassignment probe
struct SampleTable {
    const uint64_t* tk;
    const uint32_t* tc;
    uint64_t tn;
    int tmem;
};
// One row of a statistics pass: its genome, its [lo, hi) in the pass's coverage values, and the integers it comes down to
struct StatsRow {
    size_t genome;
    uint64_t lo, hi;
    row_stats_plan::RowSummary summary;
};

// unknown: with -u, what the walks over the sample's counts came down to on the device; none: they run here, over S.counts
void report(const ReportTo& to, const SequencesSketch& S, const std::string& first_file, const FirstPass& first, const SampleTable& table, sylph_db* rdb,
            const std::optional<UnknownSummary>& unknown = std::nullopt) {
    const ContainCmdArgs& args = to.args;
    const std::vector<GenomeSketch>& genome_sketches = to.genome_sketches;
    FILE* const out = to.out;
    if (genome_sketches[0].k != S.k) throw Error{1, "k parameter for reads != k parameter for genome"};   // contain.rs:608-615
    const std::string seq_name = S.sample_name ? *S.sample_name : S.file_name;   // :775-781
    // a row of the host's: summarised here, as stats_head does (contain.rs:654, :661)
    auto host_row = [&](size_t g, const void* base, uint32_t width, const uint64_t* off) {
        StatsRow r{g, off[g], off[g + 1], {}};
        std::vector<uint32_t> cv(r.hi - r.lo);
        if (width == 4) memcpy(cv.data(), (const uint32_t*)base + r.lo, (r.hi - r.lo) * 4);
        else if (width == 2) for (uint64_t i = r.lo; i < r.hi; i++) cv[i - r.lo] = ((const uint16_t*)base)[i];
        else for (uint64_t i = r.lo; i < r.hi; i++) cv[i - r.lo] = ((const uint8_t*)base)[i];
        if (cv.empty()) return r;
        if (!std::is_sorted(cv.begin(), cv.end())) std::sort(cv.begin(), cv.end());
        r.summary = row_stats_plan::summarise_row(cv.data(), (uint32_t)cv.size(), row_cut_table());
        return r;
    };
    // The statistics of different genomes are independent (contain.rs:284 runs them on the rayon pool): -t threads, results in the
    // order of the rows so that the output does not depend on the interleaving.  Between the two halves of a genome's statistics lies
    // its confidence interval: the genomes that want one are resampled together (bootstrap_batch: one device call, or the host's loop).
    // `row(i)`, i < n: the pass's rows, ascending by genome and with it in the coverage values `base`; `lost`: the second pass.
    const BootstrapRoute ci_route = args.no_ci ? BootstrapRoute::Host : bootstrap_route();
    const bool log_reassign = args.pseudotax && args.log_reassignments;   // (`query` ignores the flag, as the reference does)
    auto run_stats = [&](size_t n, const void* base, uint32_t width, const uint32_t* lost, auto&& row) {
        std::vector<StatsHead> heads(n);
        std::vector<StatsRow> rows(n);
        parallel_for(n, args.threads, [&](size_t i) {
            rows[i] = row(i);
            const size_t g = rows[i].genome;
            heads[i] = stats_head_from_summary(args, rows[i].summary, genome_sketches[g].n_kmers(), S.k, lost ? std::optional<size_t>((size_t)lost[g]) : std::nullopt);
            if (heads[i].result) heads[i].result->genome_index = g;
        });
        if (lost && log_reassign) {                                  // contain.rs:749-761: passed before the reassignment, not after it
            const double min_ani = args.minimum_ani ? *args.minimum_ani / 100. : MIN_ANI_P_DEF;
            for (size_t i = 0; i < n; i++) {
                if (!heads[i].rejected) continue;
                const GenomeSketch& g = genome_sketches[rows[i].genome];
                char num[160];
                snprintf(num, sizeof(num), " has ANI = %.2f < %.2f after reassigning %zu k-mers (%zu contained k-mers after reassign)",
                         heads[i].rejected_ani * 100., min_ani * 100., (size_t)lost[rows[i].genome], heads[i].rejected_contain_count);
                info("Genome/contig " + g.file_name + "/" + g.first_contig_name + num);
            }
        }
        std::vector<CiItem> ci;
        for (size_t i = 0; i < n; i++)
            if (heads[i].result && heads[i].want_ci) ci.push_back({&*heads[i].result, rows[i].lo, rows[i].hi, heads[i].keep, heads[i].n_total});
        bootstrap_batch(to.ctx, ci_route, args, S.k, base, width, ci, args.threads);
        std::vector<std::optional<AniResult>> res(n);
        for (size_t i = 0; i < n; i++) res[i] = std::move(heads[i].result);
        return res;
    };
    std::vector<AniResult> stats;
    for (size_t g = 0; g < genome_sketches.size(); g++)
        if (genome_sketches[g].c < S.c) throw Error{1, "c parameter for reads > c parameter for genome"};   // :616-623
    if (const Candidates* cand = first.cand) {
        // the candidates' summaries came counted on the device
        for (auto& r : run_stats(cand->n, cand->covs, cand->width, nullptr, [&](size_t i) {
                 StatsRow r{0, cand->off[i], cand->off[i + 1], {}};
                 memcpy(&r.summary, &cand->rows[i], sizeof(r.summary));
                 r.genome = r.summary.row;
                 return r;
             }))
            if (r) stats.push_back(*r);
        trace_stats_road(first_file, "device", 0, false, cand->n);
    } else {
        std::vector<size_t> with_hits;
        for (size_t g = 0; g < genome_sketches.size(); g++)
            if (first.cc[g] != 0) with_hits.push_back(g);            // :654
        for (auto& r : run_stats(with_hits.size(), first.covs, first.width, nullptr, [&](size_t i) { return host_row(with_hits[i], first.covs, first.width, first.coff); }))
            if (r) stats.push_back(*r);
        trace_stats_road(first_file, "host", with_hits.size(), true, with_hits.size());
    }
    std::optional<double> kmer_id_opt;                               // contain.rs:274-281
    if (args.seq_id) kmer_id_opt = std::pow(*args.seq_id / 100., (double)S.k);
    else if (args.estimate_unknown) kmer_id_opt = kmer_identity_from_summary(unknown ? *unknown : table_summary_host(S.counts), S.k, S.mean_read_length, S.file_name);
    estimate_true_cov(stats, kmer_id_opt, args.estimate_unknown, S.mean_read_length, S.k);   // :295
    if (args.pseudotax) {
        info(first_file + " taxonomic profiling; reassigning k-mers for " + std::to_string(stats.size()) + " genomes...");
        // winner_table (contain.rs:410-430) + second get_stats pass with the winner map (:300-307, :637-646) on the
        // device: one more probe of the resident postings (genome_kmers + tracked k-mers), passing genomes only.
        std::vector<uint32_t> pg(stats.size());
        std::vector<double> pa(stats.size());
        for (size_t i = 0; i < stats.size(); i++) { pg[i] = (uint32_t)stats[i].genome_index; pa[i] = stats[i].final_est_ani; }
        if (log_reassign) log_reassignment_edges(genome_sketches, stats, pg, pa, args.threads, rdb);
        const uint32_t *cc2 = nullptr, *covs2 = nullptr, *lost2 = nullptr;
        const uint64_t* coff2 = nullptr;
        uint64_t ncov2 = 0;
        hip_check(sylph_db_reassign_view(rdb, table.tk, table.tc, table.tn, table.tmem, pg.data(), pa.data(), (uint32_t)pg.size(), &cc2, &coff2, &covs2, &ncov2, &lost2),
                  "sylph_db_reassign_view");
        std::vector<AniResult> stats2;                           // (the passing genomes are in genome order still: ascending)
        const std::vector<std::optional<AniResult>> res2 =
            run_stats(stats.size(), covs2, 4, lost2, [&](size_t i) { return host_row(stats[i].genome_index, covs2, 4, coff2); });
        for (size_t i = 0; i < stats.size(); i++) {
            const auto& r = res2[i];
            if (!r) continue;
            // derep_if_reassign_threshold, contain.rs:353-375
            const double thr = std::pow(args.redundant_ani / 100., (double)S.k) * (double)r->n_kmers;
            if ((double)(stats[i].contain_count - r->contain_count) < thr) stats2.push_back(*r);
        }
        stats.swap(stats2);
        estimate_true_cov(stats, kmer_id_opt, args.estimate_unknown, S.mean_read_length, S.k);   // :310
        info(first_file + " has " + std::to_string(stats.size()) + " genomes passing profiling threshold. ");
        double bases_explained = 1.;                                 // :313-317
        if (args.estimate_unknown) {
            const uint64_t total_counts = unknown ? unknown->total_counts : table_summary_host(S.counts).total_counts;
            bases_explained = estimate_covered_bases(stats, genome_sketches, S.c, total_counts, S.mean_read_length, S.k);
            char buf[64];
            snprintf(buf, sizeof buf, "%.2f", bases_explained * 100.);
            info(first_file + " has " + buf + "% of reads detected in database by profile");
        }
        double total_cov = 0, total_seq_cov = 0;                     // contain.rs:319-326
        for (const auto& r : stats) { total_cov += r.final_est_cov; total_seq_cov += r.final_est_cov * (double)genome_sketches[r.genome_index].gn_size; }
        for (auto& r : stats) r.rel_abund = r.final_est_cov / total_cov * 100.;
        for (auto& r : stats) r.seq_abund = r.final_est_cov * (double)genome_sketches[r.genome_index].gn_size / total_seq_cov * 100. * bases_explained;
        std::stable_sort(stats.begin(), stats.end(), [](const AniResult& x, const AniResult& y) { return *y.rel_abund < *x.rel_abund; });   // :330
    } else {
        std::stable_sort(stats.begin(), stats.end(), [](const AniResult& x, const AniResult& y) { return y.final_est_ani < x.final_est_ani; });   // :333
    }
    for (const auto& r : stats) print_ani_result(r, seq_name, genome_sketches[r.genome_index], args.pseudotax, out, args.debug_f64);
}

void finished(const std::vector<std::string>& files) {
    info(std::string(files.size() > 1 ? "Finished paired sample " : "Finished sample ") + files[0] + ".");
}

// get_genome_sketches, contain.rs:482-541: the *.syldb files as they are, the genome files sketched here
std::vector<GenomeSketch> load_genome_sketches(Engine& e, const ContainCmdArgs& args, const std::vector<std::string>& genome_sketch_files,
                                               const std::vector<std::string>& genome_files) {
    std::vector<GenomeSketch> genome_sketches;
    std::optional<uint64_t> lowest_genome_c, current_k;
    static const bool copy_load = getenv("SYLPH_HIP_DB_COPY_LOAD") != nullptr;   // A/B + tests: every genome copied into vectors first (rounds 1-3)
    for (const auto& f : genome_sketch_files) {
        auto v = copy_load ? read_syldb(f) : read_syldb_views(f);
        if (v.empty()) continue;
        const uint64_t c = v.front().c, k = v.front().k;
        if (!lowest_genome_c || *lowest_genome_c < c) lowest_genome_c = c;
        if (!current_k) current_k = k;
        else if (*current_k != k) throw Error{1, "Query sketches have inconsistent -k. Exiting."};
        for (auto& g : v) genome_sketches.push_back(std::move(g));
    }
    GenomeBatch batch(e, args.c, args.k, args.min_spacing_kmer, args.pseudotax, genome_sketches);
    std::vector<std::string> genome_files_ok;
    for (const auto& gf : genome_files) {
        if (lowest_genome_c && *lowest_genome_c < args.c) { fprintf(stderr, "ERROR [sylph_hip] Value of -c for contain is %llu -- greater than the smallest value of -c for a genome sketch %llu. Continuing without sketching.\n", (unsigned long long)args.c, (unsigned long long)*lowest_genome_c); continue; }
        if (current_k && *current_k != args.k) { fprintf(stderr, "ERROR [sylph_hip] -k %llu is not equal to -k %llu found in sketches. Continuing without sketching.\n", (unsigned long long)args.k, (unsigned long long)*current_k); continue; }
        genome_files_ok.push_back(gf);
    }
    batch.add_files(genome_files_ok, args.individual, args.threads);
    batch.flush();
    info("Finished obtaining genome sketches.");
    if (genome_sketches.empty()) throw Error{1, "No genome sketches found; see sylph query/profile -h for help. Exiting"};
    if (!genome_sketches.front().has_tracked() && args.pseudotax)
        throw Error{1, "Attempting profiling, but *.syldb was sketched with the --disable-profiling option. Exiting"};   // :234-237

    return genome_sketches;
}

// (destroyed even on the fast way out: a 29 GB index left to the driver's own clean-up at process exit is released BEHIND the
//  process — the next command's database load then took 2.7 s instead of 0.7: profiles/r05_db_load_with_forked_profile.txt)
struct DbGuard { sylph_db* d = nullptr; ~DbGuard() { sylph_db_destroy(d); } };
void upload_database(Engine& e, const std::vector<GenomeSketch>& genome_sketches, bool pseudotax, DbGuard& db) {
    // database resident in HBM (replaces the per-genome probe loop of contain.rs:284-291)
    const auto t_db0 = std::chrono::steady_clock::now();
    sylph_ctx* const ctx = e.context();
    std::vector<uint64_t> goff;
    {
        UploadGuard ug, og;
        const uint64_t* d_k = upload_gathered(ctx, genome_sketches, false, goff, ug);
        hip_check(sylph_db_upload(ctx, d_k, upload_offsets(ctx, goff, og), genome_sketches.size(), SYLPH_MEM_DEVICE, &db.d), "sylph_db_upload");
    }
    if (pseudotax) {   // the winner table also ranges over pseudotax_tracked_nonused_kmers (contain.rs:421-428)
        UploadGuard ug, og;
        std::vector<uint64_t> toff;
        const uint64_t* d_t = upload_gathered(ctx, genome_sketches, true, toff, ug);
        hip_check(sylph_db_attach_tracked(db.d, d_t, upload_offsets(ctx, toff, og), SYLPH_MEM_DEVICE), "sylph_db_attach_tracked");
    }
    if (getenv("SYLPH_HIP_FEED_TRACE") || getenv("SYLPH_HIP_DEBUG")) {
        char b[200];
        snprintf(b, sizeof(b), "timing: database of %zu genomes (%llu k-mers) uploaded and indexed in %.3f s", genome_sketches.size(),
                 (unsigned long long)goff.back(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t_db0).count());
        info(b);
    }
}

// --gpus N|all: the database replicated on N GPUs (index copied device to device), samples dealt to them, one router pipeline over
// the replicas (sylph_pipeline_create_multi): the reference's sample loop spans the machine through its rayon pool
// (contain.rs:252-295), this is the same for the GPUs of a node.  One GPU: the database as it is, a plain pipeline.
// (SYLPH_HIP_SHARE_GPUS=1: more replicas than devices — they wrap around; how the one-GPU test box runs `--gpus 2`)
// Both sample roads — raw reads and sketch files — set their replicas and their pipeline up here.
struct ReplicaSet {
    std::vector<std::unique_ptr<Engine>> engines;                    // (declared before the replicas: destroyed after them)
    std::vector<sylph_db*> dbs;                                      // dbs[0]: the command's own database, not owned
    std::vector<int> device;
    int n_gpus = 1;
    ReplicaSet(Engine& e, const ContainCmdArgs& args, sylph_db* db, size_t n_samples) {
        n_gpus = args.gpus < 0 ? sylph_device_count() : getenv("SYLPH_HIP_SHARE_GPUS") ? args.gpus : std::min(args.gpus, std::max(1, sylph_device_count()));
        n_gpus = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, n_gpus), n_samples));
        dbs.push_back(db);
        device.push_back(e.device);
        const int dev0 = e.device < 0 ? 0 : e.device;                // (Engine(-1) = the current device = 0 in a fresh process)
        const auto t_r0 = std::chrono::steady_clock::now();
        try {
            for (int g = 1; g < n_gpus; g++) {
                const int dev = (dev0 + g) % std::max(1, sylph_device_count());
                engines.emplace_back(new Engine(dev));
                sylph_db* r = nullptr;
                hip_check(sylph_db_replicate(db, engines.back()->context(), &r), "sylph_db_replicate");
                dbs.push_back(r);
                device.push_back(dev);
            }
        } catch (...) { destroy_replicas(); throw; }
        if (n_gpus > 1) {
            char b[160];
            snprintf(b, sizeof(b), "database replicated on %d GPUs (device to device) in %.3f s", n_gpus,
                     std::chrono::duration<double>(std::chrono::steady_clock::now() - t_r0).count());
            info(b);
        }
    }
    ~ReplicaSet() { destroy_replicas(); }
    ReplicaSet(const ReplicaSet&) = delete;
    ReplicaSet& operator=(const ReplicaSet&) = delete;
    void destroy_replicas() { for (size_t i = 1; i < dbs.size(); i++) sylph_db_destroy(dbs[i]); dbs.resize(std::min<size_t>(dbs.size(), 1)); }
    // the command's pipeline over the set: `n_workers` library threads, as deep as a prepare pool that runs `ahead_limit` samples
    // ahead needs (with SYLPH_HIP_STATS_DEVICE on, its profile thread also summarises the rows: `k` is the genomes')
    sylph_pipeline* create_pipeline(const ContainCmdArgs& args, uint64_t k, uint32_t n_workers, size_t ahead_limit, sylph_pipeline_config& cfg) {
        memset(&cfg, 0, sizeof(cfg));
        cfg.struct_size = sizeof(cfg);
        cfg.n_workers = n_workers;
        cfg.depth = (uint32_t)ordered_ahead::pipeline_depth(ahead_limit);
        cfg.max_batch = 4;
        cfg.c = (uint32_t)args.c; cfg.k = (uint32_t)args.k;
        cfg.reads_mode = SYLPH_READS_PAIRED; cfg.seed_mode = SYLPH_SEED_AVX2_COMPAT;
        const bool unknown_on_device = args.estimate_unknown && unknown_route() != UnknownRoute::Host;
        cfg.want_table = args.estimate_unknown && !unknown_on_device ? 1 : 0;   // -u walks the counts on the host, or (below) the device does
        cfg.min_number_kmers = args.min_number_kmers;
        sylph_pipeline* pipe = nullptr;
        if (n_gpus > 1) hip_check(sylph_pipeline_create_multi(dbs.data(), (uint32_t)dbs.size(), &cfg, &pipe), "sylph_pipeline_create_multi");
        else hip_check(sylph_pipeline_create(dbs[0], &cfg, &pipe), "sylph_pipeline_create");
        if (unknown_on_device) {
            const int rc = sylph_pipeline_set_option(pipe, "table_summary", "1");
            if (rc != SYLPH_OK) { sylph_pipeline_destroy(pipe); hip_check(rc, "sylph_pipeline_set_option"); }
        }
        if (stats_route() != StatsRoute::Host) {
            const sylph_row_filter f = row_filter_for(args, k);
            const int rc = sylph_pipeline_set_row_filter(pipe, &f);
            if (rc != SYLPH_OK) { sylph_pipeline_destroy(pipe); hip_check(rc, "sylph_pipeline_set_row_filter"); }
        }
        return pipe;
    }
};
// of the sample sylph_pipeline_next just returned, when the pipeline carries the row filter (create_pipeline); else nothing
std::optional<Candidates> candidates_of_last(sylph_pipeline* pipe) {
    if (stats_route() == StatsRoute::Host) return std::nullopt;
    Candidates c;
    hip_check(sylph_pipeline_rows_of_last(pipe, &c.rows, &c.n, &c.off, &c.covs, &c.width), "sylph_pipeline_rows_of_last");
    return c;
}
// The pipeline of a sample road (2 library workers: they finish the sessions, or unpack the entries, that the road hands over) and
// what both roads do with a result.  The replica set outlives it.
struct SamplePipe {
    ReplicaSet& replicas;
    sylph_pipeline_config cfg;
    sylph_pipeline* const p;
    SamplePipe(ReplicaSet& r, const ContainCmdArgs& args, uint64_t genome_k, size_t ahead_limit) : replicas(r), p(r.create_pipeline(args, genome_k, 2, ahead_limit, cfg)) {}
    ~SamplePipe() { sylph_pipeline_destroy(p); }
    SamplePipe(const SamplePipe&) = delete;
    SamplePipe& operator=(const SamplePipe&) = delete;
    size_t outstanding() const { return sylph_pipeline_outstanding(p); }
    // every result still outstanding is taken: nothing reads what was submitted after that
    void drain() { sylph_pipeline_result r; while (sylph_pipeline_outstanding(p) && sylph_pipeline_next(p, &r) == SYLPH_OK) {} }
    // the next sample's result, in submission order
    sylph_pipeline_result next(const std::string& file) {
        sylph_pipeline_result r;
        hip_check(sylph_pipeline_next(p, &r), "sylph_pipeline_next");
        if (r.status != SYLPH_OK) throw Error{1, std::string("sample ") + file + ": " + (r.error ? r.error : "GPU stage failed")};
        return r;
    }
    // ... -> the counts -u walks -> the candidates -> the sample's rows, reassigned on the replica that holds its table
    void report_last(const ReportTo& to, const sylph_pipeline_result& r, SequencesSketch& S, const std::string& file) {
        if (to.args.estimate_unknown && r.counts) S.counts.assign(r.counts, r.counts + r.n_table);
        std::optional<UnknownSummary> unknown;
        if (to.args.estimate_unknown && unknown_route() != UnknownRoute::Host) {
            sylph_table_summary_t s;
            hip_check(sylph_pipeline_summary_of_last(p, &s), "sylph_pipeline_summary_of_last");
            if (!(s.flags & SYLPH_TABLE_SUMMARY_DECLINED)) unknown = unknown_from_device(s);
            else if (unknown_route() == UnknownRoute::DeviceOnly)
                throw Error{1, "SYLPH_HIP_UNKNOWN_DEVICE=only: the table summary of " + file + " declined (flags " + std::to_string(s.flags) + ")"};
            if (FeedLaps::on())
                fprintf(stderr, "[sylph_hip feed] unknown %s: road %s, rung %u, %u chunks walked again\n", file.c_str(), unknown ? "device" : "host (declined)", s.rung, s.open_chunks);
        }
        const std::optional<Candidates> cand = candidates_of_last(p);
        report(to, S, file, FirstPass{r.contain_count, r.cov_off, r.covs, r.cov_width, cand ? &*cand : nullptr},
               SampleTable{r.dev_kmers, r.dev_counts, r.n_table, SYLPH_MEM_DEVICE}, replicas.dbs[(size_t)std::max(0, sylph_pipeline_replica_of_last(p))], unknown);
    }
    // the ordered hand-over of `pool`'s jobs through this pipeline (ordered_ahead.hpp: order, failure rule, clean-up)
    template <class P, class Submit, class Consume>
    void run(ordered_ahead::Pool<P>& pool, Submit&& submit, Consume&& consume) {
        ordered_ahead::run(pool, cfg.depth, [&] { return outstanding(); }, submit, consume, [&] { drain(); });
    }
};

// ---- raw read samples (contain.rs:239-291 sketches and profiles them chunk by chunk on the rayon pool).  Here: up to `-t`
// sample threads, each with a GPU context of its own, read + index + pack + push their files into sessions, in input order;
// the sessions go through a sylph_pipeline (finish on the device -> probe, tables never leave HBM), and this thread takes the
// results in input order and does the statistics and the printing: the feed of sample j + 1 .. overlaps with the profile of
// sample j and the statistics of sample j - 1.
// interleaved[j]: read_files[j] is ONE file that holds the pairs itself (--interleaved)
void profile_raw_samples(Engine& e, const ContainCmdArgs& args, const std::vector<std::vector<std::string>>& read_files, const std::vector<uint8_t>& interleaved,
                         sylph_db* db, const ReportTo& to) {
    using ordered_ahead::Turn;
    const size_t n_raw = read_files.size();
    const uint64_t genome_c = to.genome_sketches[0].c, genome_k = to.genome_sketches[0].k;
    struct Prepared { std::optional<SequencesSketch> meta; sylph_sketch* session = nullptr; };   // no meta: refused or skipped
    ReplicaSet replicas(e, args, db, n_raw);                         // sample threads are dealt to the replicas' devices in turn
    const size_t n_workers = sample_workers(args.threads, (size_t)replicas.n_gpus, n_raw);
    std::vector<SampleFiles> job_files;
    for (size_t j = 0; j < n_raw; j++) {
        const auto& r = read_files[j];
        job_files.push_back({r[0], r.size() > 1 ? std::optional<std::string>(r[1]) : std::nullopt, interleaved[j] != 0, !args.no_mate_check});
    }
    FeedShared feed(std::move(job_files), n_workers);
    // contain.rs:591: raw pairs are sketched with the default filter (DEFAULT_FPR) — unless the exact set is asked for (not in the reference)
    const double raw_pair_fpr = exact_dedup_accepted(args.exact_dedup) ? 0. : DEFAULT_FPR;
    auto prepare = [&](Engine& eng, size_t j) {
        Prepared pr;
        const auto& files = read_files[j];
        if (genome_c < args.c) {
            fprintf(stderr, "ERROR [sylph_hip] %s error: value of -c for contain = %llu -- greater than the smallest value of -c for a genome sketch = %llu. Continuing without sketching.\n", files[0].c_str(), (unsigned long long)args.c, (unsigned long long)genome_c);
        } else if (genome_k != args.k) {
            fprintf(stderr, "ERROR [sylph_hip] %s -k %llu is not equal to -k %llu found in sketches. Continuing without sketching.\n", files[0].c_str(), (unsigned long long)args.k, (unsigned long long)genome_k);
        } else {
            try {
                SampleRoute route(eng, feed, j, false);
                SampleParams p;   // contain.rs:591: no sample name, duplicates always removed
                p.c = args.c; p.k = args.k; p.dedup_fpr = raw_pair_fpr;
                pr.meta = sketch_sample(eng, feed.ahead.files(j), p, route, &pr.session);
            } catch (...) { sylph_sketch_destroy(pr.session); throw; }
        }
        return pr;
    };
    // every sample thread brings its own context, made and destroyed on that thread: the database's context (the caller's engine)
    // stays free for the profile stage and the reassignment probes
    std::atomic<size_t> worker_no{0};
    auto sample_thread = [&]() -> ordered_ahead::Pool<Prepared>::Prepare {
        std::shared_ptr<Engine> own;
        try { own.reset(new Engine(replicas.device[worker_no++ % replicas.device.size()])); }
        catch (...) { throw Error{1, "could not create a GPU context for a sample thread"}; }
        return [own, &prepare](size_t j) { return prepare(*own, j); };
    };
    SamplePipe pipe(replicas, args, genome_k, ordered_ahead::ahead_limit(n_workers));
    std::vector<std::optional<SequencesSketch>> metas(n_raw);      // of the samples handed over, until their rows are out
    ordered_ahead::Pool<Prepared> pool(n_raw, n_workers, sample_thread, [](Prepared& pr) { sylph_sketch_destroy(pr.session); });
    pipe.run(pool,
             [&](size_t j, Prepared&& pr) {
                 if (!pr.meta || !pr.session) { sylph_sketch_destroy(pr.session); return Turn::Skip; }
                 hip_check(sylph_pipeline_submit_session(pipe.p, pr.session, j), "sylph_pipeline_submit_session");
                 metas[j] = std::move(pr.meta);
                 return Turn::Pipeline;
             },
             [&](size_t j, Turn turn) {
                 if (turn == Turn::Pipeline) pipe.report_last(to, pipe.next(read_files[j][0]), *metas[j], read_files[j][0]);
                 if (interleaved[j]) info("Finished paired sample " + read_files[j][0] + " (interleaved).");
                 else finished(read_files[j]);
                 metas[j].reset();
             });
}

// ---- samples given as sketches (*.sylsp; get_seq_sketch, contain.rs:544-599) ----
// The road sketch files take when SYLPH_HIP_SYLSP_DEVICE is not set.  The project's ship rule (as for FASTA reads): the device's
// road is the default only where whole `profile` commands over 64 sketches beat the host's road by more than both spreads, on
// ascending and on shuffled files alike — profiles/sylsp_pipeline.txt holds the record: 2.3x and 6.3x, so it is on.
constexpr bool SYLSP_DEVICE_DEFAULT = true;
// contain.rs:551-570's refusal of a sketch whose c the database cannot serve (the reference says "Exiting." and goes on, so do we)
void sketch_c_too_large(const std::string& file, uint64_t c, uint64_t genome_c) {
    fprintf(stderr, "ERROR [sylph_hip] %s value of -c is %llu; this is greater than the smallest value of -c = %llu for a genome sketch. Exiting.\n",
            file.c_str(), (unsigned long long)c, (unsigned long long)genome_c);
}
// SYLPH_HIP_FEED_TRACE: one line per sketch file — the road its table took, and whether the file's entries came strictly ascending
void trace_sketch_route(const std::string& file, const char* route, int ascending, uint64_t n_entries, uint64_t n_table) {
    if (!FeedLaps::on()) return;
    fprintf(stderr, "[sylph_hip feed] sylsp %s: route %s, table %s, %llu entries -> %llu k-mers\n", file.c_str(), route,
            ascending < 0 ? "sorted on the host" : ascending ? "ascending" : "sorted on the device", (unsigned long long)n_entries, (unsigned long long)n_table);
}
// The host's road: the table copied out of the file, sorted and deduplicated on one thread (read_sylsp), uploaded for the probe
// and, in `profile`, once more for the reassignment pass.  What every sketch file took before the device unpacked tables; still
// the road of SYLPH_HIP_SYLSP_DEVICE=0 and of a file with 2^31 entries or more.
void profile_sketch_on_host(const ContainCmdArgs& args, const std::string& file, sylph_db* db, const ReportTo& to) {
    const uint64_t genome_c = to.genome_sketches[0].c;
    const SequencesSketch S = read_sylsp(file);
    if (S.c > genome_c) { sketch_c_too_large(file, S.c, genome_c); return; }
    trace_sketch_route(file, "host", -1, S.kmers.size(), S.kmers.size());
    // first pass: GPU probe of every genome, then host statistics
    const uint32_t* cc = nullptr; const uint64_t* coff = nullptr; const uint32_t* covs = nullptr; uint64_t ncov = 0;
    hip_check(sylph_db_contain_view(db, S.kmers.data(), S.counts.data(), S.kmers.size(), SYLPH_MEM_HOST,
                                    args.min_number_kmers, &cc, &coff, &covs, &ncov), "sylph_db_contain_view");
    report(to, S, file, FirstPass{cc, coff, covs, 4, nullptr}, SampleTable{S.kmers.data(), S.counts.data(), S.kmers.size(), SYLPH_MEM_HOST}, db);
}
// SYLPH_HIP_SYLSP_DEVICE: 1 = the tables of sketch files are unpacked on the device and go through the pipeline, 0 = the host's
// road; unset = the default, which profiles/sylsp_pipeline.txt's measurement decides
bool sylsp_device_enabled() {
    static const bool on = [] { const char* v = getenv("SYLPH_HIP_SYLSP_DEVICE"); return v ? strcmp(v, "0") != 0 : SYLSP_DEVICE_DEFAULT; }();
    return on;
}

// The device's road: up to `-t` threads map and validate the files ahead, in input order, and touch the tables' pages
// (read_sylsp_header: the table stays in the mapping); this thread hands the entries to the pipeline as they lie in the file
// (sylph_pipeline_submit_entries: a worker unpacks them on the device, ascending files are never sorted), takes the results in
// input order and reports from the table in HBM, as for raw samples: file j + 1 is read while file j is probed and the
// statistics of file j - 1 run; the probe is batched; --gpus N deals the samples to N replicas.  Order and messages are the
// host road's: a file is refused, skipped or reported when its turn has come, after the rows of every file before it.
void profile_sketch_files(Engine& e, const ContainCmdArgs& args, const std::vector<std::string>& read_sketch_files, sylph_db* db, const ReportTo& to) {
    using ordered_ahead::Turn;
    const size_t n_files = read_sketch_files.size();
    if (n_files == 0) return;
    if (!sylsp_device_enabled()) {
        for (const auto& sf : read_sketch_files) { profile_sketch_on_host(args, sf, db, to); finished({sf}); }
        return;
    }
    const uint64_t genome_c = to.genome_sketches[0].c;
    using Prepared = std::optional<SylspView>;
    ReplicaSet replicas(e, args, db, n_files);
    const size_t n_workers = sample_workers(args.threads, 1, n_files);
    auto prepare = [&](size_t j) -> Prepared {
        SylspView v = read_sylsp_header(read_sketch_files[j]);
        if (v.meta.c <= genome_c && v.n_entries < (1ull << 31)) {   // (else nothing of the table is read on this road)
            const volatile uint8_t* page = v.entries;            // one byte of every page: the faults are taken here, not under the staging copy
            for (uint64_t at = 0, bytes = v.n_entries * 12; at < bytes; at += 4096) (void)page[at];
        }
        return v;
    };
    SamplePipe pipe(replicas, args, to.genome_sketches[0].k, ordered_ahead::ahead_limit(n_workers));
    std::vector<Prepared> views(n_files);                           // a file's mapping stays until its turn is over
    ordered_ahead::Pool<Prepared> pool(n_files, n_workers, [&]() -> ordered_ahead::Pool<Prepared>::Prepare { return prepare; }, [](Prepared&) {});
    pipe.run(pool,
             [&](size_t j, Prepared&& view) {
                 views[j] = std::move(view);
                 if (views[j]->meta.c > genome_c) return Turn::Skip;
                 // the host's road probes the database from this thread: it runs with the pipeline idle
                 if (views[j]->n_entries >= (1ull << 31)) return Turn::Inline;
                 hip_check(sylph_pipeline_submit_entries(pipe.p, views[j]->entries, views[j]->n_entries, SYLPH_MEM_HOST, j), "sylph_pipeline_submit_entries");
                 return Turn::Pipeline;
             },
             [&](size_t j, Turn turn) {
                 const std::string& file = read_sketch_files[j];
                 if (turn == Turn::Skip) sketch_c_too_large(file, views[j]->meta.c, genome_c);
                 else if (turn == Turn::Inline) {
                     if (stats_route() == StatsRoute::DeviceOnly) throw Error{1, "SYLPH_HIP_STATS_DEVICE=only: " + file + " takes the host's road"};
                     profile_sketch_on_host(args, file, db, to);
                 } else {
                     const sylph_pipeline_result r = pipe.next(file);
                     trace_sketch_route(file, "device", sylph_pipeline_ascending_of_last(pipe.p), views[j]->n_entries, r.n_table);
                     pipe.report_last(to, r, views[j]->meta, file);
                 }
                 finished({file});
                 views[j].reset();
             });
}
}  // namespace

// contain.rs:115-351
int contain(Engine& e, ContainCmdArgs args, bool pseudotax_in, FILE* out) {
    if (pseudotax_in) args.pseudotax = true;
    (void)stats_route();                                             // (a bad SYLPH_HIP_STATS_DEVICE fails the command before any work)
    (void)unknown_route();                                           // (and a bad SYLPH_HIP_UNKNOWN_DEVICE)
    std::vector<std::string> genome_sketch_files, genome_files, read_sketch_files;
    std::vector<std::vector<std::string>> read_files;
    std::vector<std::string> all_files = args.files;
    if (args.file_list) parse_line_file(*args.file_list, all_files);
    auto ends = [](const std::string& s, const char* suf) { const size_t n = strlen(suf); return s.size() >= n && s.compare(s.size() - n, n, suf) == 0; };
    for (const auto& f : all_files) {                                        // contain.rs:165-198
        if (ends(f, ".syldb") || ends(f, ".sylqueries")) genome_sketch_files.push_back(f);
        else if (ends(f, ".sylsp") || ends(f, ".sylsample")) read_sketch_files.push_back(f);
        else if (is_fasta(f)) genome_files.push_back(f);
        else if (is_fastq(f)) read_files.push_back({f});
        else warn(f + " file extension is not a sketch or a fasta/fastq file.");
    }
    if (args.first_pair.size() != args.second_pair.size())
        throw Error{1, "Different number of paired sequences (-1, -2) for sketching. Exiting."};
    for (size_t i = 0; i < args.first_pair.size(); i++) read_files.push_back({args.first_pair[i], args.second_pair[i]});
    std::vector<uint8_t> interleaved(read_files.size(), 0);                  // two-file pairs, then interleaved files, then single-end reads
    for (const auto& f : args.interleaved) { read_files.push_back({f}); interleaved.push_back(1); }
    for (const auto& r : args.reads) read_files.push_back({r});
    interleaved.resize(read_files.size(), 0);
    if (genome_sketch_files.empty() && genome_files.empty())
        throw Error{1, "No genome files found; see sylph query/profile -h for help. Exiting"};
    if (read_sketch_files.empty() && read_files.empty())
        throw Error{1, "No read files found; see sylph query/profile -h for help. Exiting"};

    const std::vector<GenomeSketch> genome_sketches = load_genome_sketches(e, args, genome_sketch_files, genome_files);
    DbGuard db;
    upload_database(e, genome_sketches, args.pseudotax, db);

    print_header(args.pseudotax, out, args.estimate_unknown);
    const ReportTo to{args, genome_sketches, out, e.context()};
    if (!read_files.empty()) profile_raw_samples(e, args, read_files, interleaved, db.d, to);
    profile_sketch_files(e, args, read_sketch_files, db.d, to);
    fflush(out);
    join_background();
    info("sylph finished.");
    return 0;
}

}  // namespace sylph_host
