// cmd_sketch.cpp — the `sketch` command (sketch.rs:276-479) and the genome batches behind it: genome files indexed and joined on the
// device (or, where the device declines, parsed on the host), batches pushed through the C ABI, the reference's .sylsp / .syldb files
// written.
#include <cstring>

#include "host_internal.hpp"
#include "../csrc/genome_acc_plan.h"

namespace sylph_host {

namespace acc_plan = sylph::genome_acc_plan;

uint64_t genome_push_limit() {
    static const uint64_t limit = [] {
        const char* e = getenv("SYLPH_HIP_GENOME_PUSH_BASES");
        const long long v = e ? atoll(e) : 0;
        return v > 0 && (uint64_t)v < acc_plan::PUSH_LIMIT ? (uint64_t)v : acc_plan::PUSH_LIMIT;
    }();
    return limit;
}

GenomeBatch::Parsed GenomeBatch::parse_file(const std::string& ref_file, bool /*individual: every record's id is kept either way*/) {
    Parsed p;
    p.file = ref_file;
    std::unique_ptr<FastxReader> reader;
    try { reader.reset(new FastxReader(ref_file)); }
    catch (const Error&) { p.warnings.push_back(ref_file + " is not a valid fasta/fastq file; skipping."); return p; }
    FastxRecord rec;
    try {
        while (reader->next(rec)) {
            p.ids.push_back(rec.id);
            p.bases.insert(p.bases.end(), rec.seq.begin(), rec.seq.end());
            p.ends.push_back(p.bases.size());
        }
    } catch (const Error&) {                                             // :586-589: the whole file is dropped
        p.warnings.push_back("File " + ref_file + " is not a valid fasta/fastq file");
        return p;
    }
    p.ok = true;
    return p;
}

bool fasta_device_enabled() {
    static const bool on = [] {
        if (!device_feed_enabled()) return false;
        // opt-in: with the files read, decoded and indexed window by window on the engine's thread the command is not yet faster than the
        // host road's `-t` threads (profiles/fasta_device_db_build.txt)
        if (const char* e = getenv("SYLPH_HIP_FASTA_DEVICE")) return atoi(e) != 0;
        return false;
    }();
    return on;
}

namespace {

// the bytes of a regular file as they lie on disk (never a pipe: its bytes would be gone for the host reader); false: not for this road
bool read_raw(const std::string& path, std::vector<uint8_t>& out) {
    struct stat st;
    if (stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode) || st.st_size <= 0) return false;
    FILE* fp = fopen(path.c_str(), "rb");
    if (!fp) return false;
    out.resize((size_t)st.st_size);
    const size_t got = fread(out.data(), 1, out.size(), fp);
    fclose(fp);
    return got == out.size();
}
Container container_of_bytes(const std::vector<uint8_t>& b) {
    if (b.size() >= 2 && b[0] == 0x1f && b[1] == 0x8b) return Container::Gzip;
    if (b.size() >= 2 && b[0] == 'B' && b[1] == 'Z') return Container::Bzip2;
    return Container::Plain;
}
bool declined(int rc) { return rc == SYLPH_ERR_FORMAT || rc == SYLPH_ERR_NOMEM; }

// f(i) for i in [0, n) on up to `threads` threads
template <class F>
void on_threads(size_t n, uint64_t threads, F&& f) {
    std::atomic<size_t> next{0};
    auto work = [&] { for (size_t i = next++; i < n; i = next++) f(i); };
    std::vector<std::thread> pool;
    for (size_t w = 1; w < std::min<size_t>(std::max<uint64_t>(threads, 1), n); w++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
}

}  // namespace

void GenomeBatch::add_window_device(const std::vector<std::string>& files, size_t lo, size_t n, bool individual, uint64_t threads) {
    FeedLaps laps;
    sylph_ctx* ctx = e.context();
    // the threads only read bytes
    std::vector<std::vector<uint8_t>> raw(n);
    std::vector<char> readable(n, 0);
    on_threads(n, threads, [&](size_t i) { readable[i] = read_raw(files[lo + i], raw[i]) ? 1 : 0; });
    // this thread decodes and indexes.  Compressed files of one container that follow each other are decoded by ONE call (bounded well
    // below the decoders' 3 GiB of compressed bytes, so that text and batch stay within about 2 x BATCH_BASES); a call that is declined
    // is retried file by file, and a file declined alone is the host reader's.
    constexpr uint64_t DECODE_CALL_BYTES = 256ull << 20;
    std::vector<DeviceGenomeFile> dv(n);
    std::vector<char> ok(n, 0);
    auto index = [&](size_t i, const void* text, uint64_t bytes, int mem) {
        sylph_fasta* f = nullptr;
        const int rc = sylph_fasta_index(ctx, text, bytes, mem, &f);
        if (declined(rc)) return;
        hip_check(rc, "sylph_fasta_index");
        dv[i].fa.reset(f);
        dv[i].file = files[lo + i];
        dv[i].text_bytes = bytes;
        hip_check(sylph_fasta_counts(f, &dv[i].n_records, &dv[i].n_bases, &dv[i].id_bytes), "sylph_fasta_counts");
        // More than one batch: the host reader cuts it (append).  Such a file has been read, perhaps decoded, and indexed here for nothing
        // and is read again there: the number of bases is not known before the index (the text's size bounds it only from above), and at
        // the default limit the index declines a text that large by itself.  With SYLPH_HIP_GENOME_PUSH_BASES lowered, a node that expects
        // mostly such files does better with the host road (SYLPH_HIP_FASTA_DEVICE unset).
        if (dv[i].n_bases >= genome_push_limit()) { dv[i] = DeviceGenomeFile(); return; }
        ok[i] = 1;
    };
    auto decode = [&](Container c, size_t first, size_t count) {          // true: files [first, first + count) decoded and indexed
        std::vector<const void*> ptrs;
        std::vector<uint64_t> lens;
        for (size_t i = first; i < first + count; i++) { ptrs.push_back(raw[i].data()); lens.push_back(raw[i].size()); }
        sylph_inflated* h = nullptr;
        const int rc = c == Container::Gzip ? sylph_inflate_files(ctx, ptrs.data(), lens.data(), (uint32_t)count, SYLPH_MEM_HOST, &h)
                                            : sylph_bunzip2_files(ctx, ptrs.data(), lens.data(), (uint32_t)count, SYLPH_MEM_HOST, &h);
        if (declined(rc)) return false;
        hip_check(rc, c == Container::Gzip ? "sylph_inflate_files" : "sylph_bunzip2_files");
        std::shared_ptr<sylph_inflated> text(h, sylph_inflated_destroy);
        for (size_t i = first; i < first + count; i++) {
            const void* dev = nullptr;
            uint64_t bytes = 0;
            hip_check(sylph_inflated_file(h, (uint32_t)(i - first), &dev, &bytes), "sylph_inflated_file");
            dv[i].text = text;
            if (bytes) index(i, dev, bytes, SYLPH_MEM_DEVICE);
            if (!ok[i]) dv[i].text.reset();
        }
        return true;
    };
    for (size_t i = 0; i < n;) {
        if (!readable[i]) { i++; continue; }
        const Container c = container_of_bytes(raw[i]);
        if (c == Container::Plain) { index(i, raw[i].data(), raw[i].size(), SYLPH_MEM_HOST); i++; continue; }
        if (!device_decode_enabled(c)) { i++; continue; }
        size_t count = 0;
        uint64_t bytes = 0;
        while (i + count < n && readable[i + count] && container_of_bytes(raw[i + count]) == c && (count == 0 || bytes + raw[i + count].size() <= DECODE_CALL_BYTES)) {
            bytes += raw[i + count].size();
            count++;
        }
        if (!decode(c, i, count) && count > 1)
            for (size_t j = i; j < i + count; j++) (void)decode(c, j, 1);
        i += count;
    }
    raw.clear();
    // what the device declined is read on the host, on the threads
    std::vector<size_t> host_files;
    for (size_t i = 0; i < n; i++) if (!ok[i]) host_files.push_back(i);
    std::vector<Parsed> parsed(n);
    on_threads(host_files.size(), threads, [&](size_t j) { parsed[host_files[j]] = parse_file(files[lo + host_files[j]], individual); });
    // in file order; the batch of the other road is flushed first
    const uint64_t LIMIT = genome_push_limit();
    for (size_t i = 0; i < n; i++) {
        if (!ok[i]) { flush_device(); append(std::move(parsed[i]), individual); continue; }
        flush();
        if (!dev_group.empty() && (dev_bases + dv[i].n_bases >= LIMIT || dev_text_bytes + dv[i].text_bytes >= BATCH_BASES)) flush_device();
        dev_individual = individual;
        dev_bases += dv[i].n_bases;
        dev_text_bytes += dv[i].text_bytes;
        dev_group.push_back(std::move(dv[i]));
    }
    flush_device();
    if (FeedLaps::on()) {
        char what[96];
        snprintf(what, sizeof(what), "genomes fasta-device files=%zu declined=%zu", n, host_files.size());
        laps.lap(what);
    }
}

void GenomeBatch::flush_device() {
    if (dev_group.empty()) return;
    std::vector<DeviceGenomeFile> group;
    group.swap(dev_group);
    dev_text_bytes = dev_bases = 0;
    const bool individual = dev_individual;
    uint64_t G = 0;
    std::vector<sylph_fasta*> hs;
    for (const auto& f : group) { hs.push_back(f.fa.get()); G += individual ? f.n_records : 1; }
    std::vector<uint64_t> koff(G + 1), toff(G + 1);
    uint64_t *gk = nullptr, *tr = nullptr;
    const int rc = sylph_sketch_genomes_fasta(e.context(), hs.data(), (uint32_t)hs.size(), individual ? 1 : 0, (uint32_t)c, (uint32_t)k,
                                              SYLPH_SEED_AVX2_COMPAT, min_spacing, pseudotax ? 1 : 0, &gk, koff.data(), &tr, toff.data());
    if (rc == SYLPH_ERR_NOMEM) {                                          // no room for text and batch side by side: the host road for these files
        std::vector<std::string> names;
        for (const auto& f : group) names.push_back(f.file);
        group.clear();
        for (const auto& f : names) append(parse_file(f, individual), individual);
        flush();
        return;
    }
    hip_check(rc, "sylph_sketch_genomes_fasta");
    struct Free { uint64_t* p; ~Free() { sylph_free(p); } } f1{gk}, f2{tr};
    uint64_t g = 0;
    for (const auto& f : group) {
        // names and sizes back from the index: the first record's id only unless `individual`
        const uint64_t n_ids = individual ? f.n_records : std::min<uint64_t>(1, f.n_records);
        std::vector<uint64_t> id_off(n_ids + 1, 0), len(f.n_records);
        std::vector<char> ids(f.id_bytes + 1);
        hip_check(sylph_fasta_ids(f.fa.get(), 0, n_ids, ids.data(), f.id_bytes, id_off.data()), "sylph_fasta_ids");
        hip_check(sylph_fasta_lengths(f.fa.get(), 0, f.n_records, len.data()), "sylph_fasta_lengths");
        const uint64_t n_genomes = individual ? f.n_records : 1;
        for (uint64_t r = 0; r < n_genomes; r++, g++) {
            GenomeSketch s;
            s.file_name = f.file;
            if (r < n_ids) s.first_contig_name.assign(ids.data() + id_off[r], ids.data() + id_off[r + 1]);
            s.gn_size = individual ? len[r] : f.n_bases;
            s.genome_kmers.assign(gk + koff[g], gk + koff[g + 1]);
            if (pseudotax) s.pseudotax_tracked_nonused_kmers = std::vector<uint64_t>(tr + toff[g], tr + toff[g + 1]);
            s.c = c; s.k = k; s.min_spacing = min_spacing;
            out.push_back(std::move(s));
        }
    }
}

void GenomeBatch::add_files(const std::vector<std::string>& files, bool individual, uint64_t threads) {
    const size_t window = std::max<size_t>(1, std::min<size_t>(threads, 64)) * 2;
    const bool device_road = fasta_device_enabled();
    for (size_t lo = 0; lo < files.size(); lo += window) {
        const size_t n = std::min(window, files.size() - lo);
        if (device_road) { add_window_device(files, lo, n, individual, threads); continue; }
        std::vector<Parsed> parsed(n);
        std::atomic<size_t> next{0};
        auto work = [&] { for (size_t i = next++; i < n; i = next++) parsed[i] = parse_file(files[lo + i], individual); };
        std::vector<std::thread> pool;
        for (size_t w = 1; w < std::min<size_t>(std::max<uint64_t>(threads, 1), n); w++) pool.emplace_back(work);
        work();
        for (auto& t : pool) t.join();
        for (auto& p : parsed) append(std::move(p), individual);
    }
}

bool GenomeBatch::append(Parsed p, bool individual) {
    for (const auto& w : p.warnings) warn(w);
    if (!p.ok) return false;
    const std::string& ref_file = p.file;
    // one sylph_sketch_genomes call holds fewer than L bases: a file that would push the batch over the limit starts a new batch,
    // and a file that holds L bases or more by itself is cut at its record boundaries
    const uint64_t LIMIT = genome_push_limit();
    if (p.bases.size() >= LIMIT) {
        flush();
        return individual ? append_split(p) : append_accumulated(p);
    }
    if (bases.size() + p.bases.size() >= LIMIT) flush();
    const uint64_t bases0 = bases.size();
    bases.insert(bases.end(), p.bases.begin(), p.bases.end());
    for (size_t r = 0; r < p.ends.size(); r++) {
        off.push_back(bases0 + p.ends[r]);
        if (individual) {
            GenomeSketch g;
            g.file_name = ref_file; g.first_contig_name = p.ids[r]; g.gn_size = p.ends[r] - (r ? p.ends[r - 1] : 0);
            pending.push_back(std::move(g));
            goff.push_back(off.size() - 1);
        }
    }
    if (!individual) {
        GenomeSketch whole;
        whole.file_name = ref_file;
        if (!p.ids.empty()) whole.first_contig_name = p.ids.front();
        whole.gn_size = p.bases.size();
        pending.push_back(std::move(whole));
        goff.push_back(off.size() - 1);
    }
    if (bases.size() >= BATCH_BASES) flush();
    return true;
}

namespace {
std::vector<uint64_t> record_lengths(const std::vector<uint64_t>& ends) {
    std::vector<uint64_t> lens(ends.size());
    for (size_t r = 0; r < ends.size(); r++) lens[r] = ends[r] - (r ? ends[r - 1] : 0);
    return lens;
}
std::string over_limit(uint64_t n_bases) {
    return " holds " + std::to_string(n_bases) + " bases, more than one device batch (" + std::to_string(genome_push_limit()) + ")";
}
}  // namespace

// one genome per record: every run of the plan's cut is a batch of its own, in file order
bool GenomeBatch::append_split(const Parsed& p) {
    FeedLaps laps;
    const uint64_t LIMIT = genome_push_limit();
    const std::vector<uint64_t> lens = record_lengths(p.ends);
    const uint64_t n = lens.size();
    uint64_t batches = 0, skipped = 0;
    auto batch = [&](const acc_plan::Run& run) {
        const uint64_t base0 = run.first ? p.ends[run.first - 1] : 0;
        std::vector<uint64_t> off_(run.n + 1, 0), goff_(run.n + 1, 0);
        std::vector<GenomeSketch> names(run.n);
        for (uint64_t i = 0; i < run.n; i++) {
            off_[i + 1] = p.ends[run.first + i] - base0;
            goff_[i + 1] = i + 1;
            names[i].file_name = p.file; names[i].first_contig_name = p.ids[run.first + i]; names[i].gn_size = lens[run.first + i];
        }
        sketch_batch(p.bases.data() + base0, off_, goff_, names);
        batches++;
    };
    for (uint64_t at = 0; at < n;) {
        at = acc_plan::cut(lens.data(), n, at, LIMIT, batch);
        if (at < n) {                                                     // a record no batch holds: the others are still sketched
            warn(p.file + ": record " + p.ids[at] + over_limit(lens[at]) + ": skipping it");
            skipped++;
            at++;
        }
    }
    if (FeedLaps::on()) {
        const std::string what = "genomes split: " + p.file + " records=" + std::to_string(n) + " batches=" + std::to_string(batches) +
                                 " skipped=" + std::to_string(skipped);
        laps.lap(what.c_str());
    }
    return batches > 0;
}

// one genome per file: the runs of the plan's cut are pushed through an accumulator, whose finish removes the duplicates of the whole
// file (sketch.rs:590-600) and runs the spacing filter, which restarts at every contig (:606)
bool GenomeBatch::append_accumulated(const Parsed& p) {
    FeedLaps laps;
    const uint64_t LIMIT = genome_push_limit();
    const std::vector<uint64_t> lens = record_lengths(p.ends);
    const uint64_t n = lens.size();
    std::vector<acc_plan::Run> runs;
    const uint64_t misfit = acc_plan::cut(lens.data(), n, 0, LIMIT, [&](const acc_plan::Run& run) { runs.push_back(run); });
    if (misfit < n) {   // positions inside a contig are 32-bit in the seeding kernels: the one difference from the reference left
        warn(p.file + ": contig " + p.ids[misfit] + over_limit(lens[misfit]) + ": skipping the file");
        return false;
    }
    sylph_genome_acc* h = nullptr;
    hip_check(sylph_genome_acc_create(e.context(), (uint32_t)c, (uint32_t)k, SYLPH_SEED_AVX2_COMPAT, min_spacing, pseudotax ? 1 : 0, &h),
              "sylph_genome_acc_create");
    std::unique_ptr<sylph_genome_acc, void (*)(sylph_genome_acc*)> acc(h, sylph_genome_acc_destroy);
    uint64_t pushes = 0;
    int rc = SYLPH_OK;
    const char* what = "sylph_genome_acc_push";
    for (const acc_plan::Run& run : runs) {
        if (rc != SYLPH_OK) break;
        const uint64_t base0 = run.first ? p.ends[run.first - 1] : 0;
        std::vector<uint64_t> off_(run.n + 1, 0);
        for (uint64_t i = 0; i < run.n; i++) off_[i + 1] = p.ends[run.first + i] - base0;
        rc = sylph_genome_acc_push(acc.get(), p.bases.data() + base0, off_.data(), run.n, SYLPH_MEM_HOST);
        pushes++;
    }
    uint64_t *gk = nullptr, *tr = nullptr, nk = 0, nt = 0, n_seeds = 0;
    if (rc == SYLPH_OK) {
        hip_check(sylph_genome_acc_counts(acc.get(), nullptr, nullptr, &n_seeds), "sylph_genome_acc_counts");
        what = "sylph_genome_acc_finish";
        rc = sylph_genome_acc_finish(acc.get(), &gk, &nk, &tr, &nt);
    }
    if (rc == SYLPH_ERR_NOMEM) {
        warn(p.file + ": no room on the device for the seeds of " + std::to_string(p.bases.size()) + " bases (" + what + "): skipping the file");
        return false;
    }
    hip_check(rc, what);
    struct Free { uint64_t* p; ~Free() { sylph_free(p); } } f1{gk}, f2{tr};
    GenomeSketch s;
    s.file_name = p.file;
    if (!p.ids.empty()) s.first_contig_name = p.ids.front();
    s.gn_size = p.bases.size();
    s.genome_kmers.assign(gk, gk + nk);
    if (pseudotax) s.pseudotax_tracked_nonused_kmers = std::vector<uint64_t>(tr, tr + nt);
    s.c = c; s.k = k; s.min_spacing = min_spacing;
    out.push_back(std::move(s));
    if (FeedLaps::on()) {
        const std::string line = "genomes accumulate: " + p.file + " contigs=" + std::to_string(n) + " bases=" + std::to_string(p.bases.size()) +
                                 " pushes=" + std::to_string(pushes) + " seeds=" + std::to_string(n_seeds);
        laps.lap(line.c_str());
    }
    return true;
}

void GenomeBatch::sketch_batch(const uint8_t* bases_, const std::vector<uint64_t>& off_, const std::vector<uint64_t>& goff_,
                               std::vector<GenomeSketch>& names) {
    const uint64_t G = names.size();
    std::vector<uint64_t> koff(G + 1), toff(G + 1);
    uint64_t *gk = nullptr, *tr = nullptr;
    hip_check(sylph_sketch_genomes(e.context(), bases_, off_.data(), off_.size() - 1, goff_.data(), G, (uint32_t)c, (uint32_t)k,
                                   SYLPH_SEED_AVX2_COMPAT, min_spacing, pseudotax ? 1 : 0, SYLPH_MEM_HOST, &gk, koff.data(), &tr,
                                   toff.data()),
              "sylph_sketch_genomes");
    struct Free { uint64_t* p; ~Free() { sylph_free(p); } } f1{gk}, f2{tr};
    for (uint64_t g = 0; g < G; g++) {
        GenomeSketch& s = names[g];
        s.genome_kmers.assign(gk + koff[g], gk + koff[g + 1]);
        if (pseudotax) s.pseudotax_tracked_nonused_kmers = std::vector<uint64_t>(tr + toff[g], tr + toff[g + 1]);
        s.c = c; s.k = k; s.min_spacing = min_spacing;
        out.push_back(std::move(s));
    }
}

void GenomeBatch::flush() {
    if (pending.empty()) return;
    sketch_batch(bases.data(), off, goff, pending);
    pending.clear(); bases.clear(); off.assign(1, 0); goff.assign(1, 0);
}

// sketch.rs:550-622
std::optional<GenomeSketch> sketch_genome(Engine& e, uint64_t c, uint64_t k, const std::string& ref_file, uint64_t min_spacing,
                                          bool pseudotax) {
    std::vector<GenomeSketch> out;
    GenomeBatch b(e, c, k, min_spacing, pseudotax, out);
    if (!b.add_file(ref_file, false)) return std::nullopt;
    b.flush();
    return std::move(out.front());
}

// sketch.rs:481-548
std::vector<GenomeSketch> sketch_genome_individual(Engine& e, uint64_t c, uint64_t k, const std::string& ref_file,
                                                   uint64_t min_spacing, bool pseudotax) {
    std::vector<GenomeSketch> out;
    GenomeBatch b(e, c, k, min_spacing, pseudotax, out);
    b.add_file(ref_file, true);
    b.flush();
    return out;
}

// sketch.rs:276-479
int sketch(Engine& e, const SketchArgs& args) {
    std::vector<std::string> read_inputs, genome_inputs, first_pairs, second_pairs;
    const bool nothing = args.files.empty() && !args.list_sequence && args.first_pair.empty() && args.second_pair.empty() &&
                         args.genomes.empty() && args.reads.empty() && !args.list_genomes && !args.list_reads &&
                         !args.list_first_pair && !args.list_second_pair && args.interleaved.empty() && !args.list_interleaved;
    if (nothing) throw Error{1, "No input sequences found; see sylph sketch -h for help. Exiting."};   // :144-157
    if (args.fpr < 0. || args.fpr >= 1.) throw Error{1, "Invalid FPR for sketching. Must be in [0,1)."};   // :158-161
    std::vector<std::string> all_files;
    if (args.list_sequence) parse_line_file(*args.list_sequence, all_files);
    all_files.insert(all_files.end(), args.files.begin(), args.files.end());
    for (const auto& f : all_files) {                                        // :164-189
        if (is_fastq(f)) read_inputs.push_back(f);
        else if (is_fasta(f)) genome_inputs.push_back(f);
        else warn(f + " does not have a fasta/fastq/gzip type extension; skipping");
    }
    genome_inputs.insert(genome_inputs.end(), args.genomes.begin(), args.genomes.end());   // :191-216
    read_inputs.insert(read_inputs.end(), args.reads.begin(), args.reads.end());
    if (args.list_reads) parse_line_file(*args.list_reads, read_inputs);
    if (args.list_genomes) parse_line_file(*args.list_genomes, genome_inputs);
    if (args.first_pair.size() != args.second_pair.size()) throw Error{1, "Different number of paired sequences. Exiting."};
    first_pairs = args.first_pair;
    second_pairs = args.second_pair;
    if (args.list_first_pair) parse_line_file(*args.list_first_pair, first_pairs);
    if (args.list_second_pair) parse_line_file(*args.list_second_pair, second_pairs);
    if (first_pairs.size() != second_pairs.size()) throw Error{1, "Different number of paired sequences. Exiting."};
    std::vector<std::string> interleaved = args.interleaved;                 // (not in the reference) pairs in ONE file each
    if (args.list_interleaved) parse_line_file(*args.list_interleaved, interleaved);
    std::optional<std::vector<std::string>> sample_names;                    // :260-274
    if (args.list_sample_names) { sample_names.emplace(); parse_line_file(*args.list_sample_names, *sample_names); }
    else if (args.sample_names) sample_names = args.sample_names;
    // jobs, and the names that go with them, in this order: two-file pairs, interleaved files, single-end reads
    if (sample_names && sample_names->size() != first_pairs.size() + interleaved.size() + read_inputs.size())
        throw Error{1, "Sample name length is not equal to the number of reads. Exiting"};   // :288-292
    // a10: pairs are deduplicated as the reference does — --fpr != 0 (default 1e-4, cmdline.rs:77): the set behind a cuckoo filter
    // (sketch.rs:733-769; the session option "dedup_fpr"); --fpr 0: the exact set (:690-731).  --exact-dedup / SYLPH_HIP_EXACT_DEDUP=1
    // (not in the reference) force the exact set whatever --fpr says.  (--no-dedup never consults the filter: sketch.rs:744.)
    const double pair_fpr = exact_dedup_accepted(args.exact_dedup) ? 0. : args.fpr;

    // Samples are independent (sketch.rs:313,371 runs them on the rayon pool, `-t`): a pool of `-t` worker threads, each with
    // its own GPU context (calls on one context are serialised) and its own page-locked batch, takes them in input order.
    // The parsing / inflating of different samples overlaps; the GPU work of one sample is ~2 ms per Gbp.
    create_dir_all(args.sample_output_dir);
    const size_t n_jobs = first_pairs.size() + interleaved.size() + read_inputs.size();
    // (a command's first sample is gathered into pageable memory while the GPU runtime comes up and the device route's uploader serves the
    //  samples BEHIND it: with one sample nobody ever wants the page-locked feed buffers — ~80 ms of hipHostMalloc beside the sample's own
    //  push, and as much again when the process is torn down)
    if (n_jobs <= 1) e.defer_pinned.store(true);
    // --gpus N|all (round 6): the workers are dealt to the node's GPUs — worker w runs on device w mod N, with its own context, page-locked
    // batch and uploader there; a sample never leaves its GPU, nothing is exchanged ("replicas only" for the sketch stage —
    // what the reference's rayon pool does with the machine's cores, sketch.rs:313, :371).  At least one worker per GPU.
    int n_gpus = 1;
    if (args.gpus != 1) {
        const int have = std::max(1, sylph_device_count());
        n_gpus = args.gpus < 0 ? have : std::min(args.gpus, have);
        if (args.gpus > have) warn("--gpus " + std::to_string(args.gpus) + ": this node has " + std::to_string(have) + " GPU(s); using them all");
    }
    // (tests on a one-GPU box: SYLPH_HIP_FAKE_GPUS=N deals the workers as for N GPUs and maps every one of them to device 0)
    const char* fake = getenv("SYLPH_HIP_FAKE_GPUS");
    const int n_deal = fake ? std::max(1, atoi(fake)) : n_gpus;
    const size_t n_workers = sample_workers(args.threads, args.gpus != 1 || fake ? (size_t)n_deal : 1, n_jobs);
    // the next sample of every worker is indexed while the current one is gathered and pushed
    std::vector<SampleFiles> job_files;
    for (size_t j = 0; j < first_pairs.size(); j++) job_files.push_back({first_pairs[j], second_pairs[j]});
    for (const auto& f : interleaved) job_files.push_back({f, std::nullopt, true, !args.no_mate_check});
    for (const auto& r : read_inputs) job_files.push_back({r, std::nullopt});
    FeedShared feed(std::move(job_files), n_workers);
    // a finished sketch is written by the writers' thread while its worker takes the next sample; the first error is rethrown by the command
    std::mutex write_mu;
    std::optional<Error> write_error;
    auto write_out = [&](const std::string& path, SequencesSketch&& sk, const std::string& what, std::function<void(const SequencesSketch&, const std::string&)> timing) {
        auto keep = std::make_shared<SequencesSketch>(std::move(sk));
        auto task = [&write_mu, &write_error, keep, path, what, timing] {
            try {
                write_sylsp(path, *keep);
                trace_mark("sketch: .sylsp written");
                info("Sketching " + path + " complete.");
                timing(*keep, what);
            } catch (const Error& er) {
                std::lock_guard<std::mutex> lk(write_mu);
                if (!write_error) write_error = er;
            }
        };
        if (n_jobs > 1) write_behind(task); else task();
    };
    struct DrainWriters { ~DrainWriters() { drain_writers(); } } drain_on_exit;     // (also on the way out of an exception: the tasks refer to this frame)
    auto run_job = [&](Engine& eng, size_t j) {
        const SampleFiles& files = feed.ahead.files(j);
        SampleRoute route(eng, feed, j, true);
        const auto t_job = std::chrono::steady_clock::now();
        auto timing = [t_job](const SequencesSketch& sk, const std::string& what) {   // (not a reference message: feed measurements)
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_job).count();
            uint64_t occ = 0;
            for (uint32_t c : sk.counts) occ += c;
            char b[256];
            snprintf(b, sizeof(b), "timing: %s sketched + written in %.3f s (%zu distinct k-mers, %llu counted occurrences)", what.c_str(), sec,
                     sk.kmers.size(), (unsigned long long)occ);
            info(b);
        };
        const bool paired = files.paired();                                  // pairs :311-367 (an interleaved file is one), single files :369-420
        SampleParams p;
        p.c = args.c; p.k = args.k; p.no_dedup = args.no_dedup; p.dedup_fpr = pair_fpr;
        if (sample_names) p.sample_name = (*sample_names)[j];
        auto sk = sketch_sample(eng, files, p, route, nullptr);
        if (!sk) return;
        const std::string& name = sk->sample_name ? *sk->sample_name : sk->file_name;
        const std::string path = path_join(args.sample_output_dir, basename_of(name)) + (paired ? ".paired" : "") + SAMPLE_FILE_SUFFIX;
        if (paired) trace_mark("sketch: the pair is sketched (table on the host)");
        write_out(path, std::move(*sk), files.first, timing);
    };
    if (n_workers <= 1) {
        for (size_t j = 0; j < n_jobs; j++) run_job(e, j);
    } else {
        std::atomic<size_t> next{0};
        std::mutex err_mu;
        std::optional<Error> first_error;
        std::atomic<size_t> worker_no{1};
        auto worker = [&](Engine* eng) {
            try {
                std::unique_ptr<Engine> own;
                if (!eng) {
                    const size_t w = worker_no++;
                    const int dev = n_deal > 1 ? (fake ? e.device : (int)(w % (size_t)n_deal)) : e.device;
                    if (n_deal > 1) info("sketch worker " + std::to_string(w) + " runs on GPU " + std::to_string(fake ? (int)(w % (size_t)n_deal) : dev) + (fake ? " (SYLPH_HIP_FAKE_GPUS: device 0)" : ""));
                    own.reset(new Engine(dev));
                    eng = own.get();
                }
                for (size_t j = next++; j < n_jobs; j = next++) run_job(*eng, j);
            } catch (const Error& er) {
                std::lock_guard<std::mutex> lk(err_mu);
                if (!first_error) first_error = er;
                next = n_jobs;   // stop handing out work
            }
        };
        std::vector<std::thread> pool;
        for (size_t w = 1; w < n_workers; w++) pool.emplace_back(worker, nullptr);
        worker(&e);
        for (auto& t : pool) t.join();
        if (first_error) throw *first_error;
    }
    drain_writers();
    if (write_error) throw *write_error;
    if (!genome_inputs.empty()) {                                            // :422-476
        const std::string path = args.db_out_name + QUERY_FILE_SUFFIX;
        create_dir_all(dirname_of(path));
        std::vector<GenomeSketch> all;
        GenomeBatch batch(e, args.c, args.k, args.min_spacing_kmer, !args.no_pseudotax, all);
        batch.add_files(genome_inputs, args.individual, args.threads);
        batch.flush();
        if (all.empty()) warn("No valid genomes to sketch; " + path + " is not output");
        else { write_syldb(path, all); info("Wrote all genome sketches to " + path); }
    }
    if (!fast_exit()) join_background();
    info("Finished.");
    return 0;
}

}  // namespace sylph_host
