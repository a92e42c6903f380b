// host_internal.hpp — what the host's own source files share (engine.cpp, sample_feed.cpp, cmd_sketch.cpp, cmd_contain.cpp): messages,
// path helpers, the session wrapper, the background threads and the types of a sample's way to the device.  Not part of the
// interface in sylph_host.hpp: neither installed nor exported.  (cmd_contain.cpp's hand-over of samples to the pipeline — the
// prepare-ahead pool and the ordered driver — is ordered_ahead.hpp, a header of its own that includes nothing of this one.)
#pragma once
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <future>

#include "sylph_host.hpp"

namespace sylph_host {

inline void hip_check(int rc, const char* what) {
    if (rc != SYLPH_OK) throw Error{1, std::string(what) + ": " + sylph_last_error()};
}
inline void warn(const std::string& m) { fprintf(stderr, "WARN  [sylph_hip] %s\n", m.c_str()); }
inline void info(const std::string& m) { fprintf(stderr, "INFO  [sylph_hip] %s\n", m.c_str()); }
// several info lines in ONE write: a block that samples reported from different threads must not interleave inside
inline void info_block(const std::vector<std::string>& lines) {
    std::string all;
    for (const auto& l : lines) all += "INFO  [sylph_hip] " + l + "\n";
    fwrite(all.data(), 1, all.size(), stderr);
}

template <class T>
std::vector<T> take(T* p, uint64_t n) {
    std::vector<T> v(p, p + n);
    sylph_free(p);
    return v;
}

inline std::string basename_of(const std::string& p) {
    const size_t s = p.find_last_of('/');
    return s == std::string::npos ? p : p.substr(s + 1);
}
inline std::string dirname_of(const std::string& p) {
    const size_t s = p.find_last_of('/');
    return s == std::string::npos ? std::string() : p.substr(0, s);
}
inline void create_dir_all(const std::string& dir) {
    if (dir.empty()) return;
    std::string cur;
    for (size_t i = 0; i <= dir.size(); i++) {
        if (i == dir.size() || dir[i] == '/') {
            if (!cur.empty() && cur != "." && cur != "..") mkdir(cur.c_str(), 0777);
        }
        if (i < dir.size()) cur += dir[i];
    }
}
inline std::string path_join(const std::string& a, const std::string& b) {
    if (a.empty()) return b;
    return a.back() == '/' ? a + b : a + "/" + b;
}
inline void parse_line_file(const std::string& file, std::vector<std::string>& out) {   // sketch.rs:252
    std::ifstream f(file);
    if (!f) throw Error{1, "could not open list file " + file};
    std::string line;
    while (std::getline(f, line)) out.push_back(line);
}

// f(i) for i in [0, n) on up to `threads` threads (f must not throw)
template <class F>
void parallel_for(size_t n, uint64_t threads, F&& f) {
    const size_t t = std::max<size_t>(1, std::min<size_t>(threads, (n + 15) / 16));
    if (t <= 1) { for (size_t i = 0; i < n; i++) f(i); return; }
    std::atomic<size_t> next{0};
    auto work = [&] { for (size_t i = next++; i < n; i = next++) f(i); };
    std::vector<std::thread> pool;
    for (size_t w = 1; w < t; w++) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
}
struct ThreadJoiner {   // joins on every way out of a scope (an Error thrown past a joinable std::thread is std::terminate)
    std::thread& t;
    ~ThreadJoiner() { if (t.joinable()) t.join(); }
};
// Sample threads of a command: `-t` of them, at most MAX_SAMPLE_THREADS, but at least one for every GPU the samples are dealt to;
// never more than there are samples, never none.
inline size_t sample_workers(uint64_t threads, size_t gpus_dealt, size_t n_samples) {
    const size_t wanted = std::max(std::min<size_t>(threads, MAX_SAMPLE_THREADS), gpus_dealt);
    return std::max<size_t>(1, std::min(wanted, n_samples));
}

struct Session {   // RAII
    sylph_sketch* sk = nullptr;
    // dedup_fpr != 0 (pairs): the reference's dup_removal_lsh_full over its cuckoo filter (sketch.rs:839-848); 0: the exact set (:829-838)
    Session(Engine& e, uint64_t c, uint64_t k, bool paired, bool no_dedup, double dedup_fpr = 0.) {
        hip_check(sylph_sketch_begin(e.context(), (uint32_t)c, (uint32_t)k, paired ? SYLPH_READS_PAIRED : SYLPH_READS_SINGLE,
                                     no_dedup ? 1 : 0, SYLPH_SEED_AVX2_COMPAT, &sk), "sylph_sketch_begin");
        if (paired && !no_dedup && dedup_fpr != 0.) {
            char v[64];
            snprintf(v, sizeof(v), "%.17g", dedup_fpr);
            const int rc = sylph_sketch_set_option(sk, "dedup_fpr", v);
            if (rc != SYLPH_OK) { sylph_sketch_destroy(sk); sk = nullptr; hip_check(rc, "sylph_sketch_set_option(dedup_fpr)"); }
        }
    }
    ~Session() { sylph_sketch_destroy(sk); }
    // keep != nullptr: the caller takes the pushed, unfinished session (the profile pipeline finishes it on the device and
    // probes its table where it lies); out's table stays empty
    void finish_or_keep(SequencesSketch& out, sylph_sketch** keep) {
        if (keep) { *keep = sk; sk = nullptr; return; }
        finish(out);
    }
    void finish(SequencesSketch& out) {
        uint64_t* k = nullptr; uint32_t* c = nullptr; uint64_t n = 0, dup = 0;
        hip_check(sylph_sketch_finish(sk, &k, &c, &n, &dup), "sylph_sketch_finish");
        out.kmers = take(k, n);
        out.counts = take(c, n);
    }
};

// ---- engine.cpp: the background threads ----
// Work that nobody waits for (unmapping a sample's files, handing inflated copies back) runs on ONE long-lived reaper thread;
// join_background() waits for it.
void background(std::function<void()> f);
// ... and one thread that writes finished sketches out, in the order they were finished, while their worker is at its next sample
// (a 1 Gbp pair's .sylsp: 48 MB, 25-35 ms of a warm sample's ~120); always drained before the command returns
void write_behind(std::function<void()> f);
void drain_writers();

// ---- sample_feed.cpp: the way of one sample's reads to the device ----
// second: the mate file of a pair.  interleaved (--interleaved; no second file): `first` holds the pairs itself, mate 1, mate 2,
// mate 1, ... — the sample means what `-1 A -2 B` means with A = its even records and B = its odd ones (csrc/interleave_plan.h);
// mate_check: every pair's two ids are checked before it is pushed (--no-mate-check turns that off)
struct SampleFiles {
    std::string first;
    std::optional<std::string> second;
    bool interleaved = false, mate_check = true;
    bool paired() const { return second.has_value() || interleaved; }
};
struct SampleParams {
    uint64_t c = 0, k = 0;
    bool no_dedup = false;
    double dedup_fpr = 0.;   // pairs only (Session)
    std::optional<std::string> sample_name;
};
// needletail's test for a compressed file: the first two bytes (1f 8b / "BZ"), of a regular file only — never read from a pipe
// here: the bytes would be gone for its reader
enum class Container { Plain, Gzip, Bzip2 };
Container container_of(const std::string& path);
// The device decodes files of this container (csrc/inflate.hip, csrc/bunzip2.hip: their COMPRESSED bytes travel) unless
// SYLPH_HIP_INFLATE_DEVICE=0 / SYLPH_HIP_BUNZIP2_DEVICE=0 keep the host's decoder; both need device_feed_enabled().  Plain: false.
bool device_decode_enabled(Container c);

// SYLPH_HIP_FEED_TRACE: "[sylph_hip feed] <what> <milliseconds since the previous lap>" (tools/gz_e2e_trace.py and
// tools/feed_trace.sh read these lines)
struct FeedLaps {
    static bool on() { static const bool t = getenv("SYLPH_HIP_FEED_TRACE") != nullptr; return t; }
    std::chrono::steady_clock::time_point prev = std::chrono::steady_clock::now();
    void lap(const char* what) {
        if (!on()) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[sylph_hip feed] %-28s %8.3f ms\n", what, std::chrono::duration<double>(t - prev).count() * 1e3);
        prev = t;
    }
};

// The files of a sample as the block-parallel host feed wants them: mapped (or inflated) and indexed
struct IndexedInput { std::unique_ptr<FastqIndex> a, b; };
// The index of the NEXT sample's files is built on a background thread while the current sample is gathered and pushed
// (the files of a sample are independent of everything before them).  get(j) hands over what start(j) began — or builds it
// now; at most `ahead` samples are in flight, so the memory of their mappings and index arrays stays bounded.
class IndexAhead {
   public:
    IndexAhead(std::vector<SampleFiles> files) : files_(std::move(files)) {}
    ~IndexAhead() { for (auto& kv : fut_) if (kv.second.valid()) kv.second.wait(); }
    const SampleFiles& files(size_t j) const { return files_.at(j); }
    size_t size() const { return files_.size(); }
    void start(size_t j);
    std::optional<IndexedInput> get(size_t j);
   private:
    std::vector<SampleFiles> files_;
    std::mutex mu_;
    std::map<size_t, std::future<std::optional<IndexedInput>>> fut_;
};

// What a command's sample threads share about their feed
struct FeedShared {
    IndexAhead ahead;
    const size_t n_workers;
    std::atomic<size_t> indexes_obtained{0};   // the last one says: nobody will want a recycled inflate buffer any more
    FeedShared(std::vector<SampleFiles> files, size_t workers);   // also sets the feed's thread share and memory budget
};
// Which road sample j takes, decided where its worker takes it up.  An engine that is up takes plain FASTQ by the device route
// (no host index at all), gzip and bzip2 files that the device decodes whether it is up or not; a process's first plain sample,
// whose index is built while the GPU runtime initialises, and everything the device route declines go the host way.
struct SampleRoute {
    bool dev = false;                       // the device route is tried first
    Container decode = Container::Plain;    // ... with the device decoding this container (both mates are of it)
    // !dev: the files' index from IndexAhead (empty: they are not for the block-parallel feed), or — the index says neither ok
    // nor failed — the un-indexed text of a gzip file that the host inflated: the device route takes that text from memory
    std::optional<IndexedInput> pre;
    // first_use_hint (the sketch command; not query / profile, whose sample engines have always page-locked their buffers in the
    // bring-up): a compressed sample on the device route needs none of the page-locked feed buffers — an engine still in its bring-up
    // leaves them to whoever wants them first (~80 ms of hipHostMalloc that would run beside the sample's own allocations and
    // copies) and sends its warm-up sample down the text route; the route taken is marked in the trace
    SampleRoute(Engine& eng, FeedShared& feed, size_t j, bool first_use_hint);
    // the index goes (2 x 1 GB of mappings to unmap / inflated copies to hand back: 30-60 ms per sample) on the reaper thread, behind the sample
    ~SampleRoute();
    SampleRoute(const SampleRoute&) = delete;
    SampleRoute& operator=(const SampleRoute&) = delete;
};
// One sample's reads sketched (sketch.rs:897-959 single, :771-895 paired): nullopt where the reference returns None (warn + skip).
// keep != nullptr: the pushed, unfinished session is handed over instead of the table (Session::finish_or_keep).
std::optional<SequencesSketch> sketch_sample(Engine& e, const SampleFiles& files, const SampleParams& p, SampleRoute& route, sylph_sketch** keep);

// ---- cmd_sketch.cpp ----
// SYLPH_HIP_FASTA_DEVICE=1: genome files take the device road (csrc/fasta.hip: the file's bytes travel, the device decodes them, finds
// the FASTA records and joins the sequences); unset or 0 keeps the host reader.  The road needs device_feed_enabled().
bool fasta_device_enabled();
// One genome file on the device road: its FASTA index and, for a compressed file, the decoded text the index borrows (shared by the
// files of one decode call; an index goes before its text)
struct DeviceGenomeFile {
    std::string file;
    std::shared_ptr<sylph_inflated> text;
    std::unique_ptr<sylph_fasta, void (*)(sylph_fasta*)> fa{nullptr, sylph_fasta_destroy};
    uint64_t text_bytes = 0, n_records = 0, n_bases = 0, id_bytes = 0;
};
// The per-batch limit of bases, L: 2^32 - 4096 (csrc/genome_acc_plan.h PUSH_LIMIT), or a positive SYLPH_HIP_GENOME_PUSH_BASES below it (tests,
// small-memory nodes).  A batch holds fewer bases than L; a file with L bases or more is cut at record boundaries (GenomeBatch::append).
uint64_t genome_push_limit();
// A batch of genomes sketched by ONE sylph_sketch_genomes call (seeding, genome-wide duplicate removal and the spacing
// filter all run on the device; sketch.rs:550-622 / :481-548 per genome).  On the host road files are parsed on the host and appended
// until the batch holds BATCH_BASES; on the device road (add_files) indexed files are collected and sketched by ONE
// sylph_sketch_genomes_fasta call.  A batch is all-host or all-device: whichever road a file takes, the other road's batch is flushed
// first, so results come out in input order.
struct GenomeBatch {
    static constexpr uint64_t BATCH_BASES = 1ull << 30;
    Engine& e;
    uint64_t c, k, min_spacing;
    bool pseudotax;
    std::vector<GenomeSketch>& out;
    std::vector<uint8_t> bases;
    std::vector<uint64_t> off{0}, goff{0};
    std::vector<GenomeSketch> pending;   // names + gn_size of the genomes in the batch
    GenomeBatch(Engine& en, uint64_t c_, uint64_t k_, uint64_t sp, bool pt, std::vector<GenomeSketch>& o)
        : e(en), c(c_), k(k_), min_spacing(sp), pseudotax(pt), out(o) {}
    // One genome file read into memory: records concatenated, one offset per record.  Touches nothing of the batch, so any
    // number of files can be parsed (and inflated) at the same time (the reference reads its genome files on the rayon pool,
    // sketch.rs:422-476); warnings travel with the result so that they come out in file order.
    struct Parsed {
        std::string file;
        std::vector<uint8_t> bases;
        std::vector<uint64_t> ends;                 // end of every record in `bases`
        std::vector<std::string> ids;               // one per record (a warning about a record names it)
        std::vector<std::string> warnings;
        bool ok = false;
    };
    static Parsed parse_file(const std::string& ref_file, bool individual);
    // sketch_genome (individual = false) or sketch_genome_individual (true) up to the k-mer work; false = file skipped
    bool add_file(const std::string& ref_file, bool individual) { return append(parse_file(ref_file, individual), individual); }
    // files [0, n) parsed on up to `threads` threads, a window of them at a time, appended (and flushed) in file order
    void add_files(const std::vector<std::string>& files, bool individual, uint64_t threads);
    // A file below the batch limit joins the batch.  One of L bases or more (host_internal.hpp genome_push_limit) is cut into runs of
    // whole records below L by the plan's greedy rule: one genome per record, each run is a batch of its own (append_split: a record
    // of L bases or more is skipped, the others are sketched); one genome per file, the runs go through a device accumulator that
    // removes duplicates over the whole file (append_accumulated: a contig of L bases or more refuses the file).
    bool append(Parsed p, bool individual);
    bool append_split(const Parsed& p);
    bool append_accumulated(const Parsed& p);
    void flush();
    // one sylph_sketch_genomes call: genome g = contigs [goff_[g], goff_[g + 1]) of off_ over bases_; names[g] is filled and moved to `out`
    void sketch_batch(const uint8_t* bases_, const std::vector<uint64_t>& off_, const std::vector<uint64_t>& goff_, std::vector<GenomeSketch>& names);
    // the device road: files [lo, lo + n) read by the threads, decoded and indexed by this thread; what the device declines is parsed on
    // the host as before.  A group of indexed files is bounded by BATCH_BASES bytes of text and by the batch limit of bases.
    std::vector<DeviceGenomeFile> dev_group;
    uint64_t dev_text_bytes = 0, dev_bases = 0;
    bool dev_individual = false;
    void add_window_device(const std::vector<std::string>& files, size_t lo, size_t n, bool individual, uint64_t threads);
    void flush_device();
};

}  // namespace sylph_host
