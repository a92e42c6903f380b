// sample_feed.cpp — the roads one sample's reads can take to the device (the device route, the indexed host feed, the sequential
// reader), the choice between them, and the per-sample function behind the sketch / query / profile drivers
// (sketch.rs:771-959).
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

#include <cstring>

#include "host_internal.hpp"
#include "../csrc/interleave_plan.h"

namespace sylph_host {

namespace ip = sylph::interleave_plan;

bool exact_dedup_accepted(bool flag) {
    const char* e = getenv("SYLPH_HIP_EXACT_DEDUP");
    return flag || (e && *e && strcmp(e, "0") != 0);
}
Container container_of(const std::string& f) {
    struct stat st;
    if (stat(f.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) return Container::Plain;
    FILE* fp = fopen(f.c_str(), "rb");
    if (!fp) return Container::Plain;
    unsigned char h[2] = {0, 0};
    const size_t n = fread(h, 1, 2, fp);
    fclose(fp);
    if (n == 2 && h[0] == 0x1f && h[1] == 0x8b) return Container::Gzip;
    if (n == 2 && h[0] == 'B' && h[1] == 'Z') return Container::Bzip2;
    return Container::Plain;
}
bool device_decode_enabled(Container c) {
    auto on = [](const char* name) {
        if (!device_feed_enabled()) return false;
        if (const char* e = getenv(name)) return atoi(e) != 0;
        return true;
    };
    static const bool gzip = on("SYLPH_HIP_INFLATE_DEVICE"), bzip2 = on("SYLPH_HIP_BUNZIP2_DEVICE");
    return c == Container::Gzip ? gzip : c == Container::Bzip2 ? bzip2 : false;
}

namespace {
// An interleaved sample found out of phase by one of the roads (the warning is out): sketch_sample drops the session and gives no
// sketch, as behind any invalid file.
struct SampleSkipped {};
std::string id_of_header(const uint8_t* h, size_t n) { return std::string((const char*)h, (size_t)ip::id_len(h, n)); }
void warn_out_of_phase(const std::string& file, uint64_t pair, const std::string& id1, const std::string& id2) {
    warn("Interleaved file " + file + ": records " + std::to_string(ip::record_of(pair, 0)) + " and " + std::to_string(ip::record_of(pair, 1)) +
         " are not mates ('" + id1 + "' and '" + id2 + "'): the file is out of phase from there on; skipping the sample (--no-mate-check takes the records as they come).");
}
// Uncompressed 4-line FASTQ (the common case): the files are indexed by parse_threads() workers, whole batches are gathered
// into page-locked memory in parallel and pushed; the record loop of the reference shrinks to its one sequential piece, the
// running mean of the read lengths (f64, file order: sketch.rs:941-943, :825-826), which runs on its own thread meanwhile.
// index_inputs returns nothing when a file is not that simple (gzip, FASTA, blank lines, a malformed record anywhere): the
// caller then runs the sequential reader with needletail's exact record/error semantics.  No GPU call happens before the
// files are indexed, so the engine's background bring-up overlaps with it.
// build = false: the files are mapped / inflated, not indexed — what the device-side route needs of a gzip file (finish_index does
// the rest on the host when that route is not taken after all)
std::optional<IndexedInput> index_inputs(const SampleFiles& files, bool build = true) {
    if (getenv("SYLPH_HIP_SEQUENTIAL_FEED")) return std::nullopt;
    const std::string& f1 = files.first;
    const std::string* f2 = files.second ? &*files.second : nullptr;
    const unsigned T = parse_threads();
    IndexedInput in;
    std::exception_ptr err_b;
    std::thread tb;
    ThreadJoiner jb{tb};
    if (f2) tb = std::thread([&] {                        // the two mate files are indexed concurrently
        try { in.b.reset(new FastqIndex(*f2, T, build)); } catch (...) { err_b = std::current_exception(); }
    });
    in.a.reset(new FastqIndex(f1, T, build));
    if (tb.joinable()) tb.join();
    if (err_b) std::rethrow_exception(err_b);
    if (build ? (!in.a->ok || (f2 && !in.b->ok)) : (!in.a->text_ready || (f2 && !in.b->text_ready))) return std::nullopt;
    return in;
}
bool finish_index(IndexedInput& in) {
    const unsigned T = parse_threads();
    std::exception_ptr err_b;
    std::thread tb;
    ThreadJoiner jb{tb};
    if (in.b) tb = std::thread([&] { try { in.b->build_index(T); } catch (...) { err_b = std::current_exception(); } });
    in.a->build_index(T);
    if (tb.joinable()) tb.join();
    if (err_b) std::rethrow_exception(err_b);
    return in.a->ok && (!in.b || in.b->ok);
}
// Batches of whole records (pairs) of at most BATCH_BASES bases / BATCH_RECS records
// (interleaved: pairs of ONE file, item i = its records 2 i and 2 i + 1)
std::vector<std::pair<size_t, size_t>> cut_batches(size_t n, bool paired, const std::vector<uint64_t>& ca, const std::vector<uint64_t>& cb, bool interleaved = false) {
    std::vector<std::pair<size_t, size_t>> out;
    size_t i0 = 0;
    while (i0 < n) {
        // largest i1 with at most BATCH_BASES bases and BATCH_RECS records in [i0, i1)
        size_t lo = i0 + 1, hi = std::min(n, i0 + PinnedBatch::BATCH_RECS / (paired || interleaved ? 2 : 1));
        auto bases_upto = [&](size_t i) {
            return interleaved ? ca[ip::record_of(i, 0)] - ca[ip::record_of(i0, 0)] : ca[i] - ca[i0] + (paired ? cb[i] - cb[i0] : 0);
        };
        while (lo < hi) {
            const size_t mid = lo + (hi - lo + 1) / 2;
            if (bases_upto(mid) <= PinnedBatch::BATCH_BASES) lo = mid; else hi = mid - 1;
        }
        out.emplace_back(i0, lo);
        i0 = lo;
    }
    return out;
}
// open_session: creates the sample's session — it waits for the engine's context, so it is called as late as possible: whatever
// batches can be gathered and packed before the context is up (the first sample of a process: ~0.15 s of idle parse threads otherwise)
// are gathered into pageable memory first (round 5)
// the mate check of the indexed host feed: the header of a record is the line in front of its sequence line
void check_mates_indexed(const std::string& file, const FastqIndex& a, size_t n_pairs, unsigned threads) {
    auto header = [&](size_t r, size_t& len) {
        const size_t end = (size_t)a.seq_off[r] - 1;                         // the header line's '\n'
        const void* nl = end ? memrchr(a.data, '\n', end) : nullptr;
        const size_t at = nl ? (size_t)((const uint8_t*)nl - a.data) + 1 : 0;   // its '@'
        len = end - at - 1;
        return a.data + at + 1;
    };
    std::atomic<uint64_t> bad{n_pairs};
    const size_t CHUNK = 4096;
    parallel_for((n_pairs + CHUNK - 1) / CHUNK, threads, [&](size_t c) {
        const size_t p1 = std::min(n_pairs, (c + 1) * CHUNK);
        for (size_t p = c * CHUNK; p < p1 && p < bad.load(std::memory_order_relaxed); p++) {
            size_t l1 = 0, l2 = 0;
            const uint8_t *h1 = header(ip::record_of(p, 0), l1), *h2 = header(ip::record_of(p, 1), l2);
            if (ip::mates(h1, ip::id_len(h1, l1), h2, ip::id_len(h2, l2))) continue;
            uint64_t seen = bad.load();
            while (p < seen && !bad.compare_exchange_weak(seen, p)) {}
            break;
        }
    });
    const uint64_t p = bad.load();
    if (p >= n_pairs) return;
    size_t l1 = 0, l2 = 0;
    const uint8_t *h1 = header(ip::record_of(p, 0), l1), *h2 = header(ip::record_of(p, 1), l2);
    warn_out_of_phase(file, p, id_of_header(h1, l1), id_of_header(h2, l2));
    throw SampleSkipped{};
}
void sketch_indexed(Engine& e, const std::function<sylph_sketch*()>& open_session, const IndexedInput& in, double& mean_read_length, const SampleFiles& files) {
    const unsigned T = parse_threads();
    FeedLaps laps;
    const FastqIndex& a = *in.a;
    const FastqIndex* b = in.b.get();
    const bool il = files.interleaved;                                       // pairs from consecutive records of ONE index (interleave_plan.h)
    const size_t n = il ? (size_t)ip::pairs_of(a.n_records()) : b ? std::min(a.n_records(), b->n_records()) : a.n_records();   // lock-step readers: sketch.rs:813-815
    const size_t step = il ? 2 : 1;                                          // records of `a` per item
    if (il && files.mate_check) {
        check_mates_indexed(files.first, a, n, T);
        laps.lap("host feed: interleaved mates checked");
    }
    static const std::vector<uint64_t> no_cum;
    const std::vector<uint64_t>& ca = a.cum;                             // prefix sums of the read lengths, from the index workers
    const std::vector<uint64_t>& cb = b ? b->cum : no_cum;
    // the one sequential piece of the reference's record loop (f64, file order: sketch.rs:941-943, :825-826), on its own thread
    // while the batches travel
    double mean = 0.;
    std::thread tm([&] { double counter = 0.; for (size_t i = 0; i < n; i++) { counter += 1.; mean = mean + ((double)a.seq_len[step * i] - mean) / counter; } });
    ThreadJoiner jm{tm};
    const auto batches = cut_batches(n, b != nullptr, ca, cb, il);
    size_t early = 0;
    constexpr size_t MAX_EARLY = 16;                                     // 4 Gbp = 1 GB of packed bases in pageable memory at most
    while (!e.ready() && early < batches.size() && early < MAX_EARLY) {
        e.batch.gather_packed_early(a, b, ca, b ? &cb : nullptr, step * batches[early].first, step * batches[early].second, T);
        early++;
    }
    if (early) laps.lap("early batches: gather + pack (context still coming up)");
    sylph_sketch* const sk = open_session();
    e.batch.flush(sk);
    if (early) {
        e.batch.push_early(sk);
        if (early < batches.size()) {
            a.release_behind(a.seq_off[step * batches[early].first]);
            if (b) b->release_behind(b->seq_off[batches[early].first]);
        }
        laps.lap("early batches: pushed");
    }
    // Batches are gathered AND packed to 2 bits per base by the parse threads into one of two page-locked slots while the other
    // slot is on its way to the device: the push of batch i (PCIe + kernels) hides behind the gather of batch i + 1.
    if (early < batches.size()) {
        e.wait_pinned();
        e.batch.gather_packed((int)(early & 1), a, b, ca, b ? &cb : nullptr, step * batches[early].first, step * batches[early].second, T);
        laps.lap(il ? "batch: gather + pack (interleaved)" : "batch: gather + pack");
    }
    for (size_t bi = early; bi < batches.size(); bi++) {
        std::exception_ptr err;
        std::thread tg;
        ThreadJoiner jg{tg};
        if (bi + 1 < batches.size())
            tg = std::thread([&, bi] {
                try { e.batch.gather_packed((int)((bi + 1) & 1), a, b, ca, b ? &cb : nullptr, step * batches[bi + 1].first, step * batches[bi + 1].second, T); }
                catch (...) { err = std::current_exception(); }
            });
        e.batch.push_packed(sk, (int)(bi & 1));
        if (tg.joinable()) tg.join();
        if (err) std::rethrow_exception(err);
        // everything before the next batch's first record has been gathered: an inflated copy gives those pages back
        if (bi + 1 < batches.size()) {
            a.release_behind(a.seq_off[step * batches[bi + 1].first]);
            if (b) b->release_behind(b->seq_off[batches[bi + 1].first]);
        }
        laps.lap(il ? "batch: push || gather next (interleaved)" : "batch: push || gather next");
    }
    tm.join();
    mean_read_length = mean;
    laps.lap("running mean (joined)");
}

// Round 5, the device-side route for plain FASTQ (csrc/fastq.hip): the files' TEXT goes to the device through the engine's uploader and
// the library finds the records there; the host keeps the one sequential piece (the running mean of the mate-1 read lengths, from the
// lengths the device hands back).  Taken for every sample whose engine is already up — a process's FIRST sample is indexed and gathered
// on the host while the GPU runtime initialises, which no device can do — unless SYLPH_HIP_FEED_DEVICE=0 (feed.cpp device_feed_enabled).
// Returns false, having pushed
// nothing, when the files are not text the device indexes (SYLPH_ERR_FORMAT): the caller takes the host route, whose
// record and error semantics are needletail's.
// FASTA-format reads (csrc/fasta.hip sylph_sketch_push_fasta): the first byte of each mate's TEXT says which index finds its records
// ('@': sylph_fastq_*, '>': sylph_fasta_*; ReadIndex below holds the two behind one set of calls); mates of different kinds, and
// FASTA reads with SYLPH_HIP_FASTA_READS_DEVICE=0, are declined.  A plain FASTA sample waits for the engine even as a process's
// first: its host road is the sequential reader.
// `text`: the files' text where it lies in host memory already (the inflated copies of gzip files) instead of the files themselves
// Round 6, gzip on the device (csrc/inflate.hip): a sample whose files are gzip sends their COMPRESSED bytes (0.4 B per base instead of
// 2.1) and the library inflates them there — sylph_inflate; SYLPH_HIP_INFLATE_DEVICE=0 keeps the host's inflate.  What the library
// declines (SYLPH_ERR_FORMAT: damaged, not gzip after all, a stream it does not take; SYLPH_ERR_NOMEM) goes the host way, whose
// error semantics are needletail's.
// bzip2 on the device (csrc/bunzip2.hip), the same way: the compressed bytes travel, sylph_bunzip2_files decodes them there;
// SYLPH_HIP_BUNZIP2_DEVICE=0 keeps the host's reader (libbz2 in FastxReader).  What the library declines goes the host way.
// A gzip or bzip2 sample too large for one piece, or one the device has no room for in one piece, is STREAMED through the same decoder in
// bounded memory (sketch_streamed below; SYLPH_HIP_INFLATE_STREAM / SYLPH_HIP_BUNZIP2_STREAM).
// `decode`: the container the device decodes (SampleRoute: both mates are of it, device_decode_enabled says yes); Plain: text travels.
namespace {
struct MappedFile {                       // the compressed bytes of one file (read-only mapping of the page cache)
    const uint8_t* data = nullptr;
    size_t size = 0;
    explicit MappedFile(const std::string& path) {
        const int fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) return;
        struct stat st;
        if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) {
            void* p = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
            if (p != MAP_FAILED) { data = (const uint8_t*)p; size = (size_t)st.st_size; }
        }
        close(fd);
    }
    MappedFile(const MappedFile&) = delete;
    MappedFile& operator=(const MappedFile&) = delete;
    ~MappedFile() { if (data) munmap(const_cast<uint8_t*>(data), size); }
};
struct InflatedText { sylph_inflated* h = nullptr; ~InflatedText() { sylph_inflated_destroy(h); } };

// The two kinds of read text the device indexes (csrc/fastq.hip, csrc/fasta.hip) behind one set of calls: a route is written once and
// asks the text's first byte which kind it is ('@': four-line FASTQ, '>': FASTA; needletail decides the same way).
struct ReadIndex {
    bool fasta = false;
    sylph_fastq* q = nullptr;
    sylph_fasta* a = nullptr;
    ReadIndex() = default;
    ReadIndex(const ReadIndex&) = delete;
    ReadIndex& operator=(const ReadIndex&) = delete;
    ~ReadIndex() { sylph_fastq_destroy(q); sylph_fasta_destroy(a); }
    bool made() const { return q || a; }
    void reset() { sylph_fastq_destroy(q); sylph_fasta_destroy(a); q = nullptr; a = nullptr; }
    const char* index_name() const { return fasta ? "sylph_fasta_index" : "sylph_fastq_index"; }
    const char* index_window_name() const { return fasta ? "sylph_fasta_index_window" : "sylph_fastq_index_window"; }
    const char* push_name() const { return fasta ? "sylph_sketch_push_fasta" : "sylph_sketch_push_fastq"; }
    const char* push_interleaved_name() const { return fasta ? "sylph_sketch_push_fasta_interleaved" : "sylph_sketch_push_fastq_interleaved"; }
    // an interleaved text: pairs [first_pair, +n_pairs) of this one index; the first of them that is not one of mates (n_pairs: none)
    static int push_interleaved(sylph_sketch* sk, const ReadIndex& f, uint64_t first_pair, uint64_t n_pairs) {
        return f.fasta ? sylph_sketch_push_fasta_interleaved(sk, f.a, first_pair, n_pairs) : sylph_sketch_push_fastq_interleaved(sk, f.q, first_pair, n_pairs);
    }
    uint64_t first_bad_pair(uint64_t first_pair, uint64_t n_pairs) const {
        uint64_t bad = n_pairs;
        hip_check(fasta ? sylph_fasta_mates(a, first_pair, n_pairs, &bad) : sylph_fastq_mates(q, first_pair, n_pairs, &bad), "sylph_fastx_mates");
        return bad;
    }
    int index(sylph_ctx* ctx, const void* dev, uint64_t bytes) {
        return fasta ? sylph_fasta_index(ctx, dev, bytes, SYLPH_MEM_DEVICE, &a) : sylph_fastq_index(ctx, dev, bytes, SYLPH_MEM_DEVICE, &q);
    }
    int index_window(sylph_ctx* ctx, const void* dev, uint64_t bytes, int final, uint64_t* consumed) {
        return fasta ? sylph_fasta_index_window(ctx, dev, bytes, SYLPH_MEM_DEVICE, final, &a, consumed)
                     : sylph_fastq_index_window(ctx, dev, bytes, SYLPH_MEM_DEVICE, final, &q, consumed);
    }
    void counts(uint64_t& n_rec, uint64_t& bases) const {
        hip_check(fasta ? sylph_fasta_counts(a, &n_rec, &bases, nullptr) : sylph_fastq_counts(q, &n_rec, &bases), "sylph_fastx_counts");
    }
    uint64_t record_offset(uint64_t record) const {
        uint64_t at = 0;
        hip_check(fasta ? sylph_fasta_record_offset(a, record, &at) : sylph_fastq_record_offset(q, record, &at), "sylph_fastx_record_offset");
        return at;
    }
    static int push(sylph_sketch* sk, const ReadIndex& m1, const ReadIndex* m2, uint64_t first, uint64_t n_items) {
        return m1.fasta ? sylph_sketch_push_fasta(sk, m1.a, m2 ? m2->a : nullptr, first, n_items)
                        : sylph_sketch_push_fastq(sk, m1.q, m2 ? m2->q : nullptr, first, n_items);
    }
};
// the sequence lengths of records [0, n) of an index (u32 from the FASTQ index, u64 from the FASTA one), for the one sequential piece
// of the reference's record loop: the running mean of the mate-1 read lengths (f64, file order: sketch.rs:941-943, :825-826)
struct ReadLengths {
    std::vector<uint32_t> q;
    std::vector<uint64_t> a;
    bool fasta = false;
    void fetch(const ReadIndex& x, uint64_t n) {
        fasta = x.fasta;
        if (fasta) { a.resize(n); hip_check(sylph_fasta_lengths(x.a, 0, n, a.data()), "sylph_fasta_lengths"); }
        else { q.resize(n); hip_check(sylph_fastq_lengths(x.q, 0, n, q.data()), "sylph_fastq_lengths"); }
    }
    uint64_t at(uint64_t i) const { return fasta ? a[i] : q[i]; }
    // stride 2: over the mate-1 records of an interleaved text, the even ones (interleave_plan.h MEAN_STRIDE); n counts the steps
    void continue_mean(uint64_t n, double& mean, double& counter, uint64_t stride = 1) const {
        if (fasta) for (uint64_t i = 0; i < n; i++) { counter += 1.; mean = mean + ((double)a[stride * i] - mean) / counter; }
        else for (uint64_t i = 0; i < n; i++) { counter += 1.; mean = mean + ((double)q[stride * i] - mean) / counter; }
    }
};
// what a road knows about the one file of an interleaved sample
struct Interleave { bool on = false, check = true; };
// The ids of pair `bad` of an index that knows where its records start, read from the text through read(offset, n, dst) — the text
// lies on the device or in a file —, in the warning that ends the sample.  pair: the pair's number in the file.
template <class Read>
[[noreturn]] void skip_out_of_phase(const std::string& file, const ReadIndex& x, uint64_t bad, uint64_t pair, uint64_t text_bytes, Read&& read) {
    std::string id[2];
    for (uint32_t m = 0; m < 2; m++) {
        const uint64_t at = std::min(x.record_offset(ip::record_of(bad, m)), text_bytes);
        uint8_t buf[1024];
        const uint64_t n = std::min<uint64_t>(sizeof(buf), text_bytes - at);
        if (n < 2 || !read(at, n, buf)) continue;
        const uint8_t* end = (const uint8_t*)memchr(buf + 1, '\n', n - 1);
        id[m] = id_of_header(buf + 1, end ? (size_t)(end - (buf + 1)) : (size_t)n - 1);
    }
    warn_out_of_phase(file, pair, id[0], id[1]);
    throw SampleSkipped{};
}
// pushes of whole pairs of an interleaved text below 2^31 bases and 2^30 pairs (l: the lengths of its records 0 .. 2 n_pairs)
std::vector<std::pair<uint64_t, uint64_t>> cut_pushes_interleaved(const ReadLengths& l, uint64_t n_pairs, uint64_t bases) {
    std::vector<std::pair<uint64_t, uint64_t>> pushes;
    if (bases < (1ull << 31) && n_pairs < (1ull << 29)) {
        if (n_pairs) pushes.emplace_back(0, n_pairs);
        return pushes;
    }
    uint64_t i0 = 0, sum = 0;
    for (uint64_t i = 0; i < n_pairs; i++) {
        const uint64_t len = l.at(ip::record_of(i, 0)) + l.at(ip::record_of(i, 1));
        if (i > i0 && (sum + len >= (1ull << 31) || i - i0 >= (1ull << 29))) { pushes.emplace_back(i0, i - i0); i0 = i; sum = 0; }
        sum += len;
    }
    if (n_pairs > i0) pushes.emplace_back(i0, n_pairs - i0);
    return pushes;
}
// pushes of whole records (pairs) below 2^31 bases and 2^30 items: one for anything up to ~2 Gbp
std::vector<std::pair<uint64_t, uint64_t>> cut_pushes(const ReadIndex* m2, const ReadLengths& l1, uint64_t n, uint64_t bases) {
    std::vector<std::pair<uint64_t, uint64_t>> pushes;
    if (bases < (1ull << 31) && n < (1ull << 30)) {
        if (n) pushes.emplace_back(0, n);
        return pushes;
    }
    ReadLengths l2;
    if (m2) l2.fetch(*m2, n);
    uint64_t i0 = 0, sum = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t l = l1.at(i) + (m2 ? l2.at(i) : 0);
        if (i > i0 && (sum + l >= (1ull << 31) || i - i0 >= (1ull << 30))) { pushes.emplace_back(i0, i - i0); i0 = i; sum = 0; }
        sum += l;
    }
    if (n > i0) pushes.emplace_back(i0, n - i0);
    return pushes;
}
// FASTA-format reads take the device routes unless SYLPH_HIP_FASTA_READS_DEVICE=0 keeps them on the host reader: every kind of sample
// (plain, gzip, bzip2, gzip streamed) measured 2.4 to 9.4 times faster there (profiles/fasta_reads_device.txt)
bool fasta_reads_on_device() {
    static const bool on = [] { const char* e = getenv("SYLPH_HIP_FASTA_READS_DEVICE"); return !(e && *e) || atoi(e) != 0; }();
    return on;
}
// mates of one kind: both FASTA or neither (h: the first byte of every mate's text)
bool same_kind(const std::vector<uint8_t>& h) { return h.size() < 2 || ((h[0] == '>') == (h[1] == '>')); }
// a text of this many bytes or more is not indexed in one piece by sylph_fasta_index (include/sylph_hip.h)
constexpr uint64_t FASTA_INDEX_MAX_TEXT = (1ull << 32) - 4096;
// the first byte of a decoded file's text, which lies on the device
uint8_t first_byte_of(sylph_inflated* t, const void* dev_file) {
    const void* base = nullptr;
    uint8_t c = 0;
    hip_check(sylph_inflated_text(t, &base, nullptr), "sylph_inflated_text");
    hip_check(sylph_inflated_read(t, (uint64_t)((const uint8_t*)dev_file - (const uint8_t*)base), 1, &c), "sylph_inflated_read");
    return c;
}
// ... of a regular file (0 for anything else: a pipe can be read once, front to back, and nothing may peek at it)
uint8_t first_byte_of(const std::string& file) {
    uint8_t c = 0;
    struct stat st;
    if (stat(file.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) return 0;
    const int fd = open(file.c_str(), O_RDONLY);
    if (fd < 0) return 0;
    if (pread(fd, &c, 1, 0) != 1) c = 0;
    close(fd);
    return c;
}

// The streamed decoder of a container (csrc/inflate.hip sylph_inflate_stream_*, csrc/bunzip2.hip sylph_bunzip2_stream_*) behind one set of
// calls, as ReadIndex holds the two indexes: the stream route is written once.  mode_env: "auto" (default: the stream takes what the
// whole-file road declines for size or for room), "1" always, "0" never; whole_max_env lowers the bytes (both mates together) from which
// the whole-file road is not tried (the tests); slice_env sets the slice.
struct StreamDecoder {
    const char *container, *verb, *whole_name, *open_name, *next_name, *mode_env, *whole_max_env, *slice_env;
    uint64_t whole_max;                              // of the whole-file road itself
    int (*whole)(sylph_ctx*, const void* const*, const uint64_t*, uint32_t, int, sylph_inflated**);
    int (*open)(sylph_ctx*, const void* const*, const uint64_t*, uint32_t, int, uint64_t, void**);
    int (*next)(void*, const uint8_t*, const uint64_t*, sylph_inflated**, uint8_t*);
    int (*info)(const void*, uint64_t*, uint64_t*, uint64_t*, uint64_t*);
    void (*destroy)(void*);
};
const StreamDecoder GZIP_STREAM{
    "gzip", "inflated", "sylph_inflate_files", "sylph_inflate_stream_open", "sylph_inflate_stream_next", "SYLPH_HIP_INFLATE_STREAM", "SYLPH_HIP_INFLATE_WHOLE_MAX", "SYLPH_HIP_INFLATE_SLICE",
    SYLPH_INFLATE_WHOLE_MAX_BYTES, sylph_inflate_files,
    [](sylph_ctx* c, const void* const* p, const uint64_t* n, uint32_t f, int mem, uint64_t slice, void** out) { return sylph_inflate_stream_open(c, p, n, f, mem, slice, (sylph_inflate_stream**)out); },
    [](void* h, const uint8_t* adv, const uint64_t* keep, sylph_inflated** w, uint8_t* fin) { return sylph_inflate_stream_next((sylph_inflate_stream*)h, adv, keep, w, fin); },
    [](const void* h, uint64_t* a, uint64_t* b, uint64_t* c, uint64_t* d) { return sylph_inflate_stream_info((const sylph_inflate_stream*)h, a, b, c, d); },
    [](void* h) { sylph_inflate_stream_destroy((sylph_inflate_stream*)h); }};
const StreamDecoder BZIP2_STREAM{
    "bzip2", "decoded", "sylph_bunzip2_files", "sylph_bunzip2_stream_open", "sylph_bunzip2_stream_next", "SYLPH_HIP_BUNZIP2_STREAM", "SYLPH_HIP_BUNZIP2_WHOLE_MAX", "SYLPH_HIP_BUNZIP2_SLICE",
    ~0ull, sylph_bunzip2_files,
    [](sylph_ctx* c, const void* const* p, const uint64_t* n, uint32_t f, int mem, uint64_t slice, void** out) { return sylph_bunzip2_stream_open(c, p, n, f, mem, slice, (sylph_bunzip2_stream**)out); },
    [](void* h, const uint8_t* adv, const uint64_t* keep, sylph_inflated** w, uint8_t* fin) { return sylph_bunzip2_stream_next((sylph_bunzip2_stream*)h, adv, keep, w, fin); },
    [](const void* h, uint64_t* a, uint64_t* b, uint64_t* c, uint64_t* d) { return sylph_bunzip2_stream_info((const sylph_bunzip2_stream*)h, a, b, c, d); },
    [](void* h) { sylph_bunzip2_stream_destroy((sylph_bunzip2_stream*)h); }};
enum class StreamMode { Auto, Always, Never };
StreamMode stream_mode(const StreamDecoder& d) {
    const char* e = getenv(d.mode_env);
    if (!e || !*e || !strcmp(e, "auto")) return StreamMode::Auto;
    return atoi(e) != 0 ? StreamMode::Always : StreamMode::Never;
}
uint64_t env_bytes(const char* name, uint64_t otherwise) {
    const char* e = getenv(name);
    if (!e || !*e) return otherwise;
    const unsigned long long v = strtoull(e, nullptr, 10);
    return v ? (uint64_t)v : otherwise;
}
// compressed bytes (both mates together) from which the whole-file road declines
uint64_t whole_max(const StreamDecoder& d) { return std::min<uint64_t>(env_bytes(d.whole_max_env, d.whole_max), d.whole_max); }

// The stream route for gzip and bzip2 samples (StreamDecoder): the compressed bytes go to the device one slice per mate
// at a time, the records of every window are found there and pushed, and what a window holds beyond its last pushed record is kept for
// the next one — memory is a function of the slice, not of the sample (the reference streams records in O(batch) memory too:
// sketch.rs:780-781, :806-815, :906).  Per step: next; index each mate's window (final = the file's finished flag; the FASTQ or the FASTA index, by the first byte of the mate's text); push
// min(complete records of mate 1, of mate 2) pairs; keep every mate's text from its first record that was not pushed; advance only the
// mate with fewer records waiting (both when they are level), which bounds the carried text.  Surplus records of the longer mate are
// dropped at the end (lock-step readers, sketch.rs:813-815); the running mean of the mate-1 lengths is the same f64 recurrence in
// file order, continued across windows.  false: declined at some step (the session is the caller's to drop: the host feed takes the
// sample from its start).
// An interleaved sample (il.on; one file, a paired session): every window's complete records are n, pairs_of(n) pairs are checked
// (il.check) and pushed, and the text is kept from record kept_record(n) on, so a kept tail always begins at an even record; the
// mean continues across the windows over the even records only.  A pair that fails the check ends the sample (SampleSkipped).
bool sketch_streamed(Engine& e, const StreamDecoder& dec, const std::function<sylph_sketch*()>& open_session, const std::vector<const void*>& ptrs,
                     const std::vector<uint64_t>& lens, const char* name, double& mean_read_length, Interleave il = {}) {
    const bool trace = FeedLaps::on();
    FeedLaps laps;
    sylph_ctx* ctx = e.context();
    const uint32_t F = (uint32_t)ptrs.size();
    struct Stream { const StreamDecoder& d; void* h = nullptr; ~Stream() { d.destroy(h); } } st{dec};
    auto declined = [&](int rc, const char* what) {
        if (rc != SYLPH_ERR_FORMAT && rc != SYLPH_ERR_NOMEM) hip_check(rc, what);
        if (trace) fprintf(stderr, "[sylph_hip feed] stream route declined %s at %s: %s\n", name, what, sylph_last_error());
        return false;
    };
    auto not_taken = [&](const char* why) {
        if (trace) fprintf(stderr, "[sylph_hip feed] stream route declined %s: %s\n", name, why);
        return false;
    };
    int rc = dec.open(ctx, ptrs.data(), lens.data(), F, SYLPH_MEM_HOST, env_bytes(dec.slice_env, 0), &st.h);
    if (rc != SYLPH_OK) return declined(rc, dec.open_name);
    sylph_sketch* const sk = open_session();
    e.batch.flush(sk);
    std::unique_ptr<InflatedText> prev;                        // the window of the step before: its kept tail is copied out of it by `next`
    std::vector<uint8_t> advance(F, 1), finished(F, 0);
    std::vector<uint64_t> keep(F, 0);
    ReadLengths la;
    double mean = 0., counter = 0.;
    uint64_t pairs = 0;
    std::vector<int> kind(F, -1);                              // 1: the mate's text is FASTA, 0: it is not, -1: no byte of it seen yet
    for (bool first = true;; first = false) {
        std::unique_ptr<InflatedText> win(new InflatedText());
        rc = dec.next(st.h, advance.data(), first ? nullptr : keep.data(), &win->h, finished.data());
        if (rc != SYLPH_OK) return declined(rc, dec.next_name);
        prev.reset();                                          // (its indexes went with the previous step's scope)
        std::vector<ReadIndex> fq(F);
        std::vector<uint64_t> n_rec(F, 0), bytes(F, 0), bases(F, 0);
        std::vector<const void*> dev(F, nullptr);
        for (uint32_t i = 0; i < F; i++) hip_check(sylph_inflated_file(win->h, i, &dev[i], &bytes[i]), "sylph_inflated_file");
        for (uint32_t i = 0; i < F; i++) {
            if (kind[i] >= 0 || !bytes[i]) continue;           // asked once, of the first text a mate shows
            kind[i] = first_byte_of(win->h, dev[i]) == '>';
            if (kind[i] && !fasta_reads_on_device()) return not_taken("FASTA reads stay on the host reader");
        }
        if (F == 2 && kind[0] >= 0 && kind[1] >= 0 && kind[0] != kind[1]) return not_taken("one mate is FASTA, the other is not");
        for (uint32_t i = 0; i < F; i++) {
            if (finished[i] && !bytes[i]) continue;            // nothing left of a finished file: no records
            uint64_t consumed = 0;
            fq[i].fasta = kind[i] > 0;
            rc = fq[i].index_window(ctx, dev[i], bytes[i], finished[i] ? 1 : 0, &consumed);
            if (rc != SYLPH_OK) return declined(rc, fq[i].index_window_name());
            fq[i].counts(n_rec[i], bases[i]);
        }
        const uint64_t n = il.on ? ip::pairs_of(n_rec[0]) : F == 2 ? std::min(n_rec[0], n_rec[1]) : n_rec[0];
        if (n && il.on) {
            if (il.check) {
                const uint64_t bad = fq[0].first_bad_pair(0, n);
                if (bad < n) {
                    const void* base = nullptr;
                    hip_check(sylph_inflated_text(win->h, &base, nullptr), "sylph_inflated_text");
                    const uint64_t file_at = (uint64_t)((const uint8_t*)dev[0] - (const uint8_t*)base);
                    skip_out_of_phase(name, fq[0], bad, pairs + bad, bytes[0],
                                      [&](uint64_t at, uint64_t len, uint8_t* dst) { return sylph_inflated_read(win->h, file_at + at, len, dst) == SYLPH_OK; });
                }
            }
            la.fetch(fq[0], ip::kept_record(n_rec[0]));
            la.continue_mean(n, mean, counter, ip::MEAN_STRIDE);   // sketch.rs:824-826: the mate-1 records
            for (const auto& p : cut_pushes_interleaved(la, n, bases[0])) {
                rc = ReadIndex::push_interleaved(sk, fq[0], p.first, p.second);
                if (rc == SYLPH_ERR_NOMEM) return declined(rc, fq[0].push_interleaved_name());
                hip_check(rc, fq[0].push_interleaved_name());
            }
            pairs += n;
        } else if (n) {
            la.fetch(fq[0], n);
            la.continue_mean(n, mean, counter);                // sketch.rs:941-943, :825-826
            for (const auto& p : cut_pushes(F == 2 ? &fq[1] : nullptr, la, n, bases[0] + (F == 2 ? bases[1] : 0))) {
                rc = ReadIndex::push(sk, fq[0], F == 2 ? &fq[1] : nullptr, p.first, p.second);
                if (rc == SYLPH_ERR_NOMEM) return declined(rc, fq[0].push_name());
                hip_check(rc, fq[0].push_name());
            }
            pairs += n;
        }
        bool all_done = true;
        for (uint32_t i = 0; i < F; i++) {
            keep[i] = bytes[i];
            if (fq[i].made()) keep[i] = std::min(fq[i].record_offset(il.on ? ip::kept_record(n_rec[i]) : n), bytes[i]);
            all_done = all_done && finished[i];
        }
        // a finished mate with nothing waiting ends the lock-step reading: the other mate's surplus is dropped (sketch.rs:813-815)
        bool starved = false;
        for (uint32_t i = 0; i < F && !il.on; i++) starved = starved || (finished[i] && n_rec[i] == n);
        if (all_done || starved) break;
        const uint64_t waiting0 = n_rec[0] - n, waiting1 = F == 2 ? n_rec[1] - n : 0;
        advance[0] = !finished[0] && (F == 1 || waiting0 <= waiting1 || finished[1]);
        if (F == 2) advance[1] = !finished[1] && (waiting1 <= waiting0 || finished[0]);
        fq.clear();                                            // the indexes borrow the window's text: they go first
        prev = std::move(win);
    }
    uint64_t n_slices = 0, text_bytes = 0, peak_scratch = 0, peak_window = 0;
    hip_check(dec.info(st.h, &n_slices, &text_bytes, &peak_scratch, &peak_window), "stream info");
    if (trace) {
        char what[192];
        snprintf(what, sizeof(what), "stream route: %s %s on the device in %llu slices (%llu %s%s records, %llu text bytes, peak scratch %llu, peak window %llu)",
                 dec.container, dec.verb, (unsigned long long)n_slices, (unsigned long long)pairs, il.on ? "interleaved pairs of " : "", kind[0] > 0 ? "FASTA" : "FASTQ", (unsigned long long)text_bytes, (unsigned long long)peak_scratch, (unsigned long long)peak_window);
        laps.lap(what);
    }
    mean_read_length = mean;
    return true;
}
}  // namespace

// The texts of a sample whose compressed files the device decodes, both mates in ONE call (sylph_inflate_files / sylph_bunzip2_files:
// one scan, one decode launch, one chain — the mates share a block's latency): the whole-file road, or — when asked, for what that
// road declines for size or for room, and for a FASTA text too long for one index — the stream (sketch_streamed).
enum class Decoded { OnDevice, Streamed, Declined };      // the texts lie on the device / the sample is sketched already / the host feed's
struct RouteTexts {
    std::vector<std::unique_ptr<MappedFile>> maps;   // the compressed files, for as long as a stream may still want them
    std::vector<const void*> ptrs;
    std::vector<uint64_t> lens;
    InflatedText owner;                              // of decoded texts (destroyed behind the indexes that borrow them: declared before them)
    std::vector<TextUploader::Text> texts;
    std::vector<uint8_t> heads;                      // the first byte of every mate's TEXT: '@' FASTQ, '>' FASTA
};
bool stream_sample(Engine& e, const StreamDecoder& dec, const std::function<sylph_sketch*()>& open_session, const RouteTexts& t, const char* name, FeedLaps& laps,
                   double& mean_read_length, Interleave il) {
    if (!sketch_streamed(e, dec, open_session, t.ptrs, t.lens, name, mean_read_length, il)) return false;
    if (il.on) laps.lap(&dec == &GZIP_STREAM ? "device route: interleaved gzip streamed through the device inflate" : "device route: interleaved bzip2 streamed through the device decoder");
    else laps.lap(&dec == &GZIP_STREAM ? "device route: gzip streamed through the device inflate" : "device route: bzip2 streamed through the device decoder");
    return true;
}
Decoded decode_on_device(Engine& e, const StreamDecoder& dec, const std::function<sylph_sketch*()>& open_session, const std::vector<std::string>& files, FeedLaps& laps,
                         RouteTexts& out, double& mean_read_length, Interleave il) {
    const bool trace = FeedLaps::on();
    const bool gz = &dec == &GZIP_STREAM;
    const char* name = files[0].c_str();
    std::vector<const void*>& ptrs = out.ptrs;
    std::vector<uint64_t>& lens = out.lens;
    uint64_t packed_bytes = 0;
    for (const auto& f : files) {
        out.maps.emplace_back(new MappedFile(f));
        if (!out.maps.back()->data) return Decoded::Declined;
        ptrs.push_back(out.maps.back()->data);
        lens.push_back(out.maps.back()->size);
        packed_bytes += out.maps.back()->size;
    }
    const bool may_stream = stream_mode(dec) == StreamMode::Auto;
    const bool too_large = packed_bytes >= whole_max(dec);
    bool streamed = stream_mode(dec) == StreamMode::Always || (may_stream && too_large);
    if (!streamed && too_large) {
        if (trace) fprintf(stderr, "[sylph_hip feed] device %s declined %s: %llu %s bytes, and the stream is off\n", gz ? "inflate" : "bunzip2", name,
                           (unsigned long long)packed_bytes, dec.container);
        return Decoded::Declined;
    }
    if (!streamed) {
        const int rc = dec.whole(e.context(), ptrs.data(), lens.data(), (uint32_t)ptrs.size(), SYLPH_MEM_HOST, &out.owner.h);
        if (rc == SYLPH_ERR_NOMEM && may_stream) {
            if (trace) fprintf(stderr, "[sylph_hip feed] device %s has no room for %s in one piece (%s): the stream takes it\n", gz ? "inflate" : "bunzip2", name, sylph_last_error());
            streamed = true;
        } else if (rc == SYLPH_ERR_FORMAT || rc == SYLPH_ERR_NOMEM) {
            if (trace) fprintf(stderr, "[sylph_hip feed] device %s declined %s: %s\n", gz ? "inflate" : "bunzip2", name, sylph_last_error());
            return Decoded::Declined;
        } else hip_check(rc, dec.whole_name);
    }
    if (!streamed) {
        bool fasta_too_long = false;
        for (uint32_t i = 0; i < ptrs.size(); i++) {
            const void* dev = nullptr;
            uint64_t bytes = 0;
            hip_check(sylph_inflated_file(out.owner.h, i, &dev, &bytes), "sylph_inflated_file");
            if (!bytes) return Decoded::Declined;
            out.texts.push_back(TextUploader::Text{(const uint8_t*)dev, bytes});
            out.heads.push_back(first_byte_of(out.owner.h, dev));
            fasta_too_long = fasta_too_long || (out.heads[i] == '>' && bytes >= FASTA_INDEX_MAX_TEXT);
        }
        laps.lap(gz ? "device route: gzip inflated on the device" : "device route: bzip2 decoded on the device");
        // a FASTA text too long for one FASTA index: the stream's windows are smaller
        if (may_stream && fasta_too_long && same_kind(out.heads) && fasta_reads_on_device()) {
            if (trace) fprintf(stderr, "[sylph_hip feed] device route: a FASTA text of %s is too long for one index: the stream takes it\n", name);
            out.texts.clear();
            sylph_inflated_destroy(out.owner.h);
            out.owner.h = nullptr;
            streamed = true;
        }
    }
    if (!streamed) return Decoded::OnDevice;
    return stream_sample(e, dec, open_session, out, name, laps, mean_read_length, il) ? Decoded::Streamed : Decoded::Declined;
}

// obtain the texts, decide the kind once, index, push
bool sketch_fastq_on_device(Engine& e, const std::function<sylph_sketch*()>& open_session, const SampleFiles& sample, Container decode,
                            double& mean_read_length, const IndexedInput* text = nullptr) {
    if (!device_feed_enabled()) return false;
    const std::string* f2 = sample.second ? &*sample.second : nullptr;
    const bool decoded = !text && (decode == Container::Gzip || decode == Container::Bzip2);
    const Interleave il{sample.interleaved, sample.mate_check};
    std::vector<std::string> files{sample.first};
    if (f2) files.push_back(*f2);
    RouteTexts t;
    std::vector<uint8_t>& heads = t.heads;           // of host text and of plain files here, of decoded text once it is there
    std::vector<TextUploader::Mem> mem;
    if (text) {
        mem.push_back({text->a->data, text->a->size});
        if (f2) mem.push_back({text->b->data, text->b->size});
        for (const auto& m : mem) heads.push_back(m.p && m.bytes ? m.p[0] : 0);
    } else if (!decoded) for (const auto& f : files) heads.push_back(first_byte_of(f));
    // a gzip or bzip2 sample waits for the engine: nothing on the host side is faster than that — and so does plain FASTA, whose host
    // road is the sequential reader
    const bool plain_fasta = !text && !decoded && heads[0] == '>' && fasta_reads_on_device();
    if (!decoded && !plain_fasta && !e.ready()) return false;
    const bool trace = FeedLaps::on();
    FeedLaps laps;
    sylph_ctx* ctx = e.context();
    // The first text an engine sends pays for the route's device buffers (~40-90 ms of allocations, once); skipping the host's index
    // and gather of an inflated copy buys that back only for a sample of some size: 0.45 against 0.53 s for a 1 Gbp gzip pair, 0.34
    // against 0.30 s for its first mate alone (profiles/r05_feed_device_route.txt)
    if (text && !e.text.warm() && text->a->size + (f2 ? text->b->size : 0) < (1500ull << 20)) return false;
    if (decoded) {
        const Decoded got = decode_on_device(e, decode == Container::Gzip ? GZIP_STREAM : BZIP2_STREAM, open_session, files, laps, t, mean_read_length, il);
        if (got != Decoded::OnDevice) return got == Decoded::Streamed;
    }
    // a bzip2 sample whose text is there in one piece and then has no room — or is too large — to be indexed or pushed in one piece: the
    // stream takes it from its start (its windows are smaller), unless it is off
    const bool stream_after_all = decoded && decode == Container::Bzip2 && stream_mode(BZIP2_STREAM) == StreamMode::Auto;
    // FASTA reads that stay on the host reader, mates of different kinds: declined — for host text and plain files, before anything travels
    auto declined = [&](const char* why) {
        if (trace) fprintf(stderr, "[sylph_hip feed] device route declined %s: %s\n", files[0].c_str(), why);
        return false;
    };
    if (!same_kind(heads)) return declined("one mate is FASTA, the other is not");
    const bool fasta = heads[0] == '>';
    if (fasta && !fasta_reads_on_device()) return declined("FASTA reads stay on the host reader");
    if (!decoded) {
        if (!(text ? e.text.send(ctx, mem, parse_threads(), t.texts) : e.text.send(ctx, files, parse_threads(), t.texts))) return false;
        laps.lap("device route: text uploaded");
    }
    ReadIndex fa, fb;
    fa.fasta = fb.fasta = fasta;
    bool to_stream = false;
    auto streamed_instead = [&](const char* what) {
        if (trace) fprintf(stderr, "[sylph_hip feed] device route: %s of %s in one piece (%s): the stream takes it\n", what, files[0].c_str(), sylph_last_error());
        fa.reset();                                  // (the indexes borrow the text: they go first)
        fb.reset();
        t.texts.clear();
        sylph_inflated_destroy(t.owner.h);
        t.owner.h = nullptr;
        return stream_sample(e, BZIP2_STREAM, open_session, t, files[0].c_str(), laps, mean_read_length, il);
    };
    auto index = [&](const TextUploader::Text& x, ReadIndex& out) {
        // (an interleaved text: the index that also knows where its records start — a warning names two of them by their ids)
        uint64_t consumed = 0;
        const int rc = il.on ? out.index_window(ctx, x.dev, x.bytes, 1, &consumed) : out.index(ctx, x.dev, x.bytes);
        if (rc == SYLPH_ERR_FORMAT || rc == SYLPH_ERR_NOMEM) {
            // no room for the index, or more text than one index holds
            to_stream = stream_after_all && (rc == SYLPH_ERR_NOMEM || strstr(sylph_last_error(), "per index") != nullptr);
            return fasta && !to_stream ? declined(sylph_last_error()) : false;   // not for this route / no room for it: the host feed
        }
        hip_check(rc, out.index_name());
        return true;
    };
    if (!index(t.texts[0], fa) || (f2 && !index(t.texts[1], fb))) return to_stream ? streamed_instead("no index") : false;
    uint64_t na = 0, nb = 0, bases_a = 0, bases_b = 0;
    fa.counts(na, bases_a);
    if (f2) fb.counts(nb, bases_b);
    // lock-step readers: sketch.rs:813-815; an interleaved text: its pairs, a last record without a mate is dropped the same way
    const uint64_t n = il.on ? ip::pairs_of(na) : f2 ? std::min(na, nb) : na;
    laps.lap(fasta ? "device route: FASTA records found" : "device route: records found");
    if (il.on && il.check) {
        const uint64_t bad = fa.first_bad_pair(0, n);
        laps.lap("device route: interleaved mates checked");
        if (bad < n) {
            const void* base = nullptr;
            if (decoded) hip_check(sylph_inflated_text(t.owner.h, &base, nullptr), "sylph_inflated_text");
            struct Fd { int fd = -1; ~Fd() { if (fd >= 0) close(fd); } } file;
            if (!decoded && !text) file.fd = open(sample.first.c_str(), O_RDONLY);
            skip_out_of_phase(sample.first, fa, bad, bad, t.texts[0].bytes, [&](uint64_t at, uint64_t len, uint8_t* dst) {
                if (text) { memcpy(dst, text->a->data + at, len); return true; }
                if (decoded) return sylph_inflated_read(t.owner.h, (uint64_t)(t.texts[0].dev - (const uint8_t*)base) + at, len, dst) == SYLPH_OK;
                return file.fd >= 0 && pread(file.fd, dst, len, (off_t)at) == (ssize_t)len;
            });
        }
    }
    ReadLengths la;
    la.fetch(fa, il.on ? ip::kept_record(na) : n);
    // the one sequential piece of the reference's record loop (f64, file order: sketch.rs:941-943, :825-826), on its own thread
    double mean = 0.;
    std::thread tm([&] { double counter = 0.; la.continue_mean(n, mean, counter, il.on ? ip::MEAN_STRIDE : 1); });
    ThreadJoiner jm{tm};
    const auto pushes = il.on ? cut_pushes_interleaved(la, n, bases_a) : cut_pushes(f2 ? &fb : nullptr, la, n, bases_a + bases_b);
    sylph_sketch* const sk = open_session();
    e.batch.flush(sk);
    // one push: the batch is the session's own buffer, valid until finish — the seeding verdict may wait for it (one host round trip less)
    if (pushes.size() == 1) hip_check(sylph_sketch_set_option(sk, "borrow_until_finish", "1"), "sylph_sketch_set_option");
    for (const auto& p : pushes) {
        const int rc = il.on ? ReadIndex::push_interleaved(sk, fa, p.first, p.second) : ReadIndex::push(sk, fa, f2 ? &fb : nullptr, p.first, p.second);
        if (rc == SYLPH_ERR_NOMEM) {
            // no room on the device for this route's batch (the whole sample in one piece, up to 2 Gbp): not an error — the host feed, which
            // works through a sample in 256 Mbp batches, takes the sample from its start; the caller opens a fresh session
            if (trace) fprintf(stderr, "[sylph_hip feed] device route: no room for the batch (%s): the host feed takes the sample\n", sylph_last_error());
            tm.join();
            return stream_after_all ? streamed_instead("no room for the push") : false;
        }
        hip_check(rc, il.on ? fa.push_interleaved_name() : fa.push_name());
    }
    laps.lap(il.on ? "device route: interleaved pairs pushed" : "device route: pushed");
    tm.join();
    mean_read_length = mean;
    return true;
}

// MemAvailable of /proc/meminfo in bytes (0 if unknown)
size_t mem_available() {
    std::ifstream f("/proc/meminfo");
    std::string key;
    unsigned long long kb = 0;
    while (f >> key) {
        if (key == "MemAvailable:") { f >> kb; return (size_t)kb * 1024; }
        f.ignore(1 << 20, '\n');
    }
    return 0;
}
// what ONE index may hold in anonymous memory when `concurrent` of them can be alive at the same time: half of what is available
void set_feed_budget(size_t concurrent) {
    if (const char* e = getenv("SYLPH_HIP_FEED_MEM_GB")) { set_index_memory_budget((size_t)(atof(e) * (1ull << 30))); return; }
    const size_t avail = mem_available();
    set_index_memory_budget(avail ? avail / 2 / std::max<size_t>(1, concurrent) : 0);
}

// The sequential reader: needletail's exact record and error semantics, for whatever the two parallel roads do not take.  Each
// loop opens the sample's session once its files are open, pushes the records, and returns the running mean of the read lengths —
// or nothing where the reference gives no sketch.
std::optional<double> read_single_sequentially(Engine& e, const std::function<sylph_sketch*()>& open_session, const std::string& read_file) {
    std::unique_ptr<ChunkStream> reader;
    try { reader.reset(new ChunkStream(read_file)); }
    catch (const Error&) { warn(read_file + " is not a valid fasta/fastq file; skipping."); return std::nullopt; }   // sketch.rs:911-914
    sylph_sketch* const sk = open_session();
    double mean_read_length = 0., counter = 0.;
    const uint8_t* seq = nullptr;
    uint32_t len = 0;
    for (;;) {
        const ChunkStream::Kind kind = reader->next(seq, len);
        if (kind == ChunkStream::ERR) { warn("File " + read_file + " is not a valid fasta/fastq file"); break; }   // :945
        if (kind == ChunkStream::END) break;
        e.batch.add(sk, seq, len, nullptr, 0, false);
        counter += 1.;                                                       // :941-943
        mean_read_length = mean_read_length + ((double)len - mean_read_length) / counter;
    }
    e.batch.flush(sk);
    return mean_read_length;
}
std::optional<double> read_pair_sequentially(Engine& e, const std::function<sylph_sketch*()>& open_session, const std::string& read_file1,
                                             const std::string& read_file2) {
    std::unique_ptr<ChunkStream> r1, r2;   // the two mate files are parsed/inflated concurrently by their reader threads
    try { r1.reset(new ChunkStream(read_file1)); r2.reset(new ChunkStream(read_file2)); }
    catch (const Error&) {
        throw Error{1, "Paired end reading failed for '" + read_file1 + "' and '" + read_file2 +
                           "'. Make sure the files are present or the sequences are valid."};   // sketch.rs:781-784
    }
    sylph_sketch* const sk = open_session();
    double mean_read_length = 0., counter = 0.;
    const uint8_t *s1 = nullptr, *s2 = nullptr;
    uint32_t l1 = 0, l2 = 0;
    for (;;) {
        const ChunkStream::Kind k1 = r1->next(s1, l1);
        if (k1 == ChunkStream::ERR) { e.batch.flush(sk); return std::nullopt; }   // :878-880
        const ChunkStream::Kind k2 = r2->next(s2, l2);
        if (k1 == ChunkStream::END) break;                                   // :881-883
        if (k2 != ChunkStream::REC) continue;                                // mate 2 missing/invalid: pair skipped
        e.batch.add(sk, s1, l1, s2, l2, true);
        counter += 1.;                                                       // :824-826 (mate-1 length only)
        mean_read_length = mean_read_length + ((double)l1 - mean_read_length) / counter;
    }
    e.batch.flush(sk);
    return mean_read_length;
}
// An interleaved file through the one reader: records 2 i and 2 i + 1 are a pair, their headers reach the mate check, a last record
// without a mate is dropped.  There is no second reader to go on with, so the two-file rules of sketch.rs:878-883 do not carry over:
// a malformed record anywhere, or a pair that fails the check, gives no sketch.
std::optional<double> read_interleaved_sequentially(Engine& e, const std::function<sylph_sketch*()>& open_session, const SampleFiles& files) {
    const std::string& read_file = files.first;
    std::unique_ptr<ChunkStream> reader;
    try { reader.reset(new ChunkStream(read_file, true)); }
    catch (const Error&) { warn(read_file + " is not a valid fasta/fastq file; skipping."); return std::nullopt; }
    if (FeedLaps::on()) fprintf(stderr, "[sylph_hip feed] sequential reader: interleaved %s\n", read_file.c_str());
    sylph_sketch* const sk = open_session();
    double mean_read_length = 0., counter = 0.;
    std::vector<uint8_t> m1, h1;
    const uint8_t *s = nullptr, *h = nullptr;
    uint32_t len = 0, hl = 0;
    for (uint64_t pair = 0;; pair++) {
        ChunkStream::Kind kind = reader->next(s, len);
        if (kind == ChunkStream::END) break;
        if (kind == ChunkStream::REC) {
            m1.assign(s, s + len);                                           // (valid until the next call only)
            reader->last_header(h, hl);
            h1.assign(h, h + hl);
            kind = reader->next(s, len);
            if (kind == ChunkStream::END) break;                             // a last record without a mate is dropped
        }
        if (kind == ChunkStream::ERR) {
            warn("File " + read_file + " is not a valid fasta/fastq file; an interleaved file with a malformed record gives no sketch; skipping.");
            e.batch.flush(sk);
            return std::nullopt;
        }
        reader->last_header(h, hl);
        if (files.mate_check && !ip::mates(h1.data(), ip::id_len(h1.data(), h1.size()), h, ip::id_len(h, hl))) {
            warn_out_of_phase(read_file, pair, id_of_header(h1.data(), h1.size()), id_of_header(h, hl));
            e.batch.flush(sk);
            return std::nullopt;
        }
        e.batch.add(sk, m1.data(), (uint32_t)m1.size(), s, len, true);
        counter += 1.;                                                       // :824-826 (mate-1 length only)
        mean_read_length = mean_read_length + ((double)m1.size() - mean_read_length) / counter;
    }
    e.batch.flush(sk);
    return mean_read_length;
}
}  // namespace

void IndexAhead::start(size_t j) {
    std::lock_guard<std::mutex> lk(mu_);
    if (j >= files_.size() || fut_.count(j)) return;
    const SampleFiles f = files_[j];
    fut_[j] = std::async(std::launch::async, [f] { return index_inputs(f); });
}
std::optional<IndexedInput> IndexAhead::get(size_t j) {
    std::future<std::optional<IndexedInput>> f;
    {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = fut_.find(j);
        if (it != fut_.end()) { f = std::move(it->second); fut_.erase(it); }
    }
    if (f.valid()) return f.get();
    return index_inputs(files_.at(j));
}

FeedShared::FeedShared(std::vector<SampleFiles> files, size_t workers) : ahead(std::move(files)), n_workers(workers) {
    set_parse_share((unsigned)n_workers);
    set_feed_budget(4 * n_workers);            // two files per sample, the current and the next sample of every worker
    set_no_more_inflates(false);
}

SampleRoute::SampleRoute(Engine& eng, FeedShared& feed, size_t j, bool first_use_hint) {
    const SampleFiles& files = feed.ahead.files(j);
    const bool feed_dev = device_feed_enabled();
    const Container c1 = feed_dev ? container_of(files.first) : Container::Plain;
    const bool compressed = c1 != Container::Plain;
    const bool decoded = device_decode_enabled(c1);           // the compressed bytes travel, the device inflates / decodes (mate 1 decides the road)
    // plain FASTA reads: the host road is the sequential reader, so the sample waits for the engine as a compressed one does
    const bool plain_fasta = feed_dev && !compressed && fasta_reads_on_device() && first_byte_of(files.first) == '>';
    dev = feed_dev && (decoded || plain_fasta || (eng.ready() && !compressed));
    // ... the device's decoder is the one to use if mate 2 is of the same container; if not, the device route declines the pair
    if (decoded && (!files.second || container_of(*files.second) == c1)) decode = c1;
    if (c1 == Container::Gzip && !decoded) pre = index_inputs(files, false);   // inflated on the host, its text then sent as it is
    else if (!dev) pre = feed.ahead.get(j);
    if (first_use_hint) {
        if ((decoded || plain_fasta) && !eng.ready()) { eng.defer_pinned.store(true); eng.warm_text_route.store(true); }
        trace_mark(dev ? "sketch: the sample goes the device route" : "sketch: the sample's files are indexed (or not indexable)");
    }
    if (++feed.indexes_obtained == feed.ahead.size()) set_no_more_inflates(true);
    if (!feed_dev) feed.ahead.start(j + feed.n_workers);
}
SampleRoute::~SampleRoute() {
    if (pre) background([x = std::make_shared<std::optional<IndexedInput>>(std::move(pre))]() mutable { x.reset(); });
}

namespace {
std::optional<SequencesSketch> sketch_by_route(Engine& e, const SampleFiles& files, const SampleParams& p, SampleRoute& route, sylph_sketch** keep) {
    const bool paired = files.paired();
    std::optional<Session> so;
    const std::function<sylph_sketch*()> open_session = [&] { so.emplace(e, p.c, p.k, paired, p.no_dedup, p.dedup_fpr); return so->sk; };
    auto sketched = [&](double mean_read_length) {
        SequencesSketch out;
        so->finish_or_keep(out, keep);
        out.file_name = files.first; out.c = p.c; out.k = p.k; out.paired = paired;
        out.sample_name = p.sample_name;
        out.mean_read_length = mean_read_length;
        return out;
    };
    double mean = 0.;
    // `index`: the files' index if the route obtained it (an empty optional: the files are not for the block-parallel feed);
    // nullptr: nobody has tried yet — the sample was meant for the device
    std::optional<IndexedInput>* index = route.dev ? nullptr : &route.pre;
    const bool text_only = index && *index && !(*index)->a->ok;
    if (route.dev || text_only) {
        if (sketch_fastq_on_device(e, open_session, files, route.decode, mean, text_only ? &**index : nullptr)) return sketched(mean);
        // declined: the host feed takes the sample from its start, with a fresh session
        if (text_only && !finish_index(**index)) index->reset();
        so.reset();
    }
    std::optional<IndexedInput> own;
    if (!index) { own = index_inputs(files); index = &own; }
    if (*index) {   // uncompressed 4-line FASTQ: block-parallel feed
        sketch_indexed(e, open_session, **index, mean, files);
        return sketched(mean);
    }
    const std::optional<double> seq_mean = files.interleaved ? read_interleaved_sequentially(e, open_session, files)
                                           : paired          ? read_pair_sequentially(e, open_session, files.first, *files.second)
                                                             : read_single_sequentially(e, open_session, files.first);
    if (!seq_mean) return std::nullopt;
    return sketched(*seq_mean);
}
}  // namespace

std::optional<SequencesSketch> sketch_sample(Engine& e, const SampleFiles& files, const SampleParams& p, SampleRoute& route, sylph_sketch** keep) {
    try { return sketch_by_route(e, files, p, route, keep); }
    catch (const SampleSkipped&) { return std::nullopt; }   // an interleaved sample out of phase: warned about, its session dropped on the way here
}

}  // namespace sylph_host
