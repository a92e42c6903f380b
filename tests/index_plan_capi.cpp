// C wrapper around sylph_amd/csrc/index_plan.h for tests/test_index_plan.py and tests/index_sanitize_main.cpp (g++, no HIP): the very
// header the index build and the probe include — geometry, pass split, bucket division, slot codec, hit key rules — and a model of the
// line index in host memory, built pass by pass with the plan's bucket writer and looked up with the plan's slot scan.  Compiled with
// -DSYLPH_LINE_SLOTS=4 it is the model of the 32-byte line.  Test infrastructure: the product never runs this.
#include <cstddef>
#include <vector>

#include "../sylph_amd/csrc/index_plan.h"

using namespace sylph::index_plan;
using std::size_t;

namespace {
struct Model {
    Geometry geo;
    uint64_t base = 0, n_ovf = 0;
    uint32_t n_pass = 0;
    std::vector<uint64_t> lines, ovf;
};
}  // namespace

extern "C" {

void ip_constants(uint64_t* out4) { out4[0] = LINE_SLOTS; out4[1] = LONG_RUN_MIN; out4[2] = DEFAULT_INDEX_LAMBDA; out4[3] = SLOT_EMPTY; }
uint64_t ip_magic(uint64_t div) { return magic_of(div); }
void ip_bucket_rem(const uint64_t* x, const uint64_t* div, uint64_t n, uint64_t* q, uint64_t* rem) {
    for (uint64_t i = 0; i < n; i++) bucket_rem(x[i], div[i], magic_of(div[i]), q[i], rem[i]);
}
void ip_geometry(uint64_t n_genomes, uint64_t kmer_lo, uint64_t max_key, uint64_t postings, uint64_t lambda, uint64_t* out7) {
    const Geometry g = geometry(n_genomes, kmer_lo, max_key, postings, lambda);
    out7[0] = (uint64_t)g.why; out7[1] = (uint64_t)g.gb; out7[2] = (uint64_t)g.gshift; out7[3] = g.div_cap; out7[4] = g.div; out7[5] = g.magic; out7[6] = g.n_buckets;
}
int ip_overflow_fits(uint64_t n_ovf, int gb) { return overflow_fits(n_ovf, gb) ? 1 : 0; }
uint32_t ip_n_passes(uint64_t n_buckets, uint64_t postings, uint64_t pass_max) { return n_passes(n_buckets, postings, pass_max); }
void ip_pass_of(uint32_t p, uint32_t n_pass, uint64_t n_buckets, uint64_t kmer_lo, uint64_t kmer_hi, uint64_t div, uint64_t* out4) {
    const Pass r = pass_of(p, n_pass, n_buckets, kmer_lo, kmer_hi, div);
    out4[0] = r.b0; out4[1] = r.b1; out4[2] = r.klo; out4[3] = r.khi;
}
uint64_t ip_encode_posting(uint64_t rem, uint32_t genome, int gshift) { return encode_posting(rem, genome, gshift); }
uint64_t ip_encode_descriptor(uint64_t start, uint64_t len, int gshift) { return encode_descriptor(start, len, gshift); }
// {remainder, is a descriptor, genome, run start, run length}
void ip_decode(uint64_t s, int gshift, uint64_t* out5) {
    out5[0] = slot_rem(s, gshift); out5[1] = slot_is_descriptor(s, gshift) ? 1 : 0; out5[2] = slot_genome(s, gshift);
    out5[3] = slot_run_start(s, gshift); out5[4] = slot_run_len(s, gshift);
}
void ip_layout(uint32_t c, uint32_t* out2) { out2[0] = postings_in_line(c); out2[1] = overflow_need(c); }
uint64_t ip_hit_key(uint64_t row, uint32_t count) { return hit_key(row, count); }
void ip_compact_key(uint32_t max_count, uint64_t n_rows, int* out3) {
    const CompactKey k = compact_key(max_count, n_rows);
    out3[0] = k.cb; out3[1] = k.rb; out3[2] = k.fits ? 1 : 0;
}
uint32_t ip_coverage_width(int want_narrow, uint32_t max_count) { return coverage_width(want_narrow != 0, max_count); }

// The index over n postings sorted by (k-mer, genome id), all inside [kmer_lo, kmer_hi) (kmer_hi = 0: open), the way the device build
// goes about it: geometry, then per pass the postings of [klo, khi), their buckets by bucket_rem, the overflow offsets by
// overflow_need, one write_bucket per bucket.  nullptr: refused by the geometry, or a posting fell outside its pass's buckets.
void* ip_model_build(const uint64_t* keys, const uint32_t* gids, uint64_t n, uint64_t n_genomes, uint64_t kmer_lo, uint64_t kmer_hi,
                     uint64_t lambda, uint64_t pass_max) {
    if (!n) return nullptr;
    Model* m = new Model;
    m->base = kmer_lo;
    m->geo = geometry(n_genomes, kmer_lo, keys[n - 1], n, lambda);
    if (m->geo.why != BUILDABLE) { delete m; return nullptr; }
    m->lines.assign((size_t)m->geo.n_buckets * LINE_SLOTS, 0);
    m->n_pass = n_passes(m->geo.n_buckets, n, pass_max);
    uint64_t at = 0;
    for (uint32_t p = 0; p < m->n_pass; p++) {
        const Pass ps = pass_of(p, m->n_pass, m->geo.n_buckets, kmer_lo, kmer_hi, m->geo.div);
        uint64_t end = at;
        while (end < n && keys[end] >= ps.klo && (ps.khi == 0 || keys[end] < ps.khi)) end++;
        std::vector<uint64_t> first((size_t)(ps.b1 - ps.b0) + 1, end);         // first posting of every bucket of the pass
        for (uint64_t i = end; i-- > at;) {
            uint64_t q, rem;
            bucket_rem(keys[i] - kmer_lo, m->geo.div, m->geo.magic, q, rem);
            if (q < ps.b0 || q >= ps.b1 || rem >= m->geo.div) { delete m; return nullptr; }
            first[q - ps.b0] = i;
        }
        for (size_t b = first.size() - 1; b-- > 0;) if (first[b] > first[b + 1]) first[b] = first[b + 1];   // empty buckets
        uint64_t need = 0;
        for (size_t b = 0; b + 1 < first.size(); b++) need += overflow_need((uint32_t)(first[b + 1] - first[b]));
        m->ovf.resize(m->n_ovf + need + 1, 0);
        uint64_t run_start = m->n_ovf;
        for (size_t b = 0; b + 1 < first.size(); b++) {
            const uint32_t c = (uint32_t)(first[b + 1] - first[b]);
            uint64_t s[LINE_SLOTS];
            write_bucket(keys + first[b], gids + first[b], c, kmer_lo + (ps.b0 + b) * m->geo.div, m->geo.gshift, run_start, s, m->ovf.data());
            for (int j = 0; j < LINE_SLOTS; j++) m->lines[(size_t)(ps.b0 + b) * LINE_SLOTS + j] = s[j];
            run_start += overflow_need(c);
        }
        m->n_ovf = run_start;
        at = end;
    }
    if (at != n || !overflow_fits(m->n_ovf, m->geo.gb)) { delete m; return nullptr; }
    return m;
}
void ip_model_free(void* mp) { delete (Model*)mp; }
// {buckets, overflow entries, passes, div, gshift}
void ip_model_info(const void* mp, uint64_t* out5) {
    const Model* m = (const Model*)mp;
    out5[0] = m->geo.n_buckets; out5[1] = m->n_ovf; out5[2] = m->n_pass; out5[3] = m->geo.div; out5[4] = (uint64_t)m->geo.gshift;
}
const uint64_t* ip_model_lines(const void* mp) { return ((const Model*)mp)->lines.data(); }
const uint64_t* ip_model_ovf(const void* mp) { return ((const Model*)mp)->ovf.data(); }
// The genomes of k-mer km, in the order the probe meets them: bucket_rem, scan_slots over the bucket's line and — a long run handed
// back (*long_run = 1) — the run's entries one by one as the wavefront's step reads them (run_stops, bounded by the overflow size).
// Returns how many there are; the first `cap` are stored.
uint64_t ip_model_lookup(const void* mp, uint64_t km, uint32_t* out, uint64_t cap, int* long_run) {
    const Model* m = (const Model*)mp;
    *long_run = 0;
    if (km < m->base) return 0;
    uint64_t q, rem;
    bucket_rem(km - m->base, m->geo.div, m->geo.magic, q, rem);
    if (q >= m->geo.n_buckets) return 0;
    uint64_t s[LINE_SLOTS];
    for (int j = 0; j < LINE_SLOTS; j++) s[j] = m->lines[(size_t)q * LINE_SLOTS + j];
    uint64_t n = 0, long_start = NO_LONG_RUN, long_rem = 0;
    auto take = [&](uint32_t g) { if (n < cap) out[n] = g; n++; };
    scan_slots(s, rem, m->geo.gshift, m->ovf.data(), take, &long_start, &long_rem);
    if (long_start != NO_LONG_RUN) {
        *long_run = 1;
        for (uint64_t i = long_start;; i++) {
            const uint64_t y = i < m->n_ovf ? m->ovf[i] : SLOT_EMPTY;
            if (run_stops(y, long_rem, m->geo.gshift)) break;
            if (slot_rem(y, m->geo.gshift) == long_rem) take(slot_genome(y, m->geo.gshift));
        }
    }
    return n;
}

}  // extern "C"
