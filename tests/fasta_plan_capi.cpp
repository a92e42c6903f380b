// C wrapper around sylph_amd/csrc/fasta_plan.h for tests/test_fasta_plan.py (g++, no HIP): a SEQUENTIAL model of the FASTA index and
// join of csrc/fasta.hip.  Every step walks the tiles and lanes the kernels walk and calls the very per-lane, per-line and per-tile
// functions of fasta_plan.h the kernels call; what the kernels do with workgroup scans and atomics is a running sum here.  Test
// infrastructure: the product never runs this.
#include "../sylph_amd/csrc/fasta_plan.h"

#include <cstring>
#include <vector>

using namespace sylph::fasta_plan;

namespace {

struct Model {
    std::vector<uint8_t> stream;          // the aligned stream: `bias` bytes of junk, the text, junk up to a whole lane and one more
    uint32_t bias = 0;
    uint64_t n = 0, n_tiles = 0, n_lines = 0, n_rec = 0, n_bases = 0, id_bytes = 0;
    std::vector<uint32_t> tile_base;
    std::vector<uint64_t> line_start, scan, rec_off, id_pos;
    std::vector<uint32_t> id_len;
    const uint8_t* text() const { return stream.data() + bias; }
};

// fa_lane_load: the lane's four dwords and the mask of its bytes inside the text
uint32_t lane_load(const Model& m, uint64_t tile, uint32_t lane, uint32_t w[4], int64_t& i0) {
    const uint64_t p = tile * TILE_BYTES + (uint64_t)lane * LANE_BYTES;
    i0 = (int64_t)p - (int64_t)m.bias;
    const uint32_t valid = lane_valid(i0, m.n);
    w[0] = w[1] = w[2] = w[3] = 0;
    if (valid) memcpy(w, m.stream.data() + p, LANE_BYTES);
    return valid;
}

}  // namespace

extern "C" {

uint64_t fa_max_text_bytes() { return MAX_TEXT_BYTES; }
int fa_size_refused(uint64_t n_bytes, uint64_t n_newlines) { return !text_size_ok(n_bytes) || !line_count_ok(n_newlines); }

// 0 and a model in *out, or -5 (SYLPH_ERR_FORMAT) and nothing.  The text is copied to byte `bias` (0..15) of a 16-byte aligned stream whose
// other bytes are junk that looks like structure ('\n', '\r', '>').
int fa_index(const uint8_t* text, uint64_t n, uint32_t bias, void** out) {
    *out = nullptr;
    if (!text_size_ok(n) || bias >= LANE_BYTES) return -5;
    Model* m = new Model;
    m->bias = bias;
    m->n = n;
    m->n_tiles = (n + bias + TILE_BYTES - 1) / TILE_BYTES;
    m->stream.resize(m->n_tiles * TILE_BYTES + LANE_BYTES);
    for (size_t i = 0; i < m->stream.size(); i++) m->stream[i] = (uint8_t)"\n\r>"[i % 3];
    memcpy(m->stream.data() + bias, text, n);
    bool bad = m->text()[0] != '>';                                                    // fa_init_kernel
    // fa_count_kernel
    std::vector<uint32_t> tile_cnt(m->n_tiles + 1, 0);
    uint64_t n_nl = 0;
    for (uint64_t t = 0; t < m->n_tiles; t++)
        for (uint32_t l = 0; l < TILE_LANES; l++) {
            uint32_t w[4];
            int64_t i0;
            const uint32_t valid = lane_load(*m, t, l, w, i0);
            const uint32_t nl = lane_mask(w, '\n') & valid, cr = lane_mask(w, '\r') & valid;
            if (cr) {
                const int64_t nx = i0 + (int64_t)LANE_BYTES;
                const bool next_ok = nx >= (int64_t)n || m->stream[(uint64_t)(nx + bias)] == '\n';
                if (lane_stray_cr(cr, nl, valid, next_ok)) bad = true;
            }
            tile_cnt[t] += (uint32_t)__builtin_popcount(nl);
            n_nl += (uint32_t)__builtin_popcount(nl);
        }
    if (bad || !line_count_ok(n_nl)) { delete m; return -5; }
    m->tile_base.assign(m->n_tiles + 1, 0);
    for (uint64_t t = 0; t < m->n_tiles; t++) m->tile_base[t + 1] = m->tile_base[t] + tile_cnt[t];
    m->n_lines = n_nl + 1;
    // fq_lines_kernel: the byte behind every newline starts a line; one entry past a virtual final newline
    m->line_start.assign(m->n_lines + 1, 0);
    m->line_start[m->n_lines] = n + 1;
    for (uint64_t t = 0; t < m->n_tiles; t++) {
        uint64_t ord = m->tile_base[t];
        for (uint32_t l = 0; l < TILE_LANES; l++) {
            uint32_t w[4];
            int64_t i0;
            const uint32_t valid = lane_load(*m, t, l, w, i0);
            const uint32_t nl = lane_mask(w, '\n') & valid;
            for (uint32_t b = 0; b < LANE_BYTES; b++)
                if (nl >> b & 1u) { ord++; if (ord < m->n_lines) m->line_start[ord] = (uint64_t)(i0 + b) + 1; }
        }
    }
    // fa_values_kernel + the exclusive scan
    m->scan.assign(m->n_lines + 1, 0);
    const uint8_t* tx = m->text();
    for (uint64_t L = 0; L < m->n_lines; L++) {
        const uint64_t s = m->line_start[L], raw = m->line_start[L + 1] - 1 - s;
        m->scan[L + 1] = m->scan[L] + (raw ? line_value(raw, tx[s], tx[s + raw - 1]) : 0ull);
    }
    m->n_rec = scan_headers(m->scan[m->n_lines]);
    m->n_bases = scan_bases(m->scan[m->n_lines]);
    // fa_records_kernel
    m->rec_off.assign(m->n_rec + 1, ~0ull);
    m->id_pos.assign(m->n_rec, ~0ull);
    m->id_len.assign(m->n_rec, ~0u);
    for (uint64_t L = 0; L < m->n_lines; L++) {
        const uint64_t sl = m->scan[L], sn = m->scan[L + 1];
        if (!scan_line_is_header(sl, sn)) continue;
        const uint64_t r = scan_headers(sl), s = m->line_start[L], raw = m->line_start[L + 1] - 1 - s;
        const uint64_t idl = line_len(raw, tx[s + raw - 1]) - 1;
        if (r < m->n_rec) { m->rec_off[r] = scan_bases(sl); m->id_pos[r] = s + 1; m->id_len[r] = (uint32_t)idl; }
        m->id_bytes += idl;
    }
    m->rec_off[m->n_rec] = m->n_bases;
    *out = m;
    return 0;
}

void fa_counts(const void* h, uint64_t* n_rec, uint64_t* n_bases, uint64_t* id_bytes, uint64_t* n_lines) {
    const Model* m = (const Model*)h;
    *n_rec = m->n_rec; *n_bases = m->n_bases; *id_bytes = m->id_bytes; *n_lines = m->n_lines;
}
void fa_records(const void* h, uint64_t* rec_off /* n_rec + 1 */, uint64_t* id_pos, uint32_t* id_len) {
    const Model* m = (const Model*)h;
    memcpy(rec_off, m->rec_off.data(), (m->n_rec + 1) * 8);
    memcpy(id_pos, m->id_pos.data(), m->n_rec * 8);
    memcpy(id_len, m->id_len.data(), m->n_rec * 4);
}

// fa_join_kernel, tile by tile, into mem[0, mem_bytes): base 0 of the text goes to mem + out_pos (mem is taken as 16-byte aligned, as the
// device's allocations are, so out_pos decides the alignment of every store).  Returns the kernel's error word; *wide / *narrow count the
// 16-byte and the single-byte stores.  A store outside [out_pos, out_pos + n_bases) is counted in *outside and not made.
uint32_t fa_join(const void* h, uint8_t* mem, uint64_t mem_bytes, uint64_t out_pos, uint64_t* wide, uint64_t* narrow, uint64_t* outside) {
    const Model* m = (const Model*)h;
    uint32_t err = 0;
    *wide = *narrow = *outside = 0;
    std::vector<uint8_t> lds((TILE_LANES + 2) * LANE_BYTES);
    for (uint64_t t = 0; t < m->n_tiles; t++) {
        uint64_t L = m->tile_base[t];
        uint32_t d0 = 0, off = 0, kept = 0;
        std::vector<uint32_t> keeps(TILE_LANES), offs(TILE_LANES), dests(TILE_LANES), valids(TILE_LANES);
        std::vector<uint32_t> words(TILE_LANES * 4);
        for (uint32_t l = 0; l < TILE_LANES; l++) {
            uint32_t* w = &words[l * 4];
            int64_t i0;
            const uint32_t valid = lane_load(*m, t, l, w, i0);
            const uint32_t nl = lane_mask(w, '\n') & valid, cr = lane_mask(w, '\r') & valid, gt = lane_mask(w, '>') & valid;
            uint32_t keep = 0, dest = 0;
            if (valid) {
                const uint64_t sl = m->scan[L], sn = m->scan[L + 1];
                dest = dest_at((uint64_t)(i0 < 0 ? 0 : i0), m->line_start[L], sl, sn);
                keep = lane_keep(nl, cr, gt, valid, scan_line_is_header(sl, sn));
            }
            if (l == 0) d0 = dest;
            keeps[l] = keep; offs[l] = off; dests[l] = dest; valids[l] = valid;
            off += (uint32_t)__builtin_popcount(keep);
            L += (uint32_t)__builtin_popcount(nl);
        }
        kept = off;
        for (uint32_t l = 0; l < TILE_LANES; l++)
            if (valids[l] && dests[l] != d0 + offs[l]) err |= 1u;
        if ((uint64_t)d0 + kept > m->n_bases) { err |= 2u; continue; }
        const uint64_t first = out_pos + d0;
        const uint32_t shift = (uint32_t)(first & 15);
        for (uint32_t l = 0; l < TILE_LANES; l++) {
            uint32_t o = shift + offs[l];
            for (uint32_t b = 0; b < LANE_BYTES; b++)
                if (keeps[l] >> b & 1u) lds[o++] = (uint8_t)(words[l * 4 + (b >> 2)] >> (8 * (b & 3)));
        }
        const uint64_t base = first - shift;
        const uint32_t chunks = store_chunks(shift, kept);
        for (uint32_t j = 0; j < chunks; j++) {
            uint32_t lo, hi;
            store_chunk_range(j, shift, kept, lo, hi);
            const uint64_t a = base + (uint64_t)j * LANE_BYTES;
            if (a + lo < out_pos || a + hi > out_pos + m->n_bases || a + hi > mem_bytes) { (*outside)++; continue; }
            if (lo == 0 && hi == LANE_BYTES) { (*wide)++; memcpy(mem + a, &lds[j * LANE_BYTES], LANE_BYTES); }
            else for (uint32_t x = lo; x < hi; x++) { (*narrow)++; mem[a + x] = lds[j * LANE_BYTES + x]; }
        }
    }
    return err;
}

void fa_free(void* h) { delete (Model*)h; }

}  // extern "C"
