// C entry points over sylph_amd/csrc/fasta_reads_plan.h for tests/test_fasta_reads_plan.py and tests/fasta_reads_sanitize_main.cpp: a
// sequential model of fa_batch_kernel (every tile, every lane, the plan's walk, cut and lay — the aligned 16-byte loads and the one
// 16-byte store per lane included) and of the window rule of sylph_fasta_index_window.  Built with g++, no HIP.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../sylph_amd/csrc/fasta_reads_plan.h"

namespace rp = sylph::fasta_reads_plan;

namespace {
// the batch's 32-bit offsets, as batch_lens_kernel (csrc/read_text.h) + the exclusive scan make them; false: 2^32 - 64 bases or more
bool batch_offsets(const uint64_t* ro_a, const uint64_t* ro_b, uint64_t first, uint64_t n_items, std::vector<uint32_t>& off) {
    const uint64_t n_rec = rp::batch_records(n_items, ro_b != nullptr);
    off.assign(n_rec + 1, 0);
    uint64_t sum = 0;
    for (uint64_t j = 0; j < n_rec; j++) {
        off[j] = (uint32_t)sum;
        sum += rp::batch_len(ro_a, ro_b, first, j);
    }
    off[n_rec] = (uint32_t)sum;
    return sum < (1ull << 32) - 64;
}
struct Aligned {                     // a copy of n bytes at a 16-byte aligned address, 64 readable bytes of 0xEE behind it
    uint8_t* p;
    Aligned(const uint8_t* src, uint64_t n) : p((uint8_t*)aligned_alloc(16, (n + 64 + 15) / 16 * 16)) {
        memset(p, 0xEE, (n + 64 + 15) / 16 * 16);
        if (n) memcpy(p, src, n);
    }
    ~Aligned() { free(p); }
};
}  // namespace

extern "C" {

uint32_t fr_tile_bytes() { return rp::TILE_BYTES; }

// bases of the batch, or ~0 when it is too large for 32-bit offsets
uint64_t fr_batch_total(const uint64_t* ro_a, const uint64_t* ro_b, uint64_t first, uint64_t n_items) {
    std::vector<uint32_t> off;
    if (!batch_offsets(ro_a, ro_b, first, n_items, off)) return ~0ull;
    return off.back();
}

// For every output byte of the batch: the mate (0 / 1), the record in that file and the index in that file's joined bases, as the lanes
// of every tile find them.  *max_pieces: the most pieces one lane walked over.  Returns the number of bytes no lane (or more than one)
// claimed — 0 for a correct plan.
uint64_t fr_batch_map(const uint64_t* ro_a, const uint64_t* ro_b, uint64_t first, uint64_t n_items, uint8_t* mate, uint64_t* rec, uint64_t* src,
                      uint32_t* max_pieces) {
    std::vector<uint32_t> off;
    if (!batch_offsets(ro_a, ro_b, first, n_items, off)) return ~0ull;
    const uint64_t n_rec = off.size() - 1, total = off.back();
    const bool paired = ro_b != nullptr;
    std::vector<uint8_t> seen(total, 0);
    uint32_t most = 0;
    const uint64_t tiles = (total + rp::TILE_BYTES - 1) / rp::TILE_BYTES;
    for (uint64_t t = 0; t < tiles; t++)
        for (uint32_t lane = 0; lane < rp::TILE_LANES; lane++) {
            const uint64_t o = t * rp::TILE_BYTES + (uint64_t)lane * rp::LANE_BYTES;
            uint32_t pieces = 0;
            rp::lane_walk(off.data(), n_rec, total, o, [&](uint64_t j, uint64_t p, uint32_t b0, uint32_t len) {
                pieces++;
                for (uint32_t x = 0; x < len; x++) {
                    const uint64_t q = p + x;
                    if (q >= total || q != o + b0 + x) continue;       // (stays unseen: counted below)
                    seen[q]++;
                    mate[q] = (uint8_t)rp::mate_of(j, paired);
                    rec[q] = rp::record_of(j, paired, first);
                    src[q] = rp::source_of(off.data(), ro_a, ro_b, first, j, q);
                }
            });
            if (pieces > most) most = pieces;
        }
    *max_pieces = most;
    uint64_t bad = 0;
    for (uint64_t q = 0; q < total; q++) bad += seen[q] != 1;
    return bad;
}

// The gather itself: out[0, total rounded up to 16) written with one 16-byte store per lane from aligned 16-byte loads of the joined
// bases (n_a / n_b bytes).  out must be 16-byte aligned with room for `cap` bytes.  Returns 0, or 1 when a store would leave [0, cap).
int fr_batch_gather(const uint8_t* ja, uint64_t n_a, const uint64_t* ro_a, const uint8_t* jb, uint64_t n_b, const uint64_t* ro_b, uint64_t first,
                    uint64_t n_items, uint8_t* out, uint64_t cap) {
    std::vector<uint32_t> off;
    if (!batch_offsets(ro_a, ro_b, first, n_items, off)) return 2;
    const uint64_t n_rec = off.size() - 1, total = off.back();
    const Aligned a(ja, n_a), b(ro_b ? jb : nullptr, ro_b ? n_b : 0);
    const uint64_t tiles = (total + rp::TILE_BYTES - 1) / rp::TILE_BYTES;
    for (uint64_t t = 0; t < tiles; t++)
        for (uint32_t lane = 0; lane < rp::TILE_LANES; lane++) {
            const uint64_t o = t * rp::TILE_BYTES + (uint64_t)lane * rp::LANE_BYTES;
            if (o >= total) continue;
            uint64_t out_lo = 0, out_hi = 0;
            rp::lane_walk(off.data(), n_rec, total, o, [&](uint64_t j, uint64_t p, uint32_t b0, uint32_t len) {
                const uint8_t* s = (rp::mate_of(j, ro_b != nullptr) ? b.p : a.p) + rp::source_of(off.data(), ro_a, ro_b, first, j, p);
                const uint32_t sh = (uint32_t)((uintptr_t)s & 15);
                uint64_t q[4], lo, hi;
                memcpy(q, s - sh, 32);
                rp::cut16(q[0], q[1], q[2], q[3], sh, lo, hi);
                rp::lay16(lo, hi, b0, len, out_lo, out_hi);
            });
            if (o + 16 > cap) return 1;
            memcpy(out + o, &out_lo, 8);
            memcpy(out + o + 8, &out_hi, 8);
        }
    return 0;
}

// The window rule over a text read byte by byte.  Returns 0 and the records / consumed of the window, or -5 (SYLPH_ERR_FORMAT) for what
// sylph_fasta_index refuses: no text (final only), a first byte other than '>', a '\r' not directly in front of '\n' or of the end.
int fr_window(const uint8_t* text, uint64_t n, int final, uint64_t* records, uint64_t* consumed) {
    *records = *consumed = 0;
    if (!n) return final ? -5 : 0;
    if (text[0] != '>') return -5;
    uint64_t headers = 0, last_at = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (text[i] == '\r' && i + 1 < n && text[i + 1] != '\n') return -5;
        if (text[i] == '>' && (i == 0 || text[i - 1] == '\n')) { headers++; last_at = i; }
    }
    *records = rp::window_records(headers, final != 0);
    *consumed = rp::window_consumed(headers, final != 0, n, last_at);
    return 0;
}

}  // extern "C"
