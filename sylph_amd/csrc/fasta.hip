// fasta.hip — the records of FASTA text, found and joined on the device: the sibling of fastq.hip for genome files.
//
// The reference reads a genome file record by record with needletail (sketch.rs:488-492, :557-563) and appends every record's sequence
// to the genome; the host of this repository does the same with FastxReader (host/formats.cpp), whose record semantics are the ones
// implemented here: a line that begins with '>' is a header, a record's sequence is every following non-header line joined without
// its line end ('\n', or '\r' '\n', or a '\r' at the very end of the text), an empty line contributes nothing, a header directly
// followed by a header or by the end is a record of length 0.
//
//   fa_init_kernel      the first byte must be '>'
//   fa_count_kernel     newlines per 4 KiB tile; any '\r' that is not directly followed by '\n' or by the end of the text is flagged
//   exclusive scan      first line number of every tile
//   fq_lines_kernel     start of every line (text_lines.h, shared with fastq.hip)
//   fa_values_kernel    per line: a header adds 2^32, a sequence line adds its length without the '\r' (fasta_plan.h line_value)
//   exclusive scan      ONE 64-bit scan over the lines: headers in front of a line (its record number + 1) in the high word, sequence
//                       bytes in front of it (its destination in the joined sequence) in the low word
//   fa_records_kernel   per header line: the record's first base, where its id lies in the text and how long it is
//   fa_join_kernel      per 4 KiB tile of text: the sequence bytes compacted in LDS and written with aligned 16-byte stores to their
//                       place in a batch.  The kept bytes of a tile are contiguous in the output; the tile's first destination comes
//                       from the line table.  No lane looks at more than its 16 bytes: a text of 1-byte lines and a chromosome on one
//                       line run through the same code at the same cost per byte.
//
// The same text as a SAMPLE's reads (sylph_sketch_push_fasta; fasta_reads_plan.h):
//
//   fa_join_kernel      once per index, into a buffer of the index: the file's bases side by side
//   batch_lens_kernel, exclusive scan       the 32-bit offsets of the batch's records (pairs interleaved: mate 1, mate 2)
//   fa_batch_kernel     per 4 KiB tile of the BATCH: a lane finds the record of its first output byte by a binary search in the offsets,
//                       walks over the record boundaries inside its 16 bytes, cuts every piece out of two aligned 16-byte loads of the
//                       file's joined bases and writes one aligned 16-byte store.  No lane loops over a record.
//
// sylph_fasta_index_window indexes a window of a text that goes on: all its records but the last, whose end nobody has seen yet.
//
// An empty text, a first byte other than '>', a stray '\r', a text of 2^32 - 4096 bytes or more: sylph_fasta_index returns
// SYLPH_ERR_FORMAT and nothing else happens; the caller reads the file with its host reader.  Nothing here guesses.
#include "common.h"
#include "device_common.h"
#include "sketch_session.h"
#include "genomes.h"
#include "text_lines.h"
#include "read_text.h"
#include "fasta_plan.h"
#include "fasta_reads_plan.h"

#include <algorithm>

struct sylph_fasta {
    sylph_ctx* ctx = nullptr;
    sylph::DevBuf text_own;               // the text when it came from the host (else borrowed: `text`)
    const uint8_t* text = nullptr;        // device pointer to byte 0
    uint64_t n = 0;
    sylph::DevBuf tile_base;              // u32 per tile: newlines in front of the tile
    sylph::DevBuf line_start, scan;       // u64 per line (+ 1): first byte; headers << 32 | sequence bytes in front of the line
    sylph::DevBuf rec_off, id_pos, id_len;   // u64 per record (+ 1): first base; u64: first byte of the id; u32: its length
    uint64_t n_tiles = 0, n_lines = 0, n_rec = 0, n_bases = 0, id_bytes = 0;
    // a window's index (sylph_fasta_index_window, final == 0) holds the records in front of the last header: `end` is that header's '>'
    // (else the text's size), and the join reads the text in front of it only
    uint64_t end = 0, join_tiles = 0;
    sylph::DevBuf joined;                 // sylph_sketch_push_fasta: the bases of all records side by side, joined at the first push
    bool joined_ready = false;
    explicit sylph_fasta(sylph_ctx* c)
        : ctx(c), text_own(c), tile_base(c), line_start(c), scan(c), rec_off(c), id_pos(c), id_len(c), joined(c) {}
};

namespace sylph {

namespace {

namespace fp = fasta_plan;
namespace rp = fasta_reads_plan;
static_assert(FQ_TILE == (int)fp::TILE_BYTES && FQ_TPB == (int)fp::TILE_LANES, "text_lines.h and fasta_plan.h cut the same tiles");

// q: what text_lines.h's kernels read and write (n_eff = bytes of the text: a FASTA text is not trimmed; flags: 1 = the first byte is not
// '>', 2 = a stray '\r'); id_bytes: the ids of all records summed
struct FaWords { FqWords q; unsigned long long id_bytes; };

__global__ void fa_init_kernel(const uint8_t* __restrict__ t, uint64_t n, FaWords* __restrict__ w) {
    w->q.n_eff = n;
    w->q.bad_rec = ~0ull;
    w->q.n_bases = 0;
    w->q.n_nl = 0;
    w->q.flags = t[0] == '>' ? 0ull : 1ull;
    w->id_bytes = 0;
}

// the lane's 16 bytes of the aligned stream: its dwords (zero when no byte of it lies in the text) and the mask of bytes inside the text
__device__ __forceinline__ uint32_t fa_lane_load(const uint8_t* __restrict__ al, uint32_t bias, uint64_t n, uint64_t tile, uint32_t w[4], int64_t& i0) {
    const uint64_t p = tile * fp::TILE_BYTES + (uint64_t)threadIdx.x * fp::LANE_BYTES;
    i0 = (int64_t)p - (int64_t)bias;
    const uint32_t valid = fp::lane_valid(i0, n);
    w[0] = w[1] = w[2] = w[3] = 0;
    if (valid) {
        const uint4 v = *reinterpret_cast<const uint4*>(al + p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    return valid;
}

__global__ __launch_bounds__(FQ_TPB) void fa_count_kernel(const uint8_t* __restrict__ al, uint32_t bias, uint64_t n, FaWords* __restrict__ w,
                                                          uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t s_wave[FQ_TPB / 64];
    uint32_t d[4];
    int64_t i0;
    const uint32_t valid = fa_lane_load(al, bias, n, blockIdx.x, d, i0);
    const uint32_t nl = fp::lane_mask(d, '\n') & valid, cr = fp::lane_mask(d, '\r') & valid;
    if (cr) {
        const int64_t nx = i0 + (int64_t)fp::LANE_BYTES;                 // the byte behind the lane (inside the text: readable)
        const bool next_ok = nx >= (int64_t)n || al[nx + bias] == '\n';
        if (fp::lane_stray_cr(cr, nl, valid, next_ok)) atomicOr(&w->q.flags, 2ull);
    }
    uint32_t tot = 0;
    (void)block_excl_sum<FQ_TPB>(__popc(nl), s_wave, &tot);
    if (threadIdx.x == 0) {
        tile_cnt[blockIdx.x] = tot;
        if (tot) atomicAdd(&w->q.n_nl, (unsigned long long)tot);
    }
}

// line L = bytes [line_start[L], line_start[L + 1] - 1); value[n_lines] = 0 is the scan's sentinel
__global__ __launch_bounds__(256) void fa_values_kernel(const uint8_t* __restrict__ t, const uint64_t* __restrict__ line_start, uint64_t n_lines,
                                                        uint64_t* __restrict__ value) {
    const uint64_t L = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (L > n_lines) return;
    uint64_t v = 0;
    if (L < n_lines) {
        const uint64_t s = line_start[L], raw = line_start[L + 1] - 1 - s;
        v = raw ? fp::line_value(raw, t[s], t[s + raw - 1]) : 0ull;
    }
    value[L] = v;
}

__global__ __launch_bounds__(256) void fa_records_kernel(const uint8_t* __restrict__ t, const uint64_t* __restrict__ line_start,
                                                         const uint64_t* __restrict__ scan, uint64_t n_lines, uint64_t n_rec,
                                                         uint64_t* __restrict__ rec_off, uint64_t* __restrict__ id_pos,
                                                         uint32_t* __restrict__ id_len, FaWords* __restrict__ w) {
    const uint64_t L = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long idl = 0;
    if (L < n_lines) {
        const uint64_t sl = scan[L], sn = scan[L + 1];
        if (fp::scan_line_is_header(sl, sn)) {
            const uint64_t r = fp::scan_headers(sl);
            const uint64_t s = line_start[L], raw = line_start[L + 1] - 1 - s;
            idl = fp::line_len(raw, t[s + raw - 1]) - 1;                 // without the '>'
            if (r < n_rec) {
                rec_off[r] = fp::scan_bases(sl);
                id_pos[r] = s + 1;
                id_len[r] = (uint32_t)idl;
            }
        }
    }
    if (L == n_lines) rec_off[n_rec] = fp::scan_bases(scan[n_lines]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) idl += __shfl_xor(idl, d);
    if ((threadIdx.x & 63) == 0 && idl) atomicAdd(&w->id_bytes, idl);
}

// One workgroup per tile.  out = where base 0 of this text goes (any address); n_bases = bases of the text (nothing is written behind
// them).  *err is set when the line table and the tile's own count of kept bytes disagree (never, for an index this file built).
__global__ __launch_bounds__(FQ_TPB) void fa_join_kernel(const uint8_t* __restrict__ al, uint32_t bias, uint64_t n,
                                                         const uint32_t* __restrict__ tile_base, const uint64_t* __restrict__ line_start,
                                                         const uint64_t* __restrict__ scan, uint8_t* __restrict__ out, uint32_t n_bases,
                                                         uint32_t* __restrict__ err) {
    __shared__ uint32_t s_wave[FQ_TPB / 64];
    __shared__ uint32_t s_d0;
    __shared__ uint4 s_buf[fp::TILE_LANES + 2];                          // the tile's kept bytes from index (address & 15) on
    uint8_t* const s_bytes = reinterpret_cast<uint8_t*>(s_buf);
    uint32_t d[4];
    int64_t i0;
    const uint32_t valid = fa_lane_load(al, bias, n, blockIdx.x, d, i0);
    const uint32_t nl = fp::lane_mask(d, '\n') & valid, cr = fp::lane_mask(d, '\r') & valid, gt = fp::lane_mask(d, '>') & valid;
    const uint64_t L = (uint64_t)tile_base[blockIdx.x] + block_excl_sum<FQ_TPB>(__popc(nl), s_wave, nullptr);   // the line of the lane's first byte
    uint32_t keep = 0, dest = 0;
    if (valid) {
        const uint64_t sl = scan[L], sn = scan[L + 1];
        dest = fp::dest_at((uint64_t)(i0 < 0 ? 0 : i0), line_start[L], sl, sn);
        keep = fp::lane_keep(nl, cr, gt, valid, fp::scan_line_is_header(sl, sn));
    }
    if (threadIdx.x == 0) s_d0 = dest;                                   // (lane 0 of every tile holds a byte of the text)
    uint32_t kept = 0;
    const uint32_t off = block_excl_sum<FQ_TPB>(__popc(keep), s_wave, &kept);      // (its barriers publish s_d0)
    const uint32_t d0 = s_d0;
    if (valid && dest != d0 + off) atomicOr(err, 1u);
    if ((uint64_t)d0 + kept > n_bases) { if (threadIdx.x == 0) atomicOr(err, 2u); return; }      // (uniform)
    uint8_t* const first = out + d0;
    const uint32_t shift = (uint32_t)((uintptr_t)first & 15);
    uint32_t o = shift + off;
#pragma unroll
    for (uint32_t b = 0; b < fp::LANE_BYTES; b++)
        if (keep >> b & 1u) s_bytes[o++] = (uint8_t)(d[b >> 2] >> (8 * (b & 3)));
    __syncthreads();
    uint8_t* const base = first - shift;                                 // 16-byte aligned
    const uint32_t chunks = fp::store_chunks(shift, kept);
    for (uint32_t j = threadIdx.x; j < chunks; j += FQ_TPB) {
        uint32_t lo, hi;
        fp::store_chunk_range(j, shift, kept, lo, hi);
        if (lo == 0 && hi == fp::LANE_BYTES) *reinterpret_cast<uint4*>(base + (size_t)j * fp::LANE_BYTES) = s_buf[j];
        else for (uint32_t x = lo; x < hi; x++) base[(size_t)j * fp::LANE_BYTES + x] = s_bytes[j * fp::LANE_BYTES + x];
    }
}

// one wavefront per record: its id from the text to its place behind the offsets
__global__ __launch_bounds__(256) void fa_ids_kernel(const uint8_t* __restrict__ t, const uint64_t* __restrict__ id_pos, uint64_t first, uint64_t n_rec,
                                                     const uint64_t* __restrict__ off, uint8_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t j = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < n_rec; j += waves) {
        const uint64_t o = off[j], len = off[j + 1] - o;
        const uint8_t* src = t + id_pos[first + j];
        for (uint64_t x = lane; x < len; x += 64) out[o + x] = src[x];
    }
}

// how a batch's record j reads its length (read_text.h batch_lens_kernel): from its file's record offsets (fasta_reads_plan.h batch_len)
struct FaLen {
    const uint64_t *ra, *rb;
    __device__ uint32_t operator()(uint64_t first, uint64_t j) const { return rp::batch_len(ra, rb, first, j); }
};

// the header of record r for the mate check (read_text.h mates_kernel): the '>' line behind its '>', without its line end
struct FaHdr {
    const uint8_t* t;
    const uint64_t* id_pos;
    const uint32_t* id_len;
    __device__ const uint8_t* operator()(uint64_t r, uint64_t& n) const { n = id_len[r]; return t + id_pos[r]; }
};

// One workgroup per 4 KiB tile of the batch, one lane per 16 output bytes (fasta_reads_plan.h lane_walk).  ja / jb: the joined bases of
// the two files (16-byte aligned, readable 32 bytes past their last base; jb = nullptr: single-end), ra / rb: their record offsets;
// off: the batch's offsets, n_rec of them + 1, off[n_rec] = total; bases: 16-byte aligned, room for total rounded up to 16.
__global__ __launch_bounds__(FQ_TPB) void fa_batch_kernel(const uint8_t* __restrict__ ja, const uint64_t* __restrict__ ra,
                                                          const uint8_t* __restrict__ jb, const uint64_t* __restrict__ rb, uint64_t first,
                                                          uint64_t n_rec, const uint32_t* __restrict__ off, uint64_t total,
                                                          uint8_t* __restrict__ bases) {
    const uint64_t o = (uint64_t)blockIdx.x * rp::TILE_BYTES + (uint64_t)threadIdx.x * rp::LANE_BYTES;
    if (o >= total) return;
    uint64_t out_lo = 0, out_hi = 0;
    rp::lane_walk(off, n_rec, total, o, [&](uint64_t j, uint64_t p, uint32_t b0, uint32_t len) {
        const uint8_t* src = (rp::mate_of(j, rb != nullptr) ? jb : ja) + rp::source_of(off, ra, rb, first, j, p);
        const uint32_t sh = (uint32_t)((uintptr_t)src & 15);
        const uint4* al = reinterpret_cast<const uint4*>(src - sh);
        const uint4 a = al[0], b = al[1];
        uint64_t lo, hi;
        rp::cut16((uint64_t)a.x | (uint64_t)a.y << 32, (uint64_t)a.z | (uint64_t)a.w << 32, (uint64_t)b.x | (uint64_t)b.y << 32,
                  (uint64_t)b.z | (uint64_t)b.w << 32, sh, lo, hi);
        rp::lay16(lo, hi, b0, len, out_lo, out_hi);
    });
    *reinterpret_cast<uint4*>(bases + o) = make_uint4((uint32_t)out_lo, (uint32_t)(out_lo >> 32), (uint32_t)out_hi, (uint32_t)(out_hi >> 32));
}

// window: the text goes on behind its last byte (sylph_fasta_index_window, final == 0) — the same kernels over the same bytes, and then
// the last header's record is taken off the index again (fasta_reads_plan.h window_records)
void fasta_index_impl(sylph_fasta* f, const void* text, uint64_t n_bytes, int mem, bool window = false) {
    sylph_ctx* ctx = f->ctx;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard dg(ctx->device);
    if (mem != SYLPH_MEM_DEVICE && ((const uint8_t*)text)[0] != '>') throw FormatError{"the first byte is not '>'"};   // (before anything travels)
    const auto [al, bias, n_tiles] = take_text(ctx, f->text_own, &f->text, text, n_bytes, mem);
    f->n = n_bytes;
    f->n_tiles = n_tiles;
    DevBuf& b_words = ctx->scratch[0];
    DevBuf& b_cnt = ctx->scratch[1];
    DevBuf& b_val = ctx->scratch[2];
    b_words.reserve(sizeof(FaWords));
    b_cnt.reserve((n_tiles + 1) * 4);
    f->tile_base.reserve((n_tiles + 1) * 4);
    FaWords* d_w = b_words.as<FaWords>();
    hipLaunchKernelGGL(fa_init_kernel, dim3(1), dim3(1), 0, ctx->stream, f->text, n_bytes, d_w);
    SY_HIP(hipMemsetAsync(b_cnt.as<uint32_t>() + n_tiles, 0, 4, ctx->stream));
    hipLaunchKernelGGL(fa_count_kernel, dim3((uint32_t)n_tiles), dim3(FQ_TPB), 0, ctx->stream, al, bias, n_bytes, d_w, b_cnt.as<uint32_t>());
    SY_HIP(hipGetLastError());
    exclusive_sum_u32(ctx, b_cnt.as<uint32_t>(), f->tile_base.as<uint32_t>(), n_tiles + 1);
    FaWords hw;
    uint32_t n_nl = 0;
    ctx->read_back(&n_nl, f->tile_base.as<uint32_t>() + n_tiles, 4);     // (synchronises the stream)
    ctx->read_back(&hw, d_w, sizeof(hw));
    if (hw.q.flags & 1ull) throw FormatError{"the first byte is not '>'"};
    if (hw.q.flags & 2ull) throw FormatError{"a '\\r' that is not directly followed by '\\n' or by the end of the text"};
    if (hw.q.n_nl != (unsigned long long)n_nl || !fp::line_count_ok(hw.q.n_nl)) throw FormatError{std::to_string(hw.q.n_nl + 1) + " lines: at most 2^32 - 1 per index"};
    const uint64_t n_lines = (uint64_t)n_nl + 1;                         // the last line needs no newline (it may be empty)
    f->n_lines = n_lines;
    f->line_start.reserve((n_lines + 1) * 8);
    f->scan.reserve((n_lines + 1) * 8);
    b_val.reserve((n_lines + 1) * 8);
    hipLaunchKernelGGL(fq_lines_kernel, dim3((uint32_t)n_tiles), dim3(FQ_TPB), 0, ctx->stream, al, bias, &d_w->q, f->tile_base.as<uint32_t>(), n_lines,
                       f->line_start.as<uint64_t>());
    hipLaunchKernelGGL(fa_values_kernel, dim3(grid1(n_lines + 1, 256, 1u << 30)), dim3(256), 0, ctx->stream, f->text, f->line_start.as<uint64_t>(), n_lines,
                       b_val.as<uint64_t>());
    SY_HIP(hipGetLastError());
    exclusive_sum_u64(ctx, b_val.as<uint64_t>(), f->scan.as<uint64_t>(), n_lines + 1);
    uint64_t total = 0;
    ctx->read_back(&total, f->scan.as<uint64_t>() + n_lines, 8);
    f->n_rec = fp::scan_headers(total);
    f->n_bases = fp::scan_bases(total);
    f->rec_off.reserve((f->n_rec + 1) * 8);
    f->id_pos.reserve(f->n_rec * 8 + 8);
    f->id_len.reserve(f->n_rec * 4 + 4);
    hipLaunchKernelGGL(fa_records_kernel, dim3(grid1(n_lines + 1, 256, 1u << 30)), dim3(256), 0, ctx->stream, f->text, f->line_start.as<uint64_t>(),
                       f->scan.as<uint64_t>(), n_lines, f->n_rec, f->rec_off.as<uint64_t>(), f->id_pos.as<uint64_t>(), f->id_len.as<uint32_t>(), d_w);
    SY_HIP(hipGetLastError());
    ctx->read_back(&hw, d_w, sizeof(hw));
    f->id_bytes = hw.id_bytes;
    f->end = n_bytes;
    f->join_tiles = n_tiles;
    if (!window) return;
    const uint64_t headers = f->n_rec;
    uint64_t last_at = 0;
    if (headers >= 2) {
        uint64_t last_base = 0, last_id = 0;
        uint32_t last_id_len = 0;
        ctx->read_back(&last_base, f->rec_off.as<uint64_t>() + headers - 1, 8);
        ctx->read_back(&last_id, f->id_pos.as<uint64_t>() + headers - 1, 8);
        ctx->read_back(&last_id_len, f->id_len.as<uint32_t>() + headers - 1, 4);
        last_at = last_id - 1;
        f->n_bases = last_base;
        f->id_bytes -= last_id_len;
    } else {
        f->n_bases = 0;
        f->id_bytes = 0;
    }
    f->n_rec = rp::window_records(headers, false);
    f->end = rp::window_consumed(headers, false, n_bytes, last_at);
    f->join_tiles = f->end ? (f->end + bias + FQ_TILE - 1) / FQ_TILE : 0;
}

// the text's sequences joined to out[0, n_bases) (device memory, any alignment); the caller holds the context's lock.  d_err: one zeroed word
void fasta_join(sylph_fasta* f, uint8_t* out, uint32_t* d_err) {
    sylph_ctx* ctx = f->ctx;
    const uint32_t bias = (uint32_t)((uintptr_t)f->text & 15);
    ScopedKernelTimer t(ctx, "fasta_join");
    if (!f->join_tiles) return;
    hipLaunchKernelGGL(fa_join_kernel, dim3((uint32_t)f->join_tiles), dim3(FQ_TPB), 0, ctx->stream, f->text - bias, bias, f->end, f->tile_base.as<uint32_t>(),
                       f->line_start.as<uint64_t>(), f->scan.as<uint64_t>(), out, (uint32_t)f->n_bases, d_err);
    SY_HIP(hipGetLastError());
}

void check_join(sylph_ctx* ctx, const uint32_t* d_err) {
    uint32_t e = 0;
    ctx->read_back(&e, d_err, 4);
    SY_REQUIRE(e == 0, "internal: the FASTA join disagrees with its line table (%u)", e);
}

}  // namespace
}  // namespace sylph

using namespace sylph;

extern "C" {

int sylph_fasta_index(sylph_ctx* ctx, const void* text, uint64_t n_bytes, int mem, sylph_fasta** out) {
    if (!ctx || !out || (!text && n_bytes)) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    if (!mem_kind_ok(mem)) return SYLPH_ERR_INVALID;
    *out = nullptr;
    if (n_bytes == 0) { set_error("sylph_fasta_index: no text"); return SYLPH_ERR_FORMAT; }
    if (!fasta_plan::text_size_ok(n_bytes)) {
        set_error("sylph_fasta_index: %llu bytes of text: fewer than 2^32 - 4096 per index", (unsigned long long)n_bytes);
        return SYLPH_ERR_FORMAT;
    }
    return make_index(ctx, "sylph_fasta_index", "not FASTA text this index takes", out, [&](sylph_fasta* f) { fasta_index_impl(f, text, n_bytes, mem); });
}

int sylph_fasta_index_window(sylph_ctx* ctx, const void* text, uint64_t n_bytes, int mem, int final, sylph_fasta** out, uint64_t* consumed) {
    if (!ctx || !out || !consumed || (!text && n_bytes)) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    if (!mem_kind_ok(mem)) return SYLPH_ERR_INVALID;
    *out = nullptr;
    *consumed = 0;
    if (final) {                                                         // exactly sylph_fasta_index
        const int rc = sylph_fasta_index(ctx, text, n_bytes, mem, out);
        if (rc == SYLPH_OK) *consumed = n_bytes;
        return rc;
    }
    if (n_bytes && !fasta_plan::text_size_ok(n_bytes)) {
        set_error("sylph_fasta_index_window: %llu bytes of text: fewer than 2^32 - 4096 per index", (unsigned long long)n_bytes);
        return SYLPH_ERR_FORMAT;
    }
    const int rc = make_index(ctx, "sylph_fasta_index_window", "not FASTA text this index takes", out, [&](sylph_fasta* f) {
        if (n_bytes) fasta_index_impl(f, text, n_bytes, mem, true);      // (no text yet: no records, nothing consumed)
    });
    if (rc == SYLPH_OK) *consumed = (*out)->end;
    return rc;
}

int sylph_fasta_record_offset(sylph_fasta* f, uint64_t record, uint64_t* offset) {
    return guarded([&] {
        SY_REQUIRE(f && offset, "null argument");
        SY_REQUIRE(record <= f->n_rec, "sylph_fasta_record_offset: record %llu of %llu", (unsigned long long)record, (unsigned long long)f->n_rec);
        if (record == f->n_rec) { *offset = f->end; return; }
        std::lock_guard<std::mutex> lock(f->ctx->mu);
        DeviceGuard dg(f->ctx->device);
        unsigned long long v = 0;
        f->ctx->d2h(&v, f->id_pos.as<uint64_t>() + record, 8);
        *offset = v - 1;                                                 // the id begins behind the '>'
    });
}

int sylph_sketch_push_fasta(sylph_sketch* sk, sylph_fasta* a, sylph_fasta* b, uint64_t first, uint64_t n_items) {
    if (!sk || !a) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    sylph_ctx* ctx = sk->ctx;
    const uint64_t* ra = a->rec_off.as<uint64_t>();
    const uint64_t* rb = b ? b->rec_off.as<uint64_t>() : nullptr;
    return push_read_text(
        "sylph_sketch_push_fasta", sk, a, b, first, n_items, FaLen{ra, rb},
        [&] {                                                            // room for the files that are not joined yet
            uint64_t to_join = 0;
            for (sylph_fasta* f : {a, b}) if (f && !f->joined_ready) to_join += f->n_bases + 64;
            return to_join;
        },
        [&] {                                                            // (a) the join, once per index: the file's bases side by side in a buffer of the index
            ctx->counters.reserve(64);
            bool joined_now = false;
            for (sylph_fasta* f : {a, b}) {
                if (!f || f->joined_ready) continue;
                f->joined.reserve(f->n_bases + 64);
                if (!joined_now) SY_HIP(hipMemsetAsync(ctx->counters.p, 0, 4, ctx->stream));
                if (f->n_bases) fasta_join(f, f->joined.as<uint8_t>(), ctx->counters.as<uint32_t>());
                joined_now = true;
            }
            if (joined_now) {
                check_join(ctx, ctx->counters.as<uint32_t>());
                for (sylph_fasta* f : {a, b}) if (f) f->joined_ready = true;
            }
        },
        [&](const uint32_t* off, uint64_t n_rec_batch, uint64_t n_bases) {   // (b) the gather, cut by output bytes
            if (!n_bases) return;
            ScopedKernelTimer t(ctx, "fasta_batch");
            hipLaunchKernelGGL(fa_batch_kernel, dim3((uint32_t)((n_bases + rp::TILE_BYTES - 1) / rp::TILE_BYTES)), dim3(FQ_TPB), 0, ctx->stream,
                               a->joined.as<uint8_t>(), ra, b ? b->joined.as<uint8_t>() : nullptr, rb, first, n_rec_batch, off, n_bases,
                               sk->fq_bases.as<uint8_t>());
        });
}

// The pairs of ONE interleaved text (interleave_plan.h: pair p = records 2 p and 2 p + 1) to a paired session: the batch is the
// records as they lie, which is the order a paired batch has — the single-end launch, fed record 2 first_pair + j
int sylph_sketch_push_fasta_interleaved(sylph_sketch* sk, sylph_fasta* f, uint64_t first_pair, uint64_t n_pairs) {
    if (!sk || !f) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    const char* entry = "sylph_sketch_push_fasta_interleaved";
    if (n_pairs >= (1ull << 30)) { set_error("%s: at most 2^31 - 1 records per push (%llu pairs)", entry, (unsigned long long)n_pairs); return SYLPH_ERR_INVALID; }
    const uint64_t pairs = interleave_plan::pairs_of(f->n_rec);
    if (first_pair > pairs || n_pairs > pairs - first_pair) {
        set_error("%s: pairs [%llu, +%llu) are not all there (%llu records)", entry, (unsigned long long)first_pair, (unsigned long long)n_pairs, (unsigned long long)f->n_rec);
        return SYLPH_ERR_INVALID;
    }
    sylph_ctx* ctx = sk->ctx;
    const uint64_t first = interleave_plan::record_of(first_pair, 0);
    const uint64_t* ra = f->rec_off.as<uint64_t>();
    return push_read_text(
        entry, sk, f, (sylph_fasta*)nullptr, first, 2 * n_pairs, FaLen{ra, nullptr},
        [&] { return f->joined_ready ? uint64_t(0) : f->n_bases + 64; },
        [&] {                                                            // the join, once per index (as sylph_sketch_push_fasta's)
            if (f->joined_ready) return;
            ctx->counters.reserve(64);
            f->joined.reserve(f->n_bases + 64);
            SY_HIP(hipMemsetAsync(ctx->counters.p, 0, 4, ctx->stream));
            if (f->n_bases) fasta_join(f, f->joined.as<uint8_t>(), ctx->counters.as<uint32_t>());
            check_join(ctx, ctx->counters.as<uint32_t>());
            f->joined_ready = true;
        },
        [&](const uint32_t* off, uint64_t n_rec_batch, uint64_t n_bases) {
            if (!n_bases) return;
            ScopedKernelTimer t(ctx, "fasta_batch");
            hipLaunchKernelGGL(fa_batch_kernel, dim3((uint32_t)((n_bases + rp::TILE_BYTES - 1) / rp::TILE_BYTES)), dim3(FQ_TPB), 0, ctx->stream,
                               f->joined.as<uint8_t>(), ra, (const uint8_t*)nullptr, (const uint64_t*)nullptr, first, n_rec_batch, off, n_bases,
                               sk->fq_bases.as<uint8_t>());
        },
        true);
}

int sylph_fasta_mates(sylph_fasta* f, uint64_t first_pair, uint64_t n_pairs, uint64_t* first_bad) {
    return index_mates("sylph_fasta_mates", f, first_pair, n_pairs, first_bad,
                       [&] { return FaHdr{f->text, f->id_pos.as<uint64_t>(), f->id_len.as<uint32_t>()}; });
}

int sylph_fasta_counts(const sylph_fasta* f, uint64_t* n_records, uint64_t* n_bases, uint64_t* id_bytes) {
    if (!f) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    if (n_records) *n_records = f->n_rec;
    if (n_bases) *n_bases = f->n_bases;
    if (id_bytes) *id_bytes = f->id_bytes;
    return SYLPH_OK;
}

int sylph_fasta_lengths(sylph_fasta* f, uint64_t first, uint64_t n, uint64_t* out) {
    return guarded([&] {
        SY_REQUIRE(f && (out || n == 0), "null argument");
        SY_REQUIRE(first <= f->n_rec && n <= f->n_rec - first, "sylph_fasta_lengths: records [%llu, +%llu) of %llu", (unsigned long long)first,
                   (unsigned long long)n, (unsigned long long)f->n_rec);
        if (!n) return;
        std::vector<uint64_t> off(n + 1);
        {
            std::lock_guard<std::mutex> lock(f->ctx->mu);
            DeviceGuard dg(f->ctx->device);
            f->ctx->d2h(off.data(), f->rec_off.as<uint64_t>() + first, (n + 1) * 8);
        }
        for (uint64_t i = 0; i < n; i++) out[i] = off[i + 1] - off[i];
    });
}

int sylph_fasta_ids(sylph_fasta* f, uint64_t first, uint64_t n, char* out, uint64_t cap, uint64_t* id_off) {
    return guarded([&] {
        SY_REQUIRE(f && id_off && (out || cap == 0), "null argument");
        SY_REQUIRE(first <= f->n_rec && n <= f->n_rec - first, "sylph_fasta_ids: records [%llu, +%llu) of %llu", (unsigned long long)first,
                   (unsigned long long)n, (unsigned long long)f->n_rec);
        id_off[0] = 0;
        if (!n) return;
        sylph_ctx* ctx = f->ctx;
        std::lock_guard<std::mutex> lock(ctx->mu);
        DeviceGuard dg(ctx->device);
        std::vector<uint32_t> len(n);
        ctx->d2h(len.data(), f->id_len.as<uint32_t>() + first, n * 4);
        for (uint64_t i = 0; i < n; i++) id_off[i + 1] = id_off[i] + len[i];
        const uint64_t total = id_off[n];
        SY_REQUIRE(total <= cap, "sylph_fasta_ids: %llu bytes of ids, room for %llu", (unsigned long long)total, (unsigned long long)cap);
        if (!total) return;
        DevBuf d_off(ctx), d_out(ctx);
        d_off.reserve((n + 1) * 8);
        d_out.reserve(total);
        ctx->h2d(d_off.p, id_off, (n + 1) * 8);
        hipLaunchKernelGGL(fa_ids_kernel, dim3(grid1(n, 4, 1u << 16)), dim3(256), 0, ctx->stream, f->text, f->id_pos.as<uint64_t>(), first, n,
                           d_off.as<uint64_t>(), d_out.as<uint8_t>());
        SY_HIP(hipGetLastError());
        ctx->d2h(out, d_out.p, total);
    });
}

int sylph_fasta_bases(sylph_fasta* f, uint64_t first, uint64_t n, uint8_t* host_out) {
    return guarded([&] {
        SY_REQUIRE(f, "null argument");
        SY_REQUIRE(first <= f->n_rec && n <= f->n_rec - first, "sylph_fasta_bases: records [%llu, +%llu) of %llu", (unsigned long long)first,
                   (unsigned long long)n, (unsigned long long)f->n_rec);
        if (!n || !f->n_bases) return;
        sylph_ctx* ctx = f->ctx;
        std::lock_guard<std::mutex> lock(ctx->mu);
        DeviceGuard dg(ctx->device);
        uint64_t range[2];
        ctx->read_back(&range[0], f->rec_off.as<uint64_t>() + first, 8);
        ctx->read_back(&range[1], f->rec_off.as<uint64_t>() + first + n, 8);
        if (range[1] == range[0]) return;
        SY_REQUIRE(host_out, "null argument");
        DevBuf d_all(ctx);
        d_all.reserve(f->n_bases + 64);
        ctx->counters.reserve(64);
        SY_HIP(hipMemsetAsync(ctx->counters.p, 0, 4, ctx->stream));
        fasta_join(f, d_all.as<uint8_t>(), ctx->counters.as<uint32_t>());
        check_join(ctx, ctx->counters.as<uint32_t>());
        ctx->d2h(host_out, d_all.as<uint8_t>() + range[0], range[1] - range[0]);
    });
}

void sylph_fasta_destroy(sylph_fasta* f) {
    if (!f) return;
    sylph_ctx* ctx = f->ctx;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        DeviceGuard dg(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);       // kernels that read the text / the index may still be queued
        delete f;
    }
    ctx_unref(ctx);
}

int sylph_sketch_genomes_fasta(sylph_ctx* ctx, sylph_fasta* const* files, uint32_t n_files, int individual, uint32_t c, uint32_t k, int seed_mode,
                               uint64_t min_spacing, int pseudotax, uint64_t** out_kmers, uint64_t* kmer_off, uint64_t** out_tracked,
                               uint64_t* tracked_off) {
    return guarded([&] {
        SY_REQUIRE(ctx && out_kmers && kmer_off && (files || n_files == 0), "null argument");
        SY_REQUIRE((out_tracked == nullptr) == (tracked_off == nullptr), "out_tracked and tracked_off go together");
        uint64_t n_bases = 0, n_contigs = 0;
        for (uint32_t i = 0; i < n_files; i++) {
            SY_REQUIRE(files[i] && files[i]->ctx == ctx, "sylph_sketch_genomes_fasta: file %u is null or lives on another context", i);
            n_bases += files[i]->n_bases;
            n_contigs += files[i]->n_rec;
        }
        SY_REQUIRE(n_bases < (1ull << 32), "batch larger than 2^32-1 bases: split it");
        // contigs of all files side by side; one genome per file, or one per record
        std::vector<uint64_t> contig_off(n_contigs + 1), genome_off;
        genome_off.reserve((individual ? n_contigs : n_files) + 1);
        genome_off.push_back(0);
        DevBuf batch(ctx);
        auto release = [&] { std::lock_guard<std::mutex> lock(ctx->mu); DeviceGuard dg(ctx->device); batch.release(); };
        try {
            {
                std::lock_guard<std::mutex> lock(ctx->mu);
                DeviceGuard dg(ctx->device);
                batch.reserve(n_bases + 64);
                ctx->counters.reserve(64);
                SY_HIP(hipMemsetAsync(ctx->counters.p, 0, 4, ctx->stream));
                SY_HIP(hipMemsetAsync(batch.as<uint8_t>() + n_bases, 0, 64, ctx->stream));
                uint64_t base = 0, contig = 0;
                contig_off[0] = 0;
                for (uint32_t i = 0; i < n_files; i++) {
                    sylph_fasta* f = files[i];
                    if (f->n_rec) {
                        ctx->d2h(contig_off.data() + contig, f->rec_off.as<uint64_t>(), (f->n_rec + 1) * 8);
                        for (uint64_t r = 0; r <= f->n_rec; r++) contig_off[contig + r] += base;
                    }
                    if (f->n_bases) fasta_join(f, batch.as<uint8_t>() + base, ctx->counters.as<uint32_t>());
                    if (individual) for (uint64_t r = 1; r <= f->n_rec; r++) genome_off.push_back(contig + r);
                    base += f->n_bases;
                    contig += f->n_rec;
                    if (!individual) genome_off.push_back(contig);
                }
                check_join(ctx, ctx->counters.as<uint32_t>());
            }
            sketch_genomes_impl(ctx, batch.as<uint8_t>(), contig_off.data(), n_contigs, genome_off.data(), genome_off.size() - 1, c, k, seed_mode,
                                min_spacing, pseudotax, SYLPH_MEM_DEVICE, out_kmers, kmer_off, out_tracked, tracked_off);
        } catch (...) { release(); throw; }
        release();
    });
}

}  // extern "C"
