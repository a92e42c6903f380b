// fastq.hip — the records of plain four-line FASTQ text, found on the device.
//
// The reference reads a sample's files record by record with needletail (sketch.rs:775-815, :897-921: parse_fastx_file + next())
// and hands each record's sequence to the seeding; the host feed of this repository (host/feed.cpp) does the same job with all parse
// threads: index the newlines, gather the sequence lines, pack them, send 0.25 B per base.  On a box whose container may use 16
// CPUs that is 60-110 ms of host work per 1 Gbp sample against ~1 ms of GPU work.  Here the TEXT travels (2.1 B per base over
// PCIe, ~37 ms per Gbp) and the device does the rest:
//
//   fq_trim_kernel      trailing '\n' / '\r' bytes are not part of the text (needletail ignores blank space behind the last record)
//   fq_count_kernel     newlines per 4 KiB tile                      (one 16-byte load per lane, exact SWAR byte test)
//   exclusive scan      first line number of every tile
//   fq_lines_kernel     start of every line: line_start[L], L = 0 .. n_lines (the last entry is one past a virtual final newline)
//   fq_records_kernel   record r = lines 4r .. 4r+3: '@' and '+' in place, sequence and quality equally long (a '\r' in front of the
//                       newline is not part of a line); start + length of the sequence line, the bases of the text summed
//   fq_gather_kernel    a batch's sequences copied side by side (pairs interleaved: mate 1, mate 2) behind one offsets array — the
//                       (bases, rec_off) batch every seeding kernel of this library takes (SYLPH_MEM_DEVICE, SYLPH_ENC_ASCII)
//
// Anything that is not exactly that — a line count that is no multiple of four, a record without its '@' or '+', unequal lengths
// (multi-line FASTQ, FASTA, damage) — makes sylph_fastq_index return SYLPH_ERR_FORMAT: the caller then reads the file with its host
// reader, whose record and error semantics are needletail's (host/formats.cpp ChunkStream).  Nothing here guesses.
#include "common.h"
#include "device_common.h"
#include "sketch_session.h"
#include "text_lines.h"
#include "read_text.h"

struct sylph_fastq {
    sylph_ctx* ctx = nullptr;
    sylph::DevBuf text_own;               // the text when it came from the host (else borrowed: `text`)
    const uint8_t* text = nullptr;        // device pointer to byte 0
    uint64_t n = 0;                       // bytes without the trailing blank space
    sylph::DevBuf seq_start, seq_len;     // u64 / u32 per record
    sylph::DevBuf hdr_start;              // u64 per record: where its '@' line starts (all three kinds of index: the mate check reads the header)
    sylph::DevBuf rec_start;              // sylph_fastq_index_window only: u64 per record + one, where its '@' line starts (the last: behind the records)
    bool has_starts = false;
    uint64_t n_rec = 0, n_bases = 0;
    explicit sylph_fastq(sylph_ctx* c) : ctx(c), text_own(c), seq_start(c), seq_len(c), hdr_start(c), rec_start(c) {}
};

namespace sylph {
namespace {

constexpr uint32_t FQ_MAX_TRAILING = 1u << 16;

__global__ void fq_trim_kernel(const uint8_t* __restrict__ t, uint64_t n, FqWords* __restrict__ w) {
    uint64_t e = n;
    uint32_t steps = 0;
    while (e > 0 && (t[e - 1] == '\n' || t[e - 1] == '\r') && steps < FQ_MAX_TRAILING) { e--; steps++; }
    w->n_eff = e;
    w->bad_rec = ~0ull;
    w->n_bases = 0;
    w->n_nl = 0;
    w->flags = (e > 0 && (t[e - 1] == '\n' || t[e - 1] == '\r')) ? 1ull : 0ull;
}

__global__ __launch_bounds__(FQ_TPB) void fq_count_kernel(const uint8_t* __restrict__ al, uint32_t bias, FqWords* __restrict__ w,
                                                          uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t s_wave[FQ_TPB / 64];
    uint32_t f[4];
    int64_t i0;
    lane_flags(al, bias, w->n_eff, blockIdx.x, f, i0);
    const uint32_t c = __popc(f[0]) + __popc(f[1]) + __popc(f[2]) + __popc(f[3]);
    uint32_t tot = 0;
    (void)block_excl_sum<FQ_TPB>(c, s_wave, &tot);
    if (threadIdx.x == 0) {
        tile_cnt[blockIdx.x] = tot;
        if (tot) atomicAdd(&w->n_nl, (unsigned long long)tot);
    }
}

__global__ __launch_bounds__(256) void fq_records_kernel(const uint8_t* __restrict__ t, const uint64_t* __restrict__ line_start, uint64_t n_rec,
                                                         uint64_t* __restrict__ seq_start, uint32_t* __restrict__ seq_len,
                                                         uint64_t* __restrict__ hdr_start, FqWords* __restrict__ w) {
    __shared__ unsigned long long s_sum[4];
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long len = 0;
    if (r < n_rec) {
        const uint64_t s0 = line_start[4 * r], s1 = line_start[4 * r + 1], s2 = line_start[4 * r + 2], s3 = line_start[4 * r + 3],
                       s4 = line_start[4 * r + 4];
        uint64_t sl = s2 - 1 - s1, ql = s4 - 1 - s3;
        if (sl && t[s1 + sl - 1] == '\r') sl--;
        if (ql && t[s3 + ql - 1] == '\r') ql--;
        const bool ok = t[s0] == '@' && t[s2] == '+' && sl == ql && sl <= 0xFFFFFFFEull;
        if (!ok) atomicMin(&w->bad_rec, (unsigned long long)r);
        seq_start[r] = s1;
        hdr_start[r] = s0;
        seq_len[r] = ok ? (uint32_t)sl : 0u;
        len = ok ? sl : 0ull;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) len += __shfl_xor(len, d);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = len;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&w->n_bases, s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]);
}

// one wavefront per record: its bytes from the text to their place in the batch
__global__ __launch_bounds__(256) void fq_gather_kernel(const uint8_t* __restrict__ ta, const uint64_t* __restrict__ sa, const uint8_t* __restrict__ tb,
                                                        const uint64_t* __restrict__ sb, uint64_t first, uint64_t n_rec_batch,
                                                        const uint32_t* __restrict__ off, uint8_t* __restrict__ bases) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t j = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < n_rec_batch; j += waves) {
        const uint32_t o = off[j], len = off[j + 1] - o;
        const uint8_t* src = tb ? ((j & 1) ? tb + sb[first + (j >> 1)] : ta + sa[first + (j >> 1)]) : ta + sa[first + j];
        for (uint32_t x = lane; x < len; x += 64) bases[o + x] = src[x];
    }
}

// rec_start[r] = line_start[4 r], r = 0 .. n_rec: where every record begins, and where the text behind the last one does
__global__ void fq_record_starts_kernel(const uint64_t* __restrict__ line_start, uint64_t n_rec, uint64_t* __restrict__ rec_start) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n_rec; r += (uint64_t)gridDim.x * blockDim.x) rec_start[r] = line_start[4 * r];
}

// how a batch's record j reads its length (read_text.h batch_lens_kernel): from the index of its mate (pairs interleaved: mate 1, mate 2)
struct FqLen {
    const uint32_t *la, *lb;
    __device__ uint32_t operator()(uint64_t first, uint64_t j) const { return lb ? ((j & 1) ? lb[first + (j >> 1)] : la[first + (j >> 1)]) : la[first + j]; }
};

// the header of record r for the mate check (read_text.h mates_kernel): the '@' line behind its '@', up to the sequence line
struct FqHdr {
    const uint8_t* t;
    const uint64_t *hdr_start, *seq_start;
    __device__ const uint8_t* operator()(uint64_t r, uint64_t& n) const {
        const uint64_t s0 = hdr_start[r];
        n = seq_start[r] - s0 - 1;
        return t + s0 + 1;
    }
};

// What there is to index.  Whole: a whole text (sylph_fastq_index).  WholeWithStarts: the same, and where every record starts
// (sylph_fastq_index_window, final != 0).  Window: the COMPLETE records of a window of a text that goes on behind it (final == 0):
// nothing is trimmed, a line is one that ends in a newline inside the text, the records are the whole groups of four such lines, and
// *consumed is where the first line behind them starts.  With n_lines = 4 * n_rec + 1 the line kernel writes the starts of lines
// 0 .. 4 * n_rec — the last of them is `consumed`, and the end of the last record's quality line + 1, as between two records of a
// whole text.
enum class FqText { Whole, WholeWithStarts, Window };
const char* entry_of(FqText what) { return what == FqText::Window ? "sylph_fastq_index_window" : "sylph_fastq_index"; }

void fastq_index_impl(sylph_fastq* f, const void* text, uint64_t n_bytes, int mem, FqText what, uint64_t* consumed = nullptr) {
    sylph_ctx* ctx = f->ctx;
    const bool window = what == FqText::Window;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard dg(ctx->device);
    if (window && !n_bytes) return;                                        // no text yet: no records, nothing consumed
    const DeviceText t = take_text(ctx, f->text_own, &f->text, text, n_bytes, mem);
    const uint64_t n_tiles = t.n_tiles;
    SY_REQUIRE(n_tiles < (1ull << 31), "%s: text too large for one index (%llu bytes)", entry_of(what), (unsigned long long)n_bytes);
    DevBuf& b_words = ctx->scratch[0];
    DevBuf& b_cnt = ctx->scratch[1];
    DevBuf& b_base = ctx->scratch[2];
    DevBuf& b_lines = ctx->scratch[3];
    b_words.reserve(sizeof(FqWords));
    b_cnt.reserve((n_tiles + 1) * 4);
    b_base.reserve((n_tiles + 1) * 4);
    FqWords* d_w = b_words.as<FqWords>();
    FqWords hw{n_bytes, ~0ull, 0, 0, 0};
    if (window) ctx->h2d(d_w, &hw, sizeof(hw));                            // a window is not trimmed
    else hipLaunchKernelGGL(fq_trim_kernel, dim3(1), dim3(1), 0, ctx->stream, f->text, n_bytes, d_w);
    SY_HIP(hipMemsetAsync(b_cnt.as<uint32_t>() + n_tiles, 0, 4, ctx->stream));
    hipLaunchKernelGGL(fq_count_kernel, dim3((uint32_t)n_tiles), dim3(FQ_TPB), 0, ctx->stream, t.al, t.bias, d_w, b_cnt.as<uint32_t>());
    SY_HIP(hipGetLastError());
    exclusive_sum_u32(ctx, b_cnt.as<uint32_t>(), b_base.as<uint32_t>(), n_tiles + 1);
    uint32_t n_nl = 0;
    ctx->read_back(&n_nl, b_base.as<uint32_t>() + n_tiles, 4);     // (synchronises the stream)
    ctx->read_back(&hw, d_w, sizeof(hw));
    if (hw.flags & 1ull) throw FormatError{"more than 64 KiB of blank space behind the last line"};
    if (!window && hw.n_eff == 0) throw FormatError{"no text"};
    if (hw.n_nl != (unsigned long long)n_nl) throw FormatError{std::to_string(hw.n_nl) + " lines: at most 2^32 - 1 per index"};
    // the last line is unterminated: its newline was trimmed — or, of a window, it is not a whole line yet, nor are the up to three before it a record
    const uint64_t n_lines = window ? 4 * (uint64_t)(n_nl / 4) + 1 : (uint64_t)n_nl + 1;
    if (!window && n_lines % 4) throw FormatError{"the number of lines (" + std::to_string(n_lines) + ") is not a multiple of four"};
    f->n_rec = n_lines / 4;
    if (window && !f->n_rec) return;
    f->n = hw.n_eff;
    b_lines.reserve((n_lines + 1) * 8);
    f->seq_start.reserve(f->n_rec * 8);
    f->seq_len.reserve(f->n_rec * 4 + 4);
    f->hdr_start.reserve(f->n_rec * 8);
    hipLaunchKernelGGL(fq_lines_kernel, dim3((uint32_t)n_tiles), dim3(FQ_TPB), 0, ctx->stream, t.al, t.bias, d_w, b_base.as<uint32_t>(), n_lines,
                       b_lines.as<uint64_t>());
    hipLaunchKernelGGL(fq_records_kernel, dim3(grid1(f->n_rec, 256, 1u << 30)), dim3(256), 0, ctx->stream, f->text, b_lines.as<uint64_t>(), f->n_rec,
                       f->seq_start.as<uint64_t>(), f->seq_len.as<uint32_t>(), f->hdr_start.as<uint64_t>(), d_w);
    SY_HIP(hipGetLastError());
    ctx->read_back(&hw, d_w, sizeof(hw));
    if (hw.bad_rec != ~0ull) throw FormatError{"record " + std::to_string(hw.bad_rec) + " is not a four-line record ('@' line, sequence, '+' line, quality of the sequence's length)"};
    f->n_bases = hw.n_bases;
    if (window) {                                                          // the text ends, for this index, behind its last record
        unsigned long long end = 0;
        ctx->read_back(&end, b_lines.as<uint64_t>() + 4 * f->n_rec, 8);
        f->n = end;
    }
    if (consumed) *consumed = window ? f->n : n_bytes;
    if (what != FqText::Whole) {                                           // (a whole text's line_start[4 n_rec] = n + 1, the virtual newline's)
        f->rec_start.reserve((f->n_rec + 1) * 8);
        hipLaunchKernelGGL(fq_record_starts_kernel, dim3(grid1(f->n_rec + 1, 256, 4096)), dim3(256), 0, ctx->stream, b_lines.as<uint64_t>(), f->n_rec,
                           f->rec_start.as<uint64_t>());
        SY_HIP(hipGetLastError());
        f->has_starts = true;
    }
}

}  // namespace
}  // namespace sylph

using namespace sylph;

extern "C" {

int sylph_fastq_index(sylph_ctx* ctx, const void* text, uint64_t n_bytes, int mem, sylph_fastq** out) {
    if (!ctx || !out || (!text && n_bytes)) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    if (!mem_kind_ok(mem)) return SYLPH_ERR_INVALID;
    *out = nullptr;
    if (n_bytes == 0) { set_error("sylph_fastq_index: no text"); return SYLPH_ERR_FORMAT; }
    return make_index(ctx, "sylph_fastq_index", "not plain four-line FASTQ", out, [&](sylph_fastq* f) { fastq_index_impl(f, text, n_bytes, mem, FqText::Whole); });
}

int sylph_fastq_index_window(sylph_ctx* ctx, const void* text, uint64_t n_bytes, int mem, int final, sylph_fastq** out, uint64_t* consumed) {
    if (!ctx || !out || !consumed || (!text && n_bytes)) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    if (!mem_kind_ok(mem)) return SYLPH_ERR_INVALID;
    *out = nullptr;
    *consumed = 0;
    if (final && n_bytes == 0) { set_error("sylph_fastq_index: no text"); return SYLPH_ERR_FORMAT; }
    const FqText what = final ? FqText::WholeWithStarts : FqText::Window;    // final: sylph_fastq_index's code, + the records' starts
    const int rc = make_index(ctx, entry_of(what), "not plain four-line FASTQ", out, [&](sylph_fastq* f) { fastq_index_impl(f, text, n_bytes, mem, what, consumed); });
    if (rc != SYLPH_OK) *consumed = 0;
    return rc;
}

int sylph_fastq_record_offset(sylph_fastq* f, uint64_t record, uint64_t* offset) {
    return guarded([&] {
        SY_REQUIRE(f && offset, "null argument");
        SY_REQUIRE(f->has_starts || f->n_rec == 0, "sylph_fastq_record_offset: only an index made by sylph_fastq_index_window knows where its records start");
        SY_REQUIRE(record <= f->n_rec, "sylph_fastq_record_offset: record %llu of %llu", (unsigned long long)record, (unsigned long long)f->n_rec);
        if (!f->has_starts) { *offset = f->n; return; }
        std::lock_guard<std::mutex> lock(f->ctx->mu);
        DeviceGuard dg(f->ctx->device);
        unsigned long long v = 0;
        f->ctx->d2h(&v, f->rec_start.as<uint64_t>() + record, 8);
        *offset = v;
    });
}

int sylph_fastq_counts(const sylph_fastq* f, uint64_t* n_records, uint64_t* n_bases) {
    if (!f) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    if (n_records) *n_records = f->n_rec;
    if (n_bases) *n_bases = f->n_bases;
    return SYLPH_OK;
}

int sylph_fastq_lengths(sylph_fastq* f, uint64_t first, uint64_t n, uint32_t* out) {
    return guarded([&] {
        SY_REQUIRE(f && (out || n == 0), "null argument");
        SY_REQUIRE(first <= f->n_rec && n <= f->n_rec - first, "sylph_fastq_lengths: records [%llu, +%llu) of %llu", (unsigned long long)first,
                   (unsigned long long)n, (unsigned long long)f->n_rec);
        if (!n) return;
        std::lock_guard<std::mutex> lock(f->ctx->mu);
        DeviceGuard dg(f->ctx->device);
        f->ctx->d2h(out, f->seq_len.as<uint32_t>() + first, n * 4);
    });
}

void sylph_fastq_destroy(sylph_fastq* f) {
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

int sylph_sketch_push_fastq(sylph_sketch* sk, sylph_fastq* a, sylph_fastq* b, uint64_t first, uint64_t n_items) {
    if (!sk || !a) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    return push_read_text(
        "sylph_sketch_push_fastq", sk, a, b, first, n_items, FqLen{a->seq_len.as<uint32_t>(), b ? b->seq_len.as<uint32_t>() : nullptr},
        [] { return uint64_t(0); }, [] {},
        [&](const uint32_t* off, uint64_t n_rec_batch, uint64_t) {
            hipLaunchKernelGGL(fq_gather_kernel, dim3(grid1(n_rec_batch, 4, 1u << 16)), dim3(256), 0, sk->ctx->stream, a->text, a->seq_start.as<uint64_t>(),
                               b ? b->text : nullptr, b ? b->seq_start.as<uint64_t>() : nullptr, first, n_rec_batch, off, sk->fq_bases.as<uint8_t>());
        });
}

// The pairs of ONE interleaved text (interleave_plan.h: pair p = records 2 p and 2 p + 1) to a paired session: the batch is the
// records as they lie, which is the order a paired batch has — the single-end gather, fed record 2 first_pair + j
int sylph_sketch_push_fastq_interleaved(sylph_sketch* sk, sylph_fastq* f, uint64_t first_pair, uint64_t n_pairs) {
    if (!sk || !f) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    const char* entry = "sylph_sketch_push_fastq_interleaved";
    if (n_pairs >= (1ull << 30)) { set_error("%s: at most 2^31 - 1 records per push (%llu pairs)", entry, (unsigned long long)n_pairs); return SYLPH_ERR_INVALID; }
    const uint64_t pairs = interleave_plan::pairs_of(f->n_rec);
    if (first_pair > pairs || n_pairs > pairs - first_pair) {
        set_error("%s: pairs [%llu, +%llu) are not all there (%llu records)", entry, (unsigned long long)first_pair, (unsigned long long)n_pairs, (unsigned long long)f->n_rec);
        return SYLPH_ERR_INVALID;
    }
    const uint64_t first = interleave_plan::record_of(first_pair, 0);
    return push_read_text(
        entry, sk, f, (sylph_fastq*)nullptr, first, 2 * n_pairs, FqLen{f->seq_len.as<uint32_t>(), nullptr}, [] { return uint64_t(0); }, [] {},
        [&](const uint32_t* off, uint64_t n_rec_batch, uint64_t) {
            hipLaunchKernelGGL(fq_gather_kernel, dim3(grid1(n_rec_batch, 4, 1u << 16)), dim3(256), 0, sk->ctx->stream, f->text, f->seq_start.as<uint64_t>(),
                               (const uint8_t*)nullptr, (const uint64_t*)nullptr, first, n_rec_batch, off, sk->fq_bases.as<uint8_t>());
        },
        true);
}

int sylph_fastq_mates(sylph_fastq* f, uint64_t first_pair, uint64_t n_pairs, uint64_t* first_bad) {
    return index_mates("sylph_fastq_mates", f, first_pair, n_pairs, first_bad,
                       [&] { return FqHdr{f->text, f->hdr_start.as<uint64_t>(), f->seq_start.as<uint64_t>()}; });
}

}  // extern "C"
