// decode_host.h — the host scaffold of the two device decompressors (inflate.hip, bunzip2.hip): how a call enters and fails, how the
// compressed files reach the device, how the candidates come back, the buffer of the text a call returns, and what the two streams'
// handles and entries have in common.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "inflated.h"
#include "stream_plan.h"

namespace sylph {
namespace decode_host {

using stream_plan::Segments;

// thrown anywhere below an entry: the bytes are not what this road decodes (-> SYLPH_ERR_FORMAT, the caller decodes on the host)
struct FormatDecline { std::string msg; };

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// The body of sylph_inflate_files / sylph_bunzip2_files.  allow_null_empty: a file of no bytes may come with a null pointer.
// impl fills the handle (and takes the context's lock itself); whatever it throws, the stream is idle and the handle, its text
// and the reference on the context are given back before this returns.
using DecodeImpl = void (*)(sylph_inflated* t, const void* const* ptrs, const uint64_t* n_bytes, uint32_t n_files);
inline int decode_entry(const char* name, bool allow_null_empty, sylph_ctx* ctx, const void* const* ptrs, const uint64_t* n_bytes, uint32_t n_files, int mem,
                        sylph_inflated** out, DecodeImpl impl) {
    if (!ctx || !out || !ptrs || !n_bytes || !n_files) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    for (uint32_t i = 0; i < n_files; i++) if (!ptrs[i] && !(allow_null_empty && !n_bytes[i])) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    if (mem != SYLPH_MEM_HOST && mem != SYLPH_MEM_HOST_PINNED) { set_error("%s: the compressed bytes must lie in host memory (mem kind %d)", name, mem); return SYLPH_ERR_INVALID; }
    *out = nullptr;
    ctx->refs.fetch_add(1);
    sylph_inflated* t = nullptr;
    int format = 0;
    const int rc = guarded([&] {
        t = new sylph_inflated();
        t->ctx = ctx;
        try { impl(t, ptrs, n_bytes, n_files); }
        catch (const FormatDecline& e) { set_error("%s: declined: %s", name, e.msg.c_str()); format = 1; }
    });
    if (rc != SYLPH_OK || format) {
        {
            std::lock_guard<std::mutex> lock(ctx->mu);
            DeviceGuard dg(ctx->device);
            (void)hipStreamSynchronize(ctx->stream);
            if (t && t->buf) (void)hipFree(t->buf);
            delete t;
        }
        ctx_unref(ctx);
        return rc != SYLPH_OK ? rc : SYLPH_ERR_FORMAT;
    }
    *out = t;
    return SYLPH_OK;
}

// ---- the streams (sylph_inflate_stream_* / sylph_bunzip2_stream_*) -------------------------------------------------------------------
// What a stream of either format holds between two calls, beside its files' carries: where the window it handed out last lies (the
// caller keeps that alive for the next call: its kept tail is copied from there), and its counts.  The handles derive from it.
struct StreamBase {
    sylph_ctx* ctx = nullptr;
    std::vector<const uint8_t*> files;             // the compressed files (the caller's memory)
    std::vector<uint64_t> n_bytes;
    uint64_t slice_bytes = 0;
    std::vector<const uint8_t*> prev_text;         // file i's text in the window handed out last
    std::vector<uint64_t> prev_len;
    bool dead = false;
    uint64_t n_slices = 0, text_bytes = 0, peak_scratch = 0, peak_window = 0;
    StreamBase(sylph_ctx* c, const void* const* ptrs, const uint64_t* nb, uint32_t n_files, uint64_t slice)
        : ctx(c), n_bytes(nb, nb + n_files), slice_bytes(slice), prev_text(n_files, nullptr), prev_len(n_files, 0) {
        for (uint32_t i = 0; i < n_files; i++) files.push_back((const uint8_t*)ptrs[i]);
    }
    uint32_t n_files() const { return (uint32_t)files.size(); }
};

// the argument checks of <name>_open; the format check and the construction are the decoder's
template <class Stream>
int stream_open_args(const char* name, sylph_ctx* ctx, const void* const* ptrs, const uint64_t* n_bytes, uint32_t n_files, int mem, Stream** out) {
    if (!ctx || !out || !ptrs || !n_bytes || !n_files) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    for (uint32_t i = 0; i < n_files; i++) if (!ptrs[i]) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    if (mem != SYLPH_MEM_HOST && mem != SYLPH_MEM_HOST_PINNED) { set_error("%s_open: the compressed bytes must lie in host memory (mem kind %d)", name, mem); return SYLPH_ERR_INVALID; }
    *out = nullptr;
    return SYLPH_OK;
}

// The body of <name>_next.  impl fills the window's handle (and takes the context's lock itself); whatever it throws, the stream is
// given up (every later call is declined), the device stream is idle and the half-built window and the reference on the context
// are given back before this returns.  Stream: a StreamBase with the files' `carry`, whose entries say `finished`.
template <class Stream>
int stream_next_entry(const char* name, Stream* st, const uint8_t* advance, const uint64_t* keep_from, sylph_inflated** window, uint8_t* finished,
                      void (*impl)(Stream* st, sylph_inflated* t, const uint8_t* advance, const uint64_t* keep_from)) {
    if (!st || !window) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    *window = nullptr;
    if (st->dead) { set_error("%s_next: the stream was given up by an earlier call", name); return SYLPH_ERR_FORMAT; }
    sylph_ctx* ctx = st->ctx;
    ctx->refs.fetch_add(1);
    sylph_inflated* t = nullptr;
    int format = 0;
    const int rc = guarded([&] {
        t = new sylph_inflated();
        t->ctx = ctx;
        try { impl(st, t, advance, keep_from); }
        catch (const FormatDecline& e) { set_error("%s_next: declined: %s", name, e.msg.c_str()); format = 1; }
    });
    if (rc != SYLPH_OK || format) {
        st->dead = true;
        {
            std::lock_guard<std::mutex> lock(ctx->mu);
            DeviceGuard dg(ctx->device);
            (void)hipStreamSynchronize(ctx->stream);
            if (t && t->buf) (void)hipFree(t->buf);
            delete t;
        }
        ctx_unref(ctx);
        return rc != SYLPH_OK ? rc : SYLPH_ERR_FORMAT;
    }
    if (finished) for (size_t i = 0; i < st->carry.size(); i++) finished[i] = st->carry[i].finished ? 1 : 0;
    *window = t;
    return SYLPH_OK;
}

inline int stream_info(const StreamBase* st, uint64_t* n_slices, uint64_t* text_bytes, uint64_t* peak_scratch_bytes, uint64_t* peak_window_bytes) {
    if (!st) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    if (n_slices) *n_slices = st->n_slices;
    if (text_bytes) *text_bytes = st->text_bytes;
    if (peak_scratch_bytes) *peak_scratch_bytes = st->peak_scratch;
    if (peak_window_bytes) *peak_window_bytes = st->peak_window;
    return SYLPH_OK;
}

// free_extra(st): the device memory that is the decoder's own, under the context's lock and with the stream idle
template <class Stream, class FreeExtra>
void stream_destroy(Stream* st, FreeExtra free_extra) {
    if (!st) return;
    sylph_ctx* ctx = st->ctx;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        DeviceGuard dg(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        free_extra(st);
        delete st;
    }
    ctx_unref(ctx);
}

// a file's slice begins at a multiple of this in a call's upload (zero bytes between the slices)
constexpr uint64_t SLICE_ALIGN = 256;
inline uint64_t slice_begin(uint64_t at) { return (at + SLICE_ALIGN - 1) / SLICE_ALIGN * SLICE_ALIGN; }

// per file: the bytes of its previous window that the caller keeps (from keep_from[f] to that window's end; null: none)
inline std::vector<uint64_t> kept_tails(const StreamBase* st, const uint64_t* keep_from, const char* name) {
    std::vector<uint64_t> kept(st->n_files(), 0);
    for (uint32_t f = 0; keep_from && f < st->n_files(); f++) {
        SY_REQUIRE(keep_from[f] <= st->prev_len[f], "%s_next: keep_from[%u] = %llu lies behind the previous window (%llu bytes)", name, f,
                   (unsigned long long)keep_from[f], (unsigned long long)st->prev_len[f]);
        kept[f] = st->prev_len[f] - keep_from[f];
    }
    return kept;
}

// where the window in t lies, file by file (text_off: n_files + 1 offsets into its text), for the next call's kept tails
inline void remember_window(StreamBase* st, const sylph_inflated* t, const std::vector<uint64_t>& text_off) {
    for (uint32_t f = 0; f < st->n_files(); f++) { st->prev_text[f] = t->text() + text_off[f]; st->prev_len[f] = text_off[f + 1] - text_off[f]; }
}

inline Segments segments_of(const void* const* ptrs, const uint64_t* n_bytes, uint32_t n_files) {
    Segments S;
    S.base.push_back(0);
    for (uint32_t i = 0; i < n_files; i++) {
        S.ptr.push_back((const uint8_t*)ptrs[i]);
        S.base.push_back(S.base.back() + n_bytes[i]);
    }
    return S;
}

// the files back to back at dst, zero from the end of the last one to pad_bytes behind the last whole word (the kernels read words)
inline void upload_segments(sylph_ctx* ctx, uint8_t* dst, const Segments& S, uint64_t pad_bytes) {
    const uint64_t n = S.total(), whole = n & ~(uint64_t)3;
    SY_HIP(hipMemsetAsync(dst + whole, 0, (n + 3) / 4 * 4 + pad_bytes - whole, ctx->stream));
    for (size_t i = 0; i + 1 < S.base.size(); i++)
        if (S.base[i + 1] != S.base[i]) ctx->h2d(dst + S.base[i], S.ptr[i], (size_t)(S.base[i + 1] - S.base[i]));
}

// what a scan found: the count it left at d_count (declined above cap, with `why`), then the candidates' bits, sorted
template <class Count>
std::vector<uint64_t> fetch_candidates(sylph_ctx* ctx, const void* d_cand, const Count* d_count, uint64_t cap, const char* why) {
    Count n = 0;
    ctx->read_back(&n, d_count, sizeof(Count));
    if (n > cap) throw FormatDecline{why};
    std::vector<uint64_t> cand(n);
    if (n) ctx->d2h(cand.data(), d_cand, (size_t)n * 8);
    std::sort(cand.begin(), cand.end());
    return cand;
}

// The text a call returns (sylph_inflated::buf): 256 zero bytes, the text, 256 zero bytes.  Grows (copying) as blocks come in; the
// caller zeroes the 256 bytes behind the text once its length is final, and takes p.
struct TextBuf {
    const char* what;                              // names the allocation in a HIP error
    void* p = nullptr;
    size_t cap = 0;                                // bytes of text it holds (+512 of padding)
    explicit TextBuf(const char* w) : what(w) {}
    TextBuf(const TextBuf&) = delete;
    ~TextBuf() { if (p) (void)hipFree(p); }         // (a declined call)
    uint8_t* text() const { return (uint8_t*)p + 256; }
    void grow(size_t need, size_t used, hipStream_t s) {
        if (p && need <= cap) return;
        const size_t c = std::max(need, cap * 2);
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, c + 512);
        if (e != hipSuccess) { (void)hipGetLastError(); throw HipError{e, what, __FILE__, __LINE__}; }
        SY_HIP(hipMemsetAsync(q, 0, 256, s));
        if (p && used) SY_HIP(hipMemcpyAsync((uint8_t*)q + 256, (uint8_t*)p + 256, used, hipMemcpyDeviceToDevice, s));
        if (p) { SY_HIP(hipStreamSynchronize(s)); (void)hipFree(p); }
        p = q;
        cap = c;
    }
    void* release() { void* q = p; p = nullptr; return q; }
};

}  // namespace decode_host
}  // namespace sylph
