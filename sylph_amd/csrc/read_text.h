// read_text.h — what fastq.hip and fasta.hip share on the host side of the library: a text taken into device memory, the scaffold of a
// C entry that makes an index, and the push of a batch of an index's records into a sketch session.  Each including translation unit
// gets its own copy, as with text_lines.h.
#pragma once
#include <algorithm>
#include <string>

#include "common.h"
#include "device_common.h"
#include "sketch_session.h"
#include "text_lines.h"
#include "interleave_plan.h"

namespace sylph {
namespace {

// the text is not what the index takes: the C entry answers SYLPH_ERR_FORMAT and the caller reads the file with its host reader
struct FormatError { std::string msg; };

inline uint32_t grid1(uint64_t n, uint32_t tpb, uint32_t cap) { return (uint32_t)std::min<uint64_t>(cap, std::max<uint64_t>(1, (n + tpb - 1) / tpb)); }

// A text in device memory as text_lines.h's kernels read it: the aligned stream `al` (text = al + bias) and its 4 KiB tiles.
struct DeviceText { const uint8_t* al; uint32_t bias; uint64_t n_tiles; };

// *dev = the text's byte 0 on the device: `text` itself (SYLPH_MEM_DEVICE: borrowed), else a copy in `own`, queued on the context's
// stream.  The caller holds the context's lock.
inline DeviceText take_text(sylph_ctx* ctx, DevBuf& own, const uint8_t** dev, const void* text, uint64_t n_bytes, int mem) {
    if (mem == SYLPH_MEM_DEVICE) {
        *dev = (const uint8_t*)text;
    } else {
        own.reserve(n_bytes + 64);
        if (mem == SYLPH_MEM_HOST_PINNED) SY_HIP(hipMemcpyAsync(own.p, text, n_bytes, hipMemcpyHostToDevice, ctx->stream));
        else ctx->h2d(own.p, text, n_bytes);
        *dev = own.as<uint8_t>();
    }
    const uint32_t bias = (uint32_t)((uintptr_t)*dev & 15);
    return DeviceText{*dev - bias, bias, (n_bytes + bias + FQ_TILE - 1) / FQ_TILE};
}

inline bool mem_kind_ok(int mem) {
    if (mem == SYLPH_MEM_HOST || mem == SYLPH_MEM_DEVICE || mem == SYLPH_MEM_HOST_PINNED) return true;
    set_error("bad mem kind %d", mem);
    return false;
}

// The scaffold of a C entry that makes an index (the arguments are checked by the entry): the index holds a reference of its context,
// body(index) builds it, a FormatError of the body is `entry: not_what: its message` and SYLPH_ERR_FORMAT.  A build that fails may have
// queued kernels that write the half-built index's buffers: the stream is synchronised before they go.
template <class Index, class Body>
int make_index(sylph_ctx* ctx, const char* entry, const char* not_what, Index** out, Body&& body) {
    ctx->refs.fetch_add(1);
    Index* f = nullptr;
    int format = 0;
    const int rc = guarded([&] {
        f = new Index(ctx);
        try { body(f); }
        catch (const FormatError& e) { set_error("%s: %s: %s", entry, not_what, e.msg.c_str()); format = 1; }
    });
    if (rc != SYLPH_OK || format) {
        if (f) { std::lock_guard<std::mutex> lock(ctx->mu); DeviceGuard dg(ctx->device); (void)hipStreamSynchronize(ctx->stream); delete f; }
        ctx_unref(ctx);
        return rc != SYLPH_OK ? rc : SYLPH_ERR_FORMAT;
    }
    *out = f;
    return SYLPH_OK;
}

// lengths of a batch's records in batch order (pairs interleaved), one sentinel 0 behind them for the scan; their 64-bit sum in *total
// (the scan is a 32-bit one: the caller checks the sum before it trusts the offsets).  len(first, j): the length of the batch's record j
template <class Len>
__global__ void batch_lens_kernel(Len len, uint64_t first, uint64_t n_rec_batch, uint32_t* __restrict__ out, unsigned long long* __restrict__ total) {
    unsigned long long sum = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= n_rec_batch; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = j == n_rec_batch ? 0u : len(first, j);
        out[j] = l;
        sum += l;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(total, sum);
}
__global__ void widen_kernel(const uint32_t* __restrict__ in, uint64_t n, uint64_t* __restrict__ out) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) out[j] = in[j];
}

// The mate check of an interleaved file (interleave_plan.h): pairs [first_pair, first_pair + n_pairs) of ONE index, pair p = records
// 2 p and 2 p + 1; *first_bad (preset to n_pairs) = the smallest pair of the range, counted from first_pair, whose records are not
// mates.  A wavefront takes 64 / GROUP_LANES pairs at a time, a group of lanes each; a group walks its two headers GROUP_LANES bytes
// per step, lane l reading byte base + l of each — one coalesced read per header and step — and votes the plan's four masks.  The
// step loop is wavefront-uniform: every lane of the wavefront runs every step and every vote until all its groups are done (a group
// that is done, or has no pair, reads nothing more: its headers count as 0 bytes long from then on).
//   hdr(record, &n)   device functor: the record's header behind its '@' / '>', n = its bytes (a line end among them is fine)
template <class Hdr>
__global__ __launch_bounds__(256) void mates_kernel(Hdr hdr, uint64_t first_pair, uint64_t n_pairs, unsigned long long* __restrict__ first_bad) {
    namespace ip = interleave_plan;
    static_assert(ip::GROUP_LANES == 32, "a group's votes are one half of a 64-lane ballot");
    constexpr uint32_t WAVE_PAIRS = 64 / ip::GROUP_LANES;
    const uint32_t lane = threadIdx.x & 63, group = lane / ip::GROUP_LANES, gl = lane % ip::GROUP_LANES;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t p0 = wave * WAVE_PAIRS; p0 < n_pairs; p0 += waves * WAVE_PAIRS) {        // (p0 is the same in all lanes of a wavefront)
        const uint64_t p = p0 + group;
        const bool has_pair = p < n_pairs;
        const uint8_t *ha = nullptr, *hb = nullptr;
        uint32_t na = 0, nb = 0;
        if (has_pair) {
            uint64_t n = 0;
            ha = hdr(ip::record_of(first_pair + p, 0), n);
            na = ip::header_bytes(n);
            hb = hdr(ip::record_of(first_pair + p, 1), n);
            nb = ip::header_bytes(n);
        }
        ip::MateScan s;
        uint32_t carry = 0;                                              // header a's byte in front of this step's first
        for (uint32_t base = 0;; base += ip::GROUP_LANES) {
            const bool live = !s.done();
            const uint32_t x = base + gl;
            const uint32_t ca = live ? ip::byte_at(ha, na, x) : (uint32_t)' ', cb = live ? ip::byte_at(hb, nb, x) : (uint32_t)' ';
            const uint32_t up = (uint32_t)__shfl_up((int)ca, 1, ip::GROUP_LANES);
            const uint32_t front = gl ? up : carry;
            const uint32_t shift = group * ip::GROUP_LANES;
            const uint32_t end_a = (uint32_t)(__ballot(ip::is_id_end((uint8_t)ca)) >> shift);
            const uint32_t end_b = (uint32_t)(__ballot(ip::is_id_end((uint8_t)cb)) >> shift);
            const uint32_t differ = (uint32_t)(__ballot(ca != cb) >> shift);
            const uint32_t slash12 = (uint32_t)(__ballot(ip::lane_slash12((uint8_t)ca, (uint8_t)cb, (uint8_t)front, x)) >> shift);
            carry = (uint32_t)__shfl((int)ca, ip::GROUP_LANES - 1, ip::GROUP_LANES);
            if (live) s.step(base, end_a, end_b, differ, slash12);
            if (!__any(!s.done())) break;
        }
        if (has_pair && gl == 0 && !s.verdict()) atomicMin(first_bad, (unsigned long long)p);
    }
}
// the launch and its answer; the caller holds the context's lock.  -> the first pair of the range (from 0) that fails, n_pairs: none
template <class Hdr>
uint64_t first_bad_pair(sylph_ctx* ctx, Hdr hdr, uint64_t first_pair, uint64_t n_pairs) {
    if (!n_pairs) return 0;
    ctx->counters.reserve(64);
    unsigned long long v = n_pairs;
    ctx->h2d(ctx->counters.p, &v, 8);
    {
        ScopedKernelTimer t(ctx, "mate_check");
        hipLaunchKernelGGL(mates_kernel<Hdr>, dim3(grid1(n_pairs, 256 / interleave_plan::GROUP_LANES, 1u << 16)), dim3(256), 0, ctx->stream, hdr,
                           first_pair, n_pairs, ctx->counters.as<unsigned long long>());
        SY_HIP(hipGetLastError());
    }
    ctx->read_back(&v, ctx->counters.p, 8);
    return v;
}
// the scaffold of sylph_fastq_mates / sylph_fasta_mates: the range is checked against the index's records, then first_bad_pair
template <class Index, class Hdr>
int index_mates(const char* entry, Index* f, uint64_t first_pair, uint64_t n_pairs, uint64_t* first_bad, Hdr&& make_hdr) {
    return guarded([&] {
        SY_REQUIRE(f && first_bad, "null argument");
        const uint64_t pairs = interleave_plan::pairs_of(f->n_rec);
        SY_REQUIRE(first_pair <= pairs && n_pairs <= pairs - first_pair, "%s: pairs [%llu, +%llu) of %llu (records 2 p and 2 p + 1 of %llu)", entry,
                   (unsigned long long)first_pair, (unsigned long long)n_pairs, (unsigned long long)pairs, (unsigned long long)f->n_rec);
        *first_bad = n_pairs;
        if (!n_pairs) return;
        std::lock_guard<std::mutex> lock(f->ctx->mu);
        DeviceGuard dg(f->ctx->device);
        *first_bad = first_bad_pair(f->ctx, make_hdr(), first_pair, n_pairs);
    });
}

// Records [first, first + n_items) of index a (pairs: of a and b, interleaved) as one batch of the session: their 32-bit offsets are
// cut, the total and the room are checked, the session's batch buffers are reserved, the offsets widened, the caller gathers the
// bases, and the batch goes to sylph_sketch_push_enc (SYLPH_MEM_DEVICE, SYLPH_ENC_ASCII).
//   entry         the C entry's name, for the messages
//   len           device functor: len(first, j) = length of the batch's record j
//   to_prepare()  bytes that must be free besides the batch's own, for what prepare() reserves
//   prepare()     runs behind the room check and before the session's buffers are touched
//   gather(off, n_rec_batch, n_bases)   launches the kernel that writes the bases to sk->fq_bases; off: the batch's 32-bit offsets
//   interleaved   the records are those of ONE interleaved file (b == nullptr) and go to a PAIRED session as they lie: first and
//                 n_items count RECORDS, both even (the *_interleaved entries hand over 2 first_pair and 2 n_pairs)
template <class Index, class Len, class ToPrepare, class Prepare, class Gather>
int push_read_text(const char* entry, sylph_sketch* sk, Index* a, Index* b, uint64_t first, uint64_t n_items, Len len, ToPrepare&& to_prepare,
                   Prepare&& prepare, Gather&& gather, bool interleaved = false) {
    uint64_t n_rec_batch = 0, n_bases = 0;
    const std::string no_room = std::string(entry) + ": no room for the batch";
    const int rc = guarded([&] {
        sylph_ctx* ctx = sk->ctx;
        SY_REQUIRE(a->ctx == ctx && (!b || b->ctx == ctx), "%s: the index lives on another context than the session", entry);
        if (interleaved) SY_REQUIRE(sk->paired != 0 && !b, "%s: the pairs of an interleaved text go to a paired session", entry);
        else SY_REQUIRE((b != nullptr) == (sk->paired != 0), "%s: a paired session takes two texts, a single-end session one", entry);
        SY_REQUIRE(first <= a->n_rec && n_items <= a->n_rec - first && (!b || (first <= b->n_rec && n_items <= b->n_rec - first)),
                   "%s: records [%llu, +%llu) are not all there", entry, (unsigned long long)first, (unsigned long long)n_items);
        if (!n_items) return;
        n_rec_batch = b ? 2 * n_items : n_items;
        SY_REQUIRE(n_rec_batch < (1ull << 31), "%s: at most 2^31 - 1 records per push", entry);
        std::lock_guard<std::mutex> lock(ctx->mu);
        DeviceGuard dg(ctx->device);
        // a deferred batch of this session reads sk->fq_bases until its verdict is in: settle it before the buffer is written again
        resolve_deferred_slots(sk);
        DevBuf& b_len = ctx->scratch[0];
        DevBuf& b_off = ctx->scratch[1];
        DevBuf& b_tot = ctx->scratch[2];
        b_len.reserve((n_rec_batch + 1) * 4);
        b_off.reserve((n_rec_batch + 1) * 4);
        b_tot.reserve(8);
        SY_HIP(hipMemsetAsync(b_tot.p, 0, 8, ctx->stream));
        hipLaunchKernelGGL(batch_lens_kernel<Len>, dim3(grid1(n_rec_batch + 1, 256, 4096)), dim3(256), 0, ctx->stream, len, first, n_rec_batch,
                           b_len.as<uint32_t>(), b_tot.as<unsigned long long>());
        SY_HIP(hipGetLastError());
        exclusive_sum_u32(ctx, b_len.as<uint32_t>(), b_off.as<uint32_t>(), n_rec_batch + 1);
        unsigned long long total = 0;
        ctx->read_back(&total, b_tot.p, 8);
        SY_REQUIRE(total < (1ull << 32) - 64, "%s: %llu bases in one push (at most 2^32 - 65: push fewer records at a time)", entry, total);
        n_bases = total;
        // no room for the gathered batch and its seeding, or for what is still to prepare?  Say so BEFORE anything of the session is
        // touched (round 6): the caller pushes fewer records at a time, or takes its host feed, which works through a sample
        // in 256 Mbp batches
        const uint64_t extra = to_prepare();
        const bool grows = n_bases + 64 > sk->fq_bases.cap;
        if (grows || extra) {
            size_t free_b = 0, total_b = 0;
            size_t pooled = 0;                                  // blocks the context's pool holds and hands out again
            for (const auto& blk : ctx->pool_free) pooled += blk.first;
            const uint64_t batch_need = grows ? n_bases + n_bases / 2 + (256u << 20) : 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b + pooled < batch_need + extra + extra / 4)
                throw HipError{hipErrorOutOfMemory, no_room.c_str(), __FILE__, __LINE__};
        }
        prepare();
        sk->fq_bases.reserve(n_bases + 64);
        sk->fq_off.reserve((n_rec_batch + 1) * 8);
        hipLaunchKernelGGL(widen_kernel, dim3(grid1(n_rec_batch + 1, 256, 4096)), dim3(256), 0, ctx->stream, b_off.as<uint32_t>(), n_rec_batch + 1,
                           sk->fq_off.as<uint64_t>());
        gather(b_off.as<uint32_t>(), n_rec_batch, n_bases);
        SY_HIP(hipMemsetAsync(sk->fq_bases.as<uint8_t>() + n_bases, 0, 64, ctx->stream));
        SY_HIP(hipGetLastError());
    });
    if (rc != SYLPH_OK || !n_rec_batch) return rc;
    return sylph_sketch_push_enc(sk, sk->fq_bases.as<uint8_t>(), sk->fq_off.as<uint64_t>(), n_rec_batch, n_bases, SYLPH_MEM_DEVICE, SYLPH_ENC_ASCII);
}

}  // namespace
}  // namespace sylph
