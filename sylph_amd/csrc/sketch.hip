// sketch.hip — the read-sketch session on gfx950: what a push does with a batch, and what finish does with the occurrences.
//
//   push():   host batches travel in chunks of whole records (push_plan.h) on a copy stream; every chunk, and every device batch, is one
//             process_batch: the short-read kernel (reads.hip) or the position road (position_road.hip: K1 seeds -> survivors by flat
//             position -> K2 annotate) appends the batch's occurrences to the session in file order
//   finish(): K3, the replay of dup_removal_lsh_full_exact: per bucket in LDS (replay_lds.hip), else device-wide (replay_generic.hip)
//             -> (k-mer, count) table in ascending k-mer order; one loop over finish_plan.h decides what a late answer from the device undoes
#include <algorithm>

#include "common.h"
#include "device_common.h"
#include "position_road.h"
#include "push_plan.h"
#include "sketch_session.h"

namespace sylph {
namespace {

// flag[0] |= 1 when some record of the batch has a length that carries a dedup marker for single-end reads (66 .. 400 bases,
// sketch.rs:627,923)
__global__ __launch_bounds__(256) void marker_lengths_kernel(const uint64_t* __restrict__ off, uint64_t n_rec, uint32_t* __restrict__ flag) {
    bool any = false;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t L = off[r + 1] - off[r];
        any |= L >= 66 && L <= 400;
    }
    if (__ballot(any) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}
__global__ __launch_bounds__(256) void plain_records_kernel(const uint64_t* __restrict__ hash, uint64_t n, OccRec* __restrict__ recs) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) recs[i] = OccRec{hash[i], 0ull, 0ull, 0ull};
}

// sk->borrow_until_finish off for a process_batch whose batch does not outlive the call (a device slot of the host pipeline, a redo):
// nothing of it may be deferred to finish.  Restored on scope exit, also by an exception.
struct NoBorrow {
    sylph_sketch* sk;
    const bool was;
    explicit NoBorrow(sylph_sketch* s) : sk(s), was(s->borrow_until_finish) { sk->borrow_until_finish = false; }
    ~NoBorrow() { sk->borrow_until_finish = was; }
};

}  // namespace

// packed (SYLPH_ENC_2BIT) stream -> ASCII, for the batches the short-read kernel declines (long records, repeats everywhere)
__global__ __launch_bounds__(256) void unpack_2bit_kernel(const uint8_t* __restrict__ packed, uint32_t phase, uint64_t n_bases, uint8_t* __restrict__ ascii) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_bases; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t b = i + phase;
        const uint32_t code = (packed[b >> 2] >> (6u - 2u * (uint32_t)(b & 3))) & 3u;
        ascii[i] = (uint8_t)((0x54474341u >> (8u * code)) & 0xFFu);   // 'A','C','G','T'
    }
}
// off_out[i] = off_in[i] - off_in[0]: a chunk of a larger batch becomes a batch of its own
__global__ __launch_bounds__(256) void rebase_offsets_kernel(const uint64_t* __restrict__ in, uint64_t n, uint64_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] - in[0];
}

void materialise_plain_records(sylph_sketch* sk) {
    if (sk->n_plain == 0) return;
    sylph_ctx* ctx = sk->ctx;
    sk->recs.grow_keep(sk->n_occ * sizeof(OccRec), 0, ctx->stream);
    hipLaunchKernelGGL(plain_records_kernel, dim3(grid_for64(sk->n_plain)), dim3(256), 0, ctx->stream, sk->hash.as<uint64_t>(), sk->n_plain, sk->recs.as<OccRec>());
    SY_HIP(hipGetLastError());
    sk->n_plain = 0;
}

// One device-resident batch: records d_off[0..n_records] over the stream at d_bases (ASCII, or packed 2-bit starting
// `phase` bases into the first byte).  Appends the batch's occurrences to the session.
static void process_batch(sylph_sketch* sk, const uint8_t* d_bases, uint32_t phase, const uint64_t* d_off, uint64_t n_records, uint64_t n_bases, int enc) {
    sylph_ctx* ctx = sk->ctx;
    flush_pending_slots(sk);   // a further batch: the previous one's occurrences (still in their slots) go to the dense arrays first
    // short-read batches (mean record length <= 300): one lane per record, seeding + markers fused (reads.hip); it declines
    // (returns false) when some record is longer than its halo, and the position kernel + annotate below take over
    bool done = false;
    const bool short_batch = ctx->seeds_mode == 0 && n_bases < (1ull << 32) - 64 && n_records < (1ull << 31) && n_bases <= 300ull * n_records;
    // Marker-less batch?  Single-end only (a pair's mate-2 rule needs the record ids), everything so far marker-less too, and
    // either --no-dedup or no record of a length that carries a marker (asked of the offsets by a small kernel whose answer
    // comes back with the seeding kernel's count).
    bool plain = !short_batch && !sk->paired && sk->n_plain == sk->n_occ && ctx->plain_records;
    uint32_t* d_marked = sk->counters.as<uint32_t>() + CNT_MARKED;
    if (plain && !sk->no_dedup) {
        SY_HIP(hipMemsetAsync(d_marked, 0, 4, ctx->stream));
        if (n_records) {
            hipLaunchKernelGGL(marker_lengths_kernel, dim3((uint32_t)std::min<uint64_t>(1024, (n_records + 255) / 256)), dim3(256), 0, ctx->stream, d_off, n_records, d_marked);
            SY_HIP(hipGetLastError());   // a launch that failed would leave d_marked at 0: the batch would pass for marker-less
        }
    }
    if (!plain) materialise_plain_records(sk);
    if (short_batch) done = push_short_reads(sk, d_bases, phase, d_off, n_records, n_bases, enc);
    if (ctx->profile) ctx->stats[done ? "short_reads" : "position_road"].launches++;     // (tests ask sylph_ctx_kernel_stats which kernel took the batch)
    if (!done && enc == SYLPH_ENC_2BIT) {   // the position kernel and the marker loads of annotate read ASCII
        sk->batch_ascii.reserve(n_bases + 64);
        if (n_bases)
            hipLaunchKernelGGL(unpack_2bit_kernel, dim3((uint32_t)std::min<uint64_t>((n_bases + 255) / 256, 65536)), dim3(256), 0, ctx->stream,
                               d_bases, phase, n_bases, sk->batch_ascii.as<uint8_t>());
        SY_HIP(hipMemsetAsync(sk->batch_ascii.as<uint8_t>() + n_bases, 0, 64, ctx->stream));
        d_bases = sk->batch_ascii.as<uint8_t>();
    }
    uint32_t* d_count = sk->counters.as<uint32_t>() + CNT_SURVIVORS;
    // K1 loads 16 B per lane: start it at the aligned address below d_bases and subtract the bias afterwards (a device
    // pointer into the middle of a larger buffer, e.g. the second batch of a sample, need not be aligned)
    const uint32_t bias = (uint32_t)((uintptr_t)d_bases & 15);
    const PosSeeds seeds = done ? PosSeeds{nullptr, nullptr, 0} : seeds_sorted_by_pos(ctx, d_bases - bias, n_bases + bias, sk->c, sk->k, d_count);
    if (plain && !sk->no_dedup && !done) {
        uint32_t marked = 0;
        ctx->read_back(&marked, d_marked, 4);        // (the stream is idle: seeds_sorted_by_pos has read its count back)
        if (marked) { plain = false; materialise_plain_records(sk); }
    }
    if (seeds.n) {
        HostPhase ph(ctx, "push: grow + annotate");
        const uint64_t need = sk->n_occ + seeds.n;
        const size_t keep = sk->n_occ * 8;
        sk->hash.grow_keep(need * 8, keep, ctx->stream);
        if (!plain) sk->recs.grow_keep(need * sizeof(OccRec), sk->n_occ * sizeof(OccRec), ctx->stream);
        annotate_reads(sk, d_bases, d_off, n_records, n_bases, bias, seeds, plain);
        if (plain) sk->n_plain = need;
        sk->n_occ = need;
    }
    sk->rec_base += n_records;
    SY_REQUIRE(sk->rec_base <= RID_MASK, "more than 2^42 records in one sample");
}

// A deferred batch whose verdict came back bad (a record too long for the short-read kernel, a block that overflowed its slots):
// the session goes back to where it was before that push and the batch — its memory is still the caller's, that was the deal —
// runs through the checked push (which falls back to the position kernel / spill regions as needed).
void redo_deferred_batch(sylph_sketch* sk) {
    const PendingSlots d = sk->drop_pending_slots();
    sk->rec_base -= d.n_records;
    if (sk->ctx->profile) sk->ctx->stats["deferred_redo"].launches++;
    NoBorrow guard(sk);
    process_batch(sk, d.bases, d.phase, d.off, d.n_records, d.n_bases, d.enc);
}

// Host batches (SYLPH_MEM_HOST / SYLPH_MEM_HOST_PINNED) are cut into chunks of whole records (whole pairs) that travel on a
// COPY stream into two device slots while the compute stream works on the previous chunk: the PCIe transfer (1 B per base,
// or 1/4 B packed) is the long pole of a host-fed sample — 18 ms per Gbp against ~1 ms of kernels — and everything else
// hides under it.  Page-locked caller memory is DMA'd in place; pageable memory goes through the ctx's pinned staging pair.
static void push_host_batch(sylph_sketch* sk, const uint8_t* bases, const uint64_t* rec_off, uint64_t n_records, int mem, int enc) {
    sylph_ctx* ctx = sk->ctx;
    const bool pinned = mem == SYLPH_MEM_HOST_PINNED;
    const uint64_t bpb = enc == SYLPH_ENC_2BIT ? 4 : 1;                         // bases per byte
    if (!ctx->copy_stream) {
        SY_HIP(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) SY_HIP(hipEventCreateWithFlags(&ctx->copy_ev[i], hipEventDisableTiming));
    }
    if (!pinned) {   // make sure the staging pair exists (ctx->h2d creates it lazily)
        uint8_t dummy = 0;
        ctx->counters.reserve(64);
        ctx->h2d(ctx->counters.as<uint8_t>() + 32, &dummy, 1);
    }
    using push_plan::Chunk;
    static_assert(push_plan::STAGE_BYTES == sylph_ctx::STAGE_BYTES, "push_plan.h plans for the ctx's staging buffers");
    const push_plan::Limits lim = push_plan::chunk_limits(pinned, ctx->push_chunk_bytes);
    auto enqueue_copy = [&](const Chunk& c, int slot) {
        // device slot: [bases (from the byte that holds base b0) | pad] and [raw offsets r0..r1]
        const uint64_t nb = c.n_bytes(bpb), no = c.off_bytes();
        sk->slot_bases[slot].reserve(nb + 64);
        sk->slot_off[slot].reserve(no * 2);
        const uint8_t* src_b = bases + c.byte0(bpb);
        const uint64_t* src_o = rec_off + c.r0;
        if (!pinned && !c.fits_stage(bpb)) {                      // one record longer than a staging buffer: the plain staged copy
            SY_HIP(hipStreamSynchronize(ctx->copy_stream));       // (it reuses the staging pair: nothing of ours may still be in flight)
            ctx->h2d(sk->slot_bases[slot].p, src_b, nb);
            SY_HIP(hipMemsetAsync(sk->slot_bases[slot].as<uint8_t>() + nb, 0, 64, ctx->stream));
            ctx->h2d(sk->slot_off[slot].p, src_o, no);
            SY_HIP(hipEventRecord(ctx->copy_ev[slot], ctx->stream));
            return;
        }
        if (!pinned) {
            SY_HIP(hipEventSynchronize(ctx->stage_ev[slot]));                   // the previous copy out of this staging buffer finished
            uint8_t* stg = (uint8_t*)ctx->stage[slot];
            if (nb) memcpy(stg, src_b, nb);
            memcpy(stg + c.staged_off_at(bpb), src_o, no);
            src_b = stg;
            src_o = reinterpret_cast<const uint64_t*>(stg + c.staged_off_at(bpb));
        }
        if (nb) SY_HIP(hipMemcpyAsync(sk->slot_bases[slot].p, src_b, nb, hipMemcpyHostToDevice, ctx->copy_stream));
        SY_HIP(hipMemsetAsync(sk->slot_bases[slot].as<uint8_t>() + nb, 0, 64, ctx->copy_stream));
        SY_HIP(hipMemcpyAsync(sk->slot_off[slot].p, src_o, no, hipMemcpyHostToDevice, ctx->copy_stream));
        SY_HIP(hipEventRecord(ctx->copy_ev[slot], ctx->copy_stream));
        if (!pinned) SY_HIP(hipEventRecord(ctx->stage_ev[slot], ctx->copy_stream));
    };
    // the device slots may still be read by kernels of the previous push (spill redo, annotate): order the copy stream behind them
    SY_HIP(hipStreamSynchronize(ctx->stream));
    Chunk cur = push_plan::next_chunk(rec_off, n_records, 0, sk->paired, bpb, lim.max_bytes, lim.max_recs);
    enqueue_copy(cur, 0);
    for (int j = 0;; j++) {
        const int slot = j & 1;
        Chunk nxt{0, 0, 0, 0};
        const bool more = cur.r1 < n_records;
        if (more) {   // travels while this chunk is processed
            nxt = push_plan::next_chunk(rec_off, n_records, cur.r1, sk->paired, bpb, lim.max_bytes, lim.max_recs);
            enqueue_copy(nxt, slot ^ 1);
        }
        SY_HIP(hipStreamWaitEvent(ctx->stream, ctx->copy_ev[slot], 0));
        const uint64_t n_rec = cur.n_records();
        uint64_t* d_raw = sk->slot_off[slot].as<uint64_t>();
        uint64_t* d_off = d_raw + (n_rec + 1);
        hipLaunchKernelGGL(rebase_offsets_kernel, dim3(grid_for64(n_rec + 1)), dim3(256), 0, ctx->stream, d_raw, n_rec + 1, d_off);
        {   // (the device slots are overwritten by the copy after next: nothing here may be deferred to finish)
            NoBorrow guard(sk);
            process_batch(sk, sk->slot_bases[slot].as<uint8_t>(), cur.phase(bpb), d_off, n_rec, cur.n_bases(), enc);
        }
        // every kernel that reads this slot must be done before the copy after next overwrites it
        SY_HIP(hipStreamSynchronize(ctx->stream));
        if (!more) break;
        cur = nxt;
    }
}

static void sketch_push_impl(sylph_sketch* sk, const uint8_t* bases, const uint64_t* rec_off, uint64_t n_records, int mem,
                             const uint64_t* n_bases_hint = nullptr, int enc = SYLPH_ENC_ASCII) {
    SY_REQUIRE(sk, "null session");
    sylph_ctx* ctx = sk->ctx;
    SY_REQUIRE(!sk->finished, "sylph_sketch_push after finish");
    SY_REQUIRE(mem == SYLPH_MEM_HOST || mem == SYLPH_MEM_DEVICE || mem == SYLPH_MEM_HOST_PINNED, "bad mem kind %d", mem);
    SY_REQUIRE(enc == SYLPH_ENC_ASCII || enc == SYLPH_ENC_2BIT, "bad encoding %d", enc);
    SY_REQUIRE(!sk->paired || (n_records % 2 == 0), "paired batches must hold an even number of records");
    if (n_records == 0) return;
    SY_REQUIRE(rec_off, "null rec_off");
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard dg(ctx->device);
    HostPhase ph_total(ctx, "push: total");
    if (mem != SYLPH_MEM_DEVICE) {
        SY_REQUIRE(rec_off[0] == 0, "rec_off[0] must be 0");
        SY_REQUIRE(bases || rec_off[n_records] == 0, "null bases");
        SY_REQUIRE(!n_bases_hint || *n_bases_hint == rec_off[n_records], "n_bases does not match rec_off[n_records]");
        push_host_batch(sk, bases, rec_off, n_records, mem, enc);
        return;
    }
    uint64_t n_bases;
    if (n_bases_hint) n_bases = *n_bases_hint;
    else ctx->read_back(&n_bases, rec_off + n_records, 8);
    SY_REQUIRE(bases || n_bases == 0, "null bases");
    SY_REQUIRE(enc == SYLPH_ENC_ASCII || ((uintptr_t)bases & 3) == 0, "a packed device stream must be 4-byte aligned");
    process_batch(sk, bases, 0, rec_off, n_records, n_bases, enc);
}

static void sketch_finish_impl(sylph_sketch* sk) {
    if (sk->finished) return;
    sylph_ctx* ctx = sk->ctx;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard dg(ctx->device);
    HostPhase ph_total(ctx, "finish: total incl. readback");
    SY_REQUIRE(sk->n_occ + sk->pend.n < (1ull << 32) - 1, "more than 2^32-2 seed occurrences in one sample");
    sk->n_out = 0;
    sk->dup_removed = 0;
    if (!sk->pend.live && sk->n_occ == 0) { sk->finished = true; return; }   // nothing came: the empty table, at every c and in every mode
    // finish_plan.h says what comes next — the filter's marks (the reference's default dedup for pairs), an attempt at the fast path
    // (bucket partition + in-LDS replay, replay_lds.hip), what a bad answer from the device undoes, and at last the device-wide path —
    // from where the occurrences lie, what their records carry and the last answer; this loop does it and reports back.
    using finish_plan::Action;
    static_assert((int)finish_plan::Mode::Auto == 0 && (int)finish_plan::Mode::Generic == 1 && (int)finish_plan::Mode::Bucket == 2, "the ctx option \"finish\"");
    FinishOutcome last = FinishOutcome::None;
    for (;;) {
        const finish_plan::State st{sk->occurrences().place, sk->a10_marks, sk->n_plain != 0, sk->filter_dedup(), (finish_plan::Mode)ctx->finish_mode, sk->c < 2};
        switch (finish_plan::next(st, last)) {
        case Action::Mark: a10_mark(sk); break;
        case Action::Attempt:
            last = finish_bucketed(sk);
            if (last == FinishOutcome::Done) { sk->finished = true; return; }
            break;
        case Action::RedoDeferred: redo_deferred_batch(sk); break;
        case Action::RemarkWalk: a10_remark_walk(sk); break;
        case Action::WriteRecords: materialise_plain_records(sk); break;
        case Action::ReadSeedingVerdict: resolve_deferred_slots(sk); break;
        case Action::ReadFilterVerdict: {
            uint32_t words[2] = {0, 0};
            ctx->read_back(words, sk->a10_tail.p, 8);
            if (!a10_verdict(sk, words)) last = FinishOutcome::MarksBad;
            break;
        }
        case Action::Fail: SY_REQUIRE(false, "bucket finish overflowed and finish=bucket forbids the fallback"); break;
        case Action::Replay:
            flush_pending_slots(sk);   // the device-wide path works on the dense file-order arrays
            generic_replay(ctx, sk->hash.as<uint64_t>(), sk->recs.as<OccRec>(), (uint32_t)sk->n_occ, sk->paired, sk->dedup_mode(), sk->out_k, sk->out_c, sk->n_out, sk->dup_removed);
            sk->finished = true;
            return;
        }
    }
}

}  // namespace sylph

using namespace sylph;

extern "C" {

int sylph_sketch_begin(sylph_ctx* ctx, uint32_t c, uint32_t k, int reads_mode, int no_dedup, int seed_mode, sylph_sketch** out) {
    return guarded([&] {
        SY_REQUIRE(ctx && out, "null argument");
        SY_REQUIRE(c >= 1, "c must be >= 1");
        SY_REQUIRE(k == 21 || k == 31, "k must be 21 or 31 (avx2_seeding.rs:46-52)");
        SY_REQUIRE(reads_mode == SYLPH_READS_SINGLE || reads_mode == SYLPH_READS_PAIRED, "bad reads_mode %d", reads_mode);
        SY_REQUIRE(seed_mode == SYLPH_SEED_SCALAR || seed_mode == SYLPH_SEED_AVX2_COMPAT, "bad seed_mode %d", seed_mode);
        std::lock_guard<std::mutex> lock(ctx->mu);
        DeviceGuard dg(ctx->device);
        sylph_sketch* sk = new sylph_sketch(ctx);
        sk->c = c; sk->k = k;
        sk->paired = reads_mode == SYLPH_READS_PAIRED;
        sk->no_dedup = no_dedup != 0;
        sk->avx2_compat = seed_mode == SYLPH_SEED_AVX2_COMPAT;
        try {
            sk->counters.reserve(64);     // (every word of it is cleared by the path that uses it, right before: no memset dispatch per sample)
        } catch (...) { delete sk; throw; }
        ctx->refs++;
        *out = sk;
    });
}

int sylph_sketch_push(sylph_sketch* sk, const uint8_t* bases, const uint64_t* rec_off, uint64_t n_records, int mem) {
    return guarded([&] { sketch_push_impl(sk, bases, rec_off, n_records, mem); });
}

int sylph_sketch_push_n(sylph_sketch* sk, const uint8_t* bases, const uint64_t* rec_off, uint64_t n_records, uint64_t n_bases, int mem) {
    return guarded([&] { sketch_push_impl(sk, bases, rec_off, n_records, mem, &n_bases); });
}

int sylph_sketch_push_enc(sylph_sketch* sk, const uint8_t* bases, const uint64_t* rec_off, uint64_t n_records, uint64_t n_bases, int mem, int enc) {
    return guarded([&] { sketch_push_impl(sk, bases, rec_off, n_records, mem, &n_bases, enc); });
}

int sylph_sketch_finish_device(sylph_sketch* sk, const uint64_t** dev_kmers, const uint32_t** dev_counts, uint64_t* out_n,
                               uint64_t* out_dup_removed) {
    return guarded([&] {
        SY_REQUIRE(sk && dev_kmers && dev_counts && out_n, "null argument");
        sketch_finish_impl(sk);
        *dev_kmers = sk->out_k.as<uint64_t>();
        *dev_counts = sk->out_c.as<uint32_t>();
        *out_n = sk->n_out;
        if (out_dup_removed) *out_dup_removed = sk->dup_removed;
    });
}

int sylph_sketch_finish(sylph_sketch* sk, uint64_t** out_kmers, uint32_t** out_counts, uint64_t* out_n,
                        uint64_t* out_dup_removed) {
    return guarded([&] {
        SY_REQUIRE(sk && out_kmers && out_counts && out_n, "null argument");
        sketch_finish_impl(sk);
        const size_t n = sk->n_out;
        uint64_t* hk = (uint64_t*)malloc(std::max<size_t>(1, n) * 8);
        uint32_t* hc = (uint32_t*)malloc(std::max<size_t>(1, n) * 4);
        if (!hk || !hc) { free(hk); free(hc); throw std::bad_alloc(); }
        try {
            if (n) {
                std::lock_guard<std::mutex> lock(sk->ctx->mu);
                DeviceGuard dg(sk->ctx->device);
                sk->ctx->d2h(hk, sk->out_k.p, n * 8);
                sk->ctx->d2h(hc, sk->out_c.p, n * 4);
            }
        } catch (...) { free(hk); free(hc); throw; }
        *out_kmers = hk; *out_counts = hc; *out_n = n;
        if (out_dup_removed) *out_dup_removed = sk->dup_removed;
    });
}

int sylph_sketch_set_option(sylph_sketch* sk, const char* key, const char* value) {
    return guarded([&] {
        SY_REQUIRE(sk && key && value, "null argument");
        std::lock_guard<std::mutex> lock(sk->ctx->mu);
        if (!strcmp(key, "borrow_until_finish")) sk->borrow_until_finish = strtol(value, nullptr, 10) != 0;
        else if (!strcmp(key, "a10")) {             // A/B and test knob: which pass marks the filter's answers (a10.hip)
            if (!strcmp(value, "auto")) sk->a10_force = 0;
            else if (!strcmp(value, "walk")) sk->a10_force = 1;
            else if (!strcmp(value, "part")) sk->a10_force = 2;
            else SY_REQUIRE(false, "a10 must be auto|walk|part");
        }
        else if (!strcmp(key, "dedup_fpr") || !strcmp(key, "dedup_capacity")) {
            SY_REQUIRE_STATE(sk->rec_base == 0 && !sk->finished, "%s must be set before the first push", key);
            if (key[6] == 'f') {
                const double v = strtod(value, nullptr);
                SY_REQUIRE(v >= 0. && v < 1., "dedup_fpr must be in [0, 1) (got %s)", value);
                sk->dedup_fpr = v;
            } else {
                const long long v = strtoll(value, nullptr, 10);
                SY_REQUIRE(v >= 1 && v < (1ll << 31), "dedup_capacity must be in [1, 2^31) (got %s)", value);
                // the filter has the next power of two above capacity / 4 buckets of four entries: a capacity that fills them beyond 80 %
                // (8, 4096: 100 %) makes cuckoo insertions fail, and what a filter answers then depends on its eviction history — which
                // a10.hip does not replay (the reference's 10^7 fills 59.6 %; every doubling keeps the ratio)
                uint64_t nb = 1;
                while (nb * 4 < (uint64_t)v) nb <<= 1;
                SY_REQUIRE((double)v <= 0.8 * 4.0 * (double)nb, "dedup_capacity %lld would fill its %llu buckets to %.0f %%: insertions fail above ~80 %% and "
                           "the result would depend on the eviction order; choose a capacity further from a power of two", v, (unsigned long long)nb,
                           100.0 * (double)v / (4.0 * (double)nb));
                sk->dedup_capacity = (uint64_t)v;
            }
        }
        else SY_REQUIRE(false, "unknown session option %s", key);
    });
}

void sylph_sketch_destroy(sylph_sketch* sk) {
    if (!sk) return;
    sylph_ctx* ctx = sk->ctx;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        delete sk;   // buffers go back to the ctx pool; stream order protects in-flight work
    }
    ctx_unref(ctx);
}


}  // extern "C"
