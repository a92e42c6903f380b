// reads.hip — seeding + per-read bookkeeping fused for SHORT-READ batches (every record <= READ_HALO = 400 bases): one lane
// per RECORD instead of one lane per 64 flat positions (seeds.hip), so that
//   * only the k-mers the reference hashes are hashed — the position kernel also hashes the k-1 positions per read whose
//     k-mer crosses a record boundary (20 % of a 150 bp read) and throws them away later;
//   * the record, the validity rule (avx2_seeding.rs:37-44) and the dedup markers (pair_kmer / pair_kmer_single,
//     sketch.rs:625-688) are known right here, from the packed bases already in LDS: the separate annotate kernel with its
//     scattered marker loads disappears, and the occurrences leave this kernel as finished 32 B records in file order.
// Replaces extract_markers + the marker half of the record loops (sketch.rs:897-959, :771-895) for Illumina-like input;
// long reads and genomes keep the position kernel (boundary waste there is k/L < 1 %).
//
// A workgroup owns the records whose start falls into a block of `rt` (16 B-aligned) base coordinates — rt is chosen by the
// host so that a block holds about 256 records — and loads that block plus a halo of READ_HALO bases on both sides (the end of its last record; mate 1 of a mate 2 that starts the block)
// as a 2-bit big-endian stream F (input may already BE 2-bit: SYLPH_ENC_2BIT, a quarter of the PCIe bytes).  Each lane then
// walks ITS record with no rolling state at all: it keeps three lane-aligned stream words A(g..g+2) (16 bases each, refilled
// from LDS once per 16 k-mers) and their reverse-complement images B = ~pairswap(bitreverse(A)); the forward k-mer t of the
// group and its reverse complement are funnel-shift and bit-field extracts (v_alignbit_b32, v_bfe_u32) of those registers at
// COMPILE-TIME shifts, both right-aligned in 64 bits with clean tops, and the smaller of the two is ONE v_min_f64 (kmer_step):
// 6 instructions per k-mer for both windows and the canonical choice, then the same hash / threshold sequences as the
// position kernel.
// Hits are accumulated as bit masks (one bit per k-mer, 32 k-mers per LDS word; the 256-lane instances set the bit with an LDS xor under
// the threshold compare's own lane mask instead of transposing it on the VALU: reads_block.h kmer_step), counted, scanned across the workgroup —
// lanes are in record order, so the scan gives file order — and only then re-hashed and written.
#include <cstddef>

#include "common.h"
#include "device_common.h"
#include "reads_block.h"
#include "seed_plan.h"
#include "sketch_session.h"

namespace sylph {

namespace {

// blk_rec[b] = first record whose aligned start coordinate (off + bias) is >= b * rt, for b in [0, n_blk]
// (also clears the words the short-read kernel accumulates into: the scan sentinel behind the block counts and the
//  long-record / overflow flags — two memset dispatches less per batch)
__global__ __launch_bounds__(256) void block_records_kernel(const uint64_t* __restrict__ off, uint64_t n_rec, uint32_t bias,
                                                            uint32_t rt, uint32_t n_entries, uint32_t* __restrict__ blk_rec,
                                                            uint32_t* __restrict__ count_sentinel, uint32_t* __restrict__ state_words) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) { *count_sentinel = 0; state_words[0] = 0; state_words[1] = 0; }
    if (b >= n_entries) return;
    blk_rec[b] = (uint32_t)first_record_of_block(off, n_rec, bias, b, rt);
}

#ifndef SYLPH_READS_HASH_DEFAULT
#define SYLPH_READS_HASH_DEFAULT 1
#endif
#ifndef SYLPH_READS_WAVES
#define SYLPH_READS_WAVES 5
#endif
// Which instances set their hit bits by LDS atomics (reads_block.h kmer_step, LB): the 256-lane ones.  The 512-lane A/B variant keeps
// v_cmp + v_addc_co_u32: 17 more registers do not fit its budget of 80 for six waves per SIMD (profiles/r14_hit_bits_lds.md).
template <int TPB>
constexpr bool hit_bits_by_lds = TPB == RTPB;
template <int K, int HV, int ENC, int TPB>
// (512 lanes are two wavefronts per SIMD and workgroup: three workgroups = six per SIMD — five would leave room for two)
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(TPB == 256 ? SYLPH_READS_WAVES : 6, TPB == 256 ? SYLPH_READS_WAVES : 6))) void reads_kernel(const uint8_t* __restrict__ bases_al, uint32_t bias, uint64_t n_al,
                                                     const uint64_t* __restrict__ off, uint64_t n_rec,
                                                     const uint32_t* __restrict__ blk_rec, uint32_t n_blk, uint32_t it_begin, uint32_t it_end,
                                                     uint32_t rt, uint64_t thr,
                                                     uint32_t cand_slack, int avx2_compat, int paired, int want_markers, uint64_t rec_base,
                                                     uint32_t slot_cap, OccRec* __restrict__ slot_rec,
                                                     uint32_t* __restrict__ slot_key, int key_sh,
                                                     uint32_t* __restrict__ blk_count,
                                                     ReadsState* __restrict__ state, const uint32_t* __restrict__ blk_list,
                                                     uint32_t* __restrict__ spill_slot_of_blk) {
    // TPB = RTPB (256: one record per lane, a block of ~256 records); RTPB_RAGGED (512) is an A/B variant for ragged input (round 6): the
    // pass's records are dealt to the lanes by length, so a wavefront pays for the longest record of ITS share — a quarter of 256 records,
    // an eighth of 512: trimmed reads of 35..151 bp would idle 11 % of their hash loop's lane-steps instead of 23 %.  Measured slower (see
    // seed_plan.h reads_block_plan): not the default.
    const ReadsLds<TPB> s = reads_lds<TPB>();
    const uint32_t tid = threadIdx.x;
    // HV == 2: the loop tests hi(h) only (kmer_step) and yields a SUPERSET of the k-mers below the threshold — about 3 in 2^32 k-mers
    // too many; finish_survivors, which hashes every candidate exactly anyway, strikes those from the hit masks and the pass's
    // bookkeeping is redone once (s.redo).  cand_slack widens the superset on purpose: the tests' way of making that road common.
    const uint64_t thr_loop = HV == 2 ? (uint64_t)((uint32_t)(thr >> 32) + 1u + cand_slack) : thr;
    if (tid == 0) *s.redo = 0;                                       // (ordered before its first reader by the barriers below)
    const HitRegs hit = hit_bits_by_lds<TPB> ? hit_regs() : HitRegs{};
    // Workgroups are dealt round-robin to the 8 XCDs (each with its own L2): give every XCD one contiguous eighth of the
    // blocks (xcd_deal_share), so that the halo a block shares with its neighbour is found in the same L2.  (Outputs are indexed by block,
    // so the order of the results does not depend on this mapping.)
    // (a launch covers the positions [it_begin, it_end) of that dealing: the pipeline launches a sample's last positions separately, see
    //  push_short_reads)
    const uint32_t n_words = stream_words(rt), per_xcd = xcd_share(n_blk);      // (uniform: computed once, as scalars)
    for (uint32_t it0 = it_begin + blockIdx.x; it0 < it_end; it0 += gridDim.x) {
        const uint32_t it = blk_list ? it0 : xcd_deal_share(it0, per_xcd);
        if (it >= n_blk) continue;                                   // padding of the last XCD's range (uniform per workgroup)
        const uint32_t blk = blk_list ? blk_list[it] : it;
        const int64_t a0 = block_a0(blk, rt);                        // aligned coordinate of stream base 0 (multiple of 16)
        const uint32_t rb = rel_bias(bias, a0);                      // offset -> stream base of this block, in 32 bits (seed_plan.h)
        load_stream<ENC, TPB>(s.sF, bases_al, n_al, blk, a0, n_words);
        const uint32_t R0 = blk_rec[blk], R1 = blk_rec[blk + 1];
        // first offset staged: a pair's mate-1 offset in front of a block that starts with a mate 2 (by value: as an out-parameter of
        // stage_offsets it cost every instance two VGPRs)
        const uint32_t w_lo = paired ? (R0 & ~1u) : R0;
        const bool in_lds = stage_offsets(s, off, n_rec, R0, R1, w_lo);
        __syncthreads();
        uint32_t base_prev = 0;                                      // survivors of the earlier passes of this block
        const uint64_t out0 = (uint64_t)it * slot_cap;
        // (the pass is counted by the records left, so that no 32-bit index wraps in front of the last pass; a lane's own index is meant
        //  only where the lane has a record)
        for (uint32_t pass = R0, left = R1 - R0; left; pass += TPB, left -= min(left, (uint32_t)TPB)) {   // more than TPB records in a block: only tiny reads
            const uint32_t n_act = min(left, (uint32_t)TPB);
            // What a lane carries through the hash loop for the steps behind it is two 32-bit stream bases (ba, bb: its marker windows);
            // its k-mer count comes back from LDS, where deal_by_length put it.
            uint32_t nh, rel, ba, bb;
            if (record_geometry<K>(s, off, in_lds, w_lo, pass + tid, tid < n_act, paired, rb, avx2_compat, want_markers, nh, rel, ba, bb))
                state->long_record = 1u;                             // the host reruns the batch through the position kernel
            uint32_t slot, rel_h, nh_h, rows;
            const bool dealt = deal_by_length<TPB, hit_bits_by_lds<TPB>>(s, nh, rel, slot, rel_h, nh_h, rows);
            hash_record<K, HV, TPB, hit_bits_by_lds<TPB>>(s, slot, rel_h, nh_h, thr_loop, hit);
            if (dealt) __syncthreads();                              // masks were written by other lanes
            nh = s.nh[tid];
            uint32_t total = 0;
            bool decode = hit_bits_by_lds<TPB>;                      // the pass's first round decodes what the LDS atomics left
            for (;;) {                                               // (once; HV == 2: again after a candidate failed the exact test)
                uint32_t first;
                const uint32_t cnt = count_hits(s, nh, decode, first, total);
                decode = false;
                publish_markers(s, cnt, first, total, ba, bb);
                const bool is_listed = list_survivors(s, nh, cnt, first, total, rows);
                __syncthreads();
                finish_survivors<K, HV>(s, is_listed, rows, total, base_prev, slot_cap, thr, rec_base, pass, paired, avx2_compat, out0, slot_rec,
                                        slot_key, key_sh);
                __syncthreads();   // s.wave and s.mask are reused by the next pass
                if constexpr (HV != 2) break;
                else {
                    if (!*s.redo) break;                             // (uniform: read behind the barrier)
                    __syncthreads();
                    if (tid == 0) *s.redo = 0;                       // the next writer is several barriers away
                }
            }
            base_prev += total;
        }
        if (tid == 0) close_slots(blk_list != nullptr, blk, it, base_prev, slot_cap, blk_count, &state->spill, spill_slot_of_blk);
        __syncthreads();   // s.sF / s.off are rewritten by the next block
    }
}

// out[blk_off[b] + i] = slot[b * slot_cap + i] (or its spill region): the occurrences of the batch in file order
__global__ __launch_bounds__(64) void compact_occ_kernel(const OccRec* __restrict__ slot_rec, const uint32_t* __restrict__ blk_count,
                                                         const uint32_t* __restrict__ blk_off, uint32_t n_blk, uint32_t slot_cap,
                                                         uint32_t spill_cap, const OccRec* __restrict__ spill_rec,
                                                         const uint32_t* __restrict__ spill_slot_of_blk,
                                                         uint64_t* __restrict__ out_hash, OccRec* __restrict__ out_rec) {
    for (uint32_t b = blockIdx.x; b < n_blk; b += gridDim.x) {
        const uint32_t n = blk_count[b], d = blk_off[b];
        const OccRec* sr = slot_rec + (uint64_t)b * slot_cap;
        if (n > slot_cap) sr = spill_rec + (uint64_t)spill_slot_of_blk[b] * spill_cap;
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
            const OccRec r = sr[i];
            out_hash[d + i] = r.hash;   // the sort key array of the session
            out_rec[d + i] = r;
        }
    }
}

uint32_t grid_for(uint64_t n, uint32_t tpb = 256) { return (uint32_t)((n + tpb - 1) / tpb); }

// total = sum of the blocks' occurrence counts, written to blk_off[n_blk] — next to the two flag words of the state, so that
// everything the host wants to know about the batch leaves in ONE 12-byte copy (one workgroup: n_blk is a few ten thousand)
__global__ __launch_bounds__(1024) void block_total_kernel(const uint32_t* __restrict__ blk_count, uint32_t n_blk, uint32_t* __restrict__ total) {
    __shared__ uint32_t s[16];
    uint32_t v = 0;
    for (uint32_t i = threadIdx.x; i < n_blk; i += 1024) v += blk_count[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < 16; w++) t += s[w];
        *total = t;
    }
}

// the region's occurrences -> the session's dense file-order arrays (hash + OccRec), behind what is there already
void compact_region(sylph_sketch* sk, uint32_t n_blk, uint32_t slot_cap, uint32_t n, uint32_t spill_cap, const OccRec* spill_rec) {
    sylph_ctx* ctx = sk->ctx;
    const SlotMeta m = slot_meta_of(sk, n_blk);
    exclusive_sum_u32(ctx, m.blk_count, m.blk_off, (size_t)n_blk + 1);
    const uint64_t need = sk->n_occ + n;
    sk->hash.grow_keep(need * 8, sk->n_occ * 8, ctx->stream);
    sk->recs.grow_keep(need * sizeof(OccRec), sk->n_occ * sizeof(OccRec), ctx->stream);
    {
        ScopedKernelTimer t(ctx, "compact");
        hipLaunchKernelGGL(compact_occ_kernel, dim3(std::min<uint32_t>(n_blk, 1u << 16)), dim3(64), 0, ctx->stream,
                           sk->slot_rec.as<OccRec>(), m.blk_count, m.blk_off, n_blk, slot_cap, spill_cap, spill_rec, m.spill_slot,
                           sk->hash.as<uint64_t>() + sk->n_occ, sk->recs.as<OccRec>() + sk->n_occ);
        SY_HIP(hipGetLastError());
    }
    sk->n_occ = need;
}

}  // namespace

// The verdict of a deferred batch, read now: the block total + the two flags (what push_short_reads reads when it does not
// defer).  A bad verdict redoes the batch through the checked push; afterwards the session is in the state an ordinary push
// would have left it in.
void resolve_deferred_slots(sylph_sketch* sk) {
    if (!sk->pend.live || !sk->pend.deferred) return;
    sylph_ctx* ctx = sk->ctx;
    const SlotMeta m = slot_meta_of(sk, sk->pend.n_blk);
    hipLaunchKernelGGL(block_total_kernel, dim3(1), dim3(1024), 0, ctx->stream, m.blk_count, sk->pend.n_blk, m.blk_off + sk->pend.n_blk);
    uint32_t res[3] = {0, 0, 0};
    ctx->read_back(res, m.blk_off + sk->pend.n_blk, 12);
    if (res[1] || res[2]) { redo_deferred_batch(sk); return; }
    sk->pend.deferred = false;
    sk->pend.n = res[0];
    if (res[0] == 0) sk->pend = PendingSlots{};
}

void flush_pending_slots(sylph_sketch* sk) {
    resolve_deferred_slots(sk);
    if (!sk->pend.live) return;
    compact_region(sk, sk->pend.n_blk, sk->pend.slot_cap, sk->pend.n, 0, nullptr);
    sk->pend = PendingSlots{};
}

// Short-read path of sylph_sketch_push: returns true with the batch's occurrences taken over by the session — left in their
// slots (sk->pend) when this is the session's first batch and no block overflowed, else appended to the dense arrays (hash +
// OccRec, file order); returns false — having taken nothing — when the batch is not for this kernel (a record longer than
// READ_HALO, or more overflowing blocks than spill regions), and the caller runs the position kernel + annotate instead.
bool push_short_reads(sylph_sketch* sk, const uint8_t* d_bases, uint32_t phase, const uint64_t* d_off, uint64_t n_records, uint64_t n_bases,
                      int enc) {
    sylph_ctx* ctx = sk->ctx;
    // the kernel works in 16 B-aligned coordinates: bias = bases between the aligned address below d_bases and d_bases
    // (a packed stream holds 4 bases per byte and may begin `phase` bases into its first byte)
    const uint32_t bias = enc == SYLPH_ENC_2BIT ? (uint32_t)((uintptr_t)d_bases & 15) * 4u + phase : (uint32_t)((uintptr_t)d_bases & 15);
    const uint8_t* bases_al = d_bases - ((uintptr_t)d_bases & 15);
    const uint64_t n_al = n_bases + bias;
    // block size, slots and LDS: seed_plan.h reads_block_plan
    static const int env_ragged_tpb = [] { const char* e = getenv("SYLPH_HIP_READS_RAGGED_TPB"); return e ? atoi(e) : RTPB; }();
    const ReadsBlockPlan plan = reads_block_plan(n_bases, n_records, bias, sk->c, sk->k, env_ragged_tpb == RTPB_RAGGED);
    const int tpb = plan.tpb;
    const uint32_t rt = plan.rt, n_blk = plan.n_blk, spill_cap = plan.spill_cap, slot_cap = plan.slot_cap;
    const size_t lds_bytes = plan.lds_bytes;
    const uint64_t thr = UINT64_MAX / (uint64_t)sk->c;
    // the slots belong to the SESSION (from the context's pool): they may outlive this call (sk->pend)
    sk->slot_rec.reserve((size_t)n_blk * slot_cap * sizeof(OccRec));
    sk->slot_key.reserve((size_t)n_blk * slot_cap * 4);
    // (the total — blk_off[n_blk] — and the two flag words of the state sit side by side and leave in ONE 12-byte copy)
    sk->slot_meta.reserve(SlotMeta::bytes(n_blk, sizeof(ReadsState)));
    const SlotMeta m = slot_meta_of(sk, n_blk);
    ReadsState* const state = reinterpret_cast<ReadsState*>(m.state_words);
    static_assert(offsetof(ReadsState, long_record) == 0 && offsetof(ReadsState, spill) == 4 && offsetof(SpillState, n_tiles) == 0,
                  "long_record and spill.n_tiles are the first two words");
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
    // the k-mer loop's hash / threshold spelling (seed_plan.h hash_variant_env).  Same results all three (tests run each).
    const int hv_want = ctx->reads_hash >= 0 ? ctx->reads_hash : hash_variant_env(SYLPH_READS_HASH_DEFAULT);
    // hi(T) + 1 + slack has to stay a 32-bit number (c = 1: every k-mer passes, T = 2^64 - 1)
    const uint32_t slack = ctx->reads_slack;
    const int hv = (hv_want == 2 && ((thr >> 32) + 1ull + slack) > 0xFFFFFFFFull) ? 1 : hv_want;
    const int key_sh = key_shift(sk->c);
    // positions [it_b, it_e) of the dealing of n_it blocks (reads_kernel)
    auto launch = [&](uint32_t n_it, uint32_t it_b, uint32_t it_e, uint32_t cap, OccRec* sr, uint32_t* skey, const uint32_t* list) {
        if (it_e <= it_b) return;
        const uint32_t grid = ctx->reads_wg_per_cu ? (uint32_t)std::min<uint64_t>(it_e - it_b, (uint64_t)cus * ctx->reads_wg_per_cu) : it_e - it_b;
        auto go = [&](auto kc, auto hc, auto ec, auto tc) {
            constexpr int KK = decltype(kc)::value, HH = decltype(hc)::value, EE = decltype(ec)::value, TT = decltype(tc)::value;
            hipLaunchKernelGGL((reads_kernel<KK, HH, EE, TT>), dim3(grid), dim3(TT), lds_bytes, ctx->stream, bases_al, bias, n_al, d_off, n_records,
                               m.blk_rec, n_it, it_b, it_e, rt, thr, slack, sk->avx2_compat, sk->paired, sk->no_dedup ? 0 : 1, sk->rec_base, cap, sr, skey,
                               key_sh, m.blk_count, state, list, m.spill_slot);
        };
        auto with_tpb = [&](auto kc, auto hc, auto ec) {
            if (tpb == RTPB_RAGGED) go(kc, hc, ec, std::integral_constant<int, RTPB_RAGGED>{}); else go(kc, hc, ec, std::integral_constant<int, RTPB>{});
        };
        // (packed input has no instance of spelling 0; the session checked k)
        if (enc == SYLPH_ENC_2BIT) with_k_hv<1, 2>(sk->k, hv, [&](auto kc, auto hc) { with_tpb(kc, hc, std::integral_constant<int, 1>{}); });
        else with_k_hv<0, 2>(sk->k, hv, [&](auto kc, auto hc) { with_tpb(kc, hc, std::integral_constant<int, 0>{}); });
        SY_HIP(hipGetLastError());
    };
    {
        HostPhase ph(ctx, "push: reads kernel");
        {
            ScopedKernelTimer t(ctx, "annotate");   // the record lookup this kernel replaces
            hipLaunchKernelGGL(block_records_kernel, dim3(grid_for(n_blk + 1)), dim3(256), 0, ctx->stream, d_off, n_records, bias, rt,
                               n_blk + 1, m.blk_rec, m.blk_count + n_blk, m.state_words);
        }
        ctx->seed_gate();
        {
            // In a pipeline's turn the sample's last positions are a launch of their own and the turn's event sits in front of it: the next
            // sample's kernel starts while this one's last workgroups drain (two seeding kernels share the chip for those few per cent of
            // one — the work is the same, the event-to-wait latency and the drain of a 26,000-workgroup grid are not paid between them).
            // (The tail is a launch of its own for the timers too: one pair of events around both would count the time the tail waits behind
            //  the turn's event — the next sample's kernel is running then — as this kernel's duration.)
            const uint32_t n_round = xcd_positions(n_blk);
            const uint32_t cut = xcd_tail_cut(n_blk, ctx->turn.done && !ctx->turn.recorded ? ctx->reads_tail_pct : 0);
            {
                ScopedKernelTimer t(ctx, "seeds");
                launch(n_blk, 0, cut, slot_cap, sk->slot_rec.as<OccRec>(), sk->slot_key.as<uint32_t>(), nullptr);
            }
            ctx->seed_done();
            if (cut < n_round) {
                ScopedKernelTimer t(ctx, "seeds");
                launch(n_blk, cut, n_round, slot_cap, sk->slot_rec.as<OccRec>(), sk->slot_key.as<uint32_t>(), nullptr);
            }
        }
        // deferred verdict (sketch_session.h PendingSlots): the caller keeps the batch valid until finish, this is the session's first
        // batch and nothing forces the dense arrays — no block total, no read-back, no wait; finish reads the flags with its own tail
        const uint64_t n_expect = plan.n_expect;
        if (sk->borrow_until_finish && sk->n_occ == 0 && sk->rec_base == 0 && ctx->finish_mode == 0 && sk->c >= 2 && n_expect >= 4096 &&
            (uint64_t)n_blk * slot_cap < (1ull << 31)) {
            sk->pend = PendingSlots{};
            sk->pend.live = true;
            sk->pend.deferred = true;
            sk->pend.n_blk = n_blk;
            sk->pend.slot_cap = slot_cap;
            sk->pend.n = n_blk * slot_cap;               // upper bound: no block holds more than its slots (else the verdict says so)
            sk->pend.n_expect = (uint32_t)std::min<uint64_t>(n_expect, sk->pend.n);
            sk->pend.bases = d_bases; sk->pend.phase = phase; sk->pend.off = d_off;
            sk->pend.n_records = n_records; sk->pend.n_bases = n_bases; sk->pend.enc = enc;
            if (ctx->profile) ctx->stats["deferred"].launches++;     // (tests ask sylph_ctx_kernel_stats whether this road was taken)
            return true;
        }
        hipLaunchKernelGGL(block_total_kernel, dim3(1), dim3(1024), 0, ctx->stream, m.blk_count, n_blk, m.blk_off + n_blk);
    }
    uint32_t res[3] = {0, 0, 0};   // total occurrences, long_record flag, overflowing blocks
    SY_HIP(hipMemcpyAsync(ctx->pinned, m.blk_off + n_blk, 12, hipMemcpyDeviceToHost, ctx->stream));
    SY_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(res, ctx->pinned, 12);
    if (!ctx->pending.empty()) profile_collect(ctx);
    if (res[1] || res[2] > SPILL_MAX_TILES) return false;
    const uint32_t n = res[0];
    if (n == 0) return true;
    // The first batch of a session stays in its slots: a sample that arrives in one batch is partitioned from there (no
    // compaction pass over its 32 B records at all).  Not with overflowing blocks (their occurrences live in spill regions), not
    // behind occurrences that are in the dense arrays already, not when the device-wide finish was asked for (it wants them dense).
    if (res[2] == 0 && sk->n_occ == 0 && ctx->finish_mode != 1 && sk->c >= 2) {
        sk->pend.live = true;
        sk->pend.n_blk = n_blk;
        sk->pend.slot_cap = slot_cap;
        sk->pend.n = n;
        return true;
    }
    const OccRec* sp_r = nullptr;
    if (res[2]) {   // a few blocks (low-complexity reads) are redone with room for every position
        DevBuf& b_x = ctx->scratch[7];   // spill records
        b_x.reserve((size_t)res[2] * spill_cap * sizeof(OccRec));
        OccRec* xr = b_x.as<OccRec>();
        ScopedKernelTimer ts(ctx, "seeds_spill");
        ScopedKernelTimer t(ctx, "seeds");
        launch(res[2], 0, res[2], spill_cap, xr, nullptr, state->spill.tiles);
        sp_r = xr;
    }
    compact_region(sk, n_blk, slot_cap, n, spill_cap, sp_r);
    return true;
}

}  // namespace sylph
