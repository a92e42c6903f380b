// replay_lds.hip — finish() of a read-sketch session without device-wide sorts: bucket partition + in-LDS replay.
//
// FracMinHash survivors are uniformly distributed below the threshold (mm_hash64 is a bijection of canonical
// k-mers), so the top bits of the hash split the sample's occurrences into B buckets of nearly equal size (~96: nearly all of them
// at most 128, one occurrence per lane of the replay workgroup — replay_bucket_lane).
// The PARTITION (partition.h: hand-written, four small kernels, no library sort, no memset dispatches) only moves 8-byte
// (bucket, occurrence index) pairs, in two levels: tiles of occurrences are histogrammed over <= 512 coarse hash ranges, a
// scan turns the (range x tile) counts into offsets, the pairs are scattered range by range, and one workgroup per coarse
// range finishes with a counting sort by bucket in LDS, which also yields the bucket offsets.  Neither level keeps the file
// order inside a bucket (ranks come from LDS atomics): the occurrence index IS the file order, and the replay workgroup
// re-establishes it for its ~128 occurrences with one rank loop.  The 32 B occurrence records never move: the replay gathers
// them through the permutation — from the session's dense arrays, or straight from the per-block slots the seeding kernel
// left them in when the sample came in one batch (no compaction pass at all).
// One workgroup then owns one bucket entirely in LDS: counting-rank sort by (hash, file order) -> k-mer segments in file
// order -> mate-2 skip, duplicate flags, cut-off and counts (the same data-parallel formulation of
// dup_removal_lsh_full_exact as sketch.hip, see its header) -> distinct (k-mer, count) pairs.  Buckets are ordered
// by hash, so concatenating their outputs gives the table in ascending k-mer order.
// A bucket beyond 1024 occurrences (a k-mer more than ~1000 deep) goes through the device-wide path of sketch.hip, as a
// small sample of its own.
// Where what is: replay_plan.h — the bucket map (HIP-free, tested on the CPU); partition.h — the partition kernels;
// replay_bucket.h — what a workgroup does with one bucket (the shared steps and the three bodies); this file — the kernels around
// the bodies, the table close, the detour of overflowing buckets and the host function finish_bucketed.
#include "replay_bucket.h"

namespace sylph {
namespace {

// What the host reads back at the end of a pass: written by table_compact_kernel (`overflow`: by the replay), copied in one piece.
struct FinishTail {
    unsigned long long removed;  // duplicates dropped
    uint32_t overflow;           // buckets with inconsistent bounds (defensive)
    uint32_t n_seg;              // rows of the table
    uint32_t n_ovf, n_mid, n_large;   // heads of the three lists
    uint32_t verdict[2];         // deferred seeding verdict (reads.hip ReadsState: long_record, overflowing blocks)
    uint32_t a10_words[2];       // verdict of the filter dedup's partitioned pass (a10.hip)
    uint32_t n_found;            // occurrences the partition found: what a deferred batch's slots really hold
};
static_assert(sizeof(FinishTail) == 48, "tail block");

// LANE: which instance of the lane body the kernel carries beside replay_bucket — LANE_OFF (none: replay_bucket runs every bucket)
// or lane_mode(paired, dedup).  The choice per bucket is uniform over the workgroup: at most LANE_CAP occurrences,
// consistent bounds, composite keys with a one-word ranking key -> the lane body; everything else (129 ... 256 occurrences, larger
// ones queued, inconsistent bounds counted) -> replay_bucket, in the same launch and the same LDS.
constexpr int LANE_OFF = -1;
constexpr int lane_mode(bool paired, int dedup) { return (paired ? 1 : 0) | (dedup << 1); }
// (num_sgpr: two bodies in one kernel take 101 scalar registers when left alone, one more than 8 wavefronts per SIMD leave each — and
//  with the LDS admitting 15 workgroups per CU, 7.5 wavefronts per SIMD, the eighth counts; held to 100 nothing spills)
template <int CAP, int RTPB, int LANE = LANE_OFF>
__global__ __launch_bounds__(RTPB) __attribute__((amdgpu_num_sgpr(100))) void bucket_replay_kernel(ReplayArgs ra) {
    __shared__ ReplayLds<CAP, RTPB> lds;
    if constexpr (LANE != LANE_OFF) {
        static_assert(CAP == CAP_SMALL && RTPB == LANE_CAP, "the lane body shares the 256-slot configuration's workgroup");
        uint32_t first, n;
        if (bucket_bounds(ra, blockIdx.x, first, n) && n >= 1 && n <= (uint32_t)LANE_CAP && ra.bm.composite && ra.bm.rank_bits[LANE_CFG]) {
            replay_bucket_lane<(LANE & 1) != 0, (LANE >> 1)>(blockIdx.x, first, n, ra, lds);
            return;
        }
    }
    replay_bucket<CAP, RTPB>(blockIdx.x, ra, lds);
}

template <int CAP, int RTPB>
__global__ __launch_bounds__(RTPB) void bucket_count_kernel(ReplayArgs ra) {
    count_bucket<CAP, RTPB>(blockIdx.x, ra);
}
// the list-driven configurations: a fixed, small grid walks the (usually empty) list of buckets an earlier configuration queued
template <int CAP, int RTPB>
__global__ __launch_bounds__(RTPB) void bucket_count_list_kernel(ReplayArgs ra, const uint32_t* __restrict__ my_list) {
    const uint32_t n_listed = my_list[0];
    for (uint32_t i = blockIdx.x; i < n_listed; i += gridDim.x) {
        count_bucket<CAP, RTPB>(my_list[1 + i], ra);
        __syncthreads();
    }
}
template <int CAP, int RTPB>
__global__ __launch_bounds__(RTPB) void bucket_replay_list_kernel(ReplayArgs ra, const uint32_t* __restrict__ my_list) {
    const uint32_t n_listed = my_list[0];
    __shared__ ReplayLds<CAP, RTPB> lds;
    for (uint32_t i = blockIdx.x; i < n_listed; i += gridDim.x) {
        replay_bucket<CAP, RTPB>(my_list[1 + i], ra, lds);
        __syncthreads();   // the LDS arrays are reused by the next bucket
    }
}

// Table offsets in two levels, no library scan: workgroup w scans the 1024 buckets of its chunk — d_loc[b] = table rows of the
// chunk's buckets before b — and leaves the chunk's row total and removed total; the compaction kernel adds the chunk totals
// before w (at most 256 of them: B <= 2^18 on this path).
constexpr uint32_t SCAN_CHUNK = 1024;
__global__ __launch_bounds__(SCAN_CHUNK) void table_scan_kernel(const uint32_t* __restrict__ n_distinct, const uint32_t* __restrict__ removed_b,
                                                                uint32_t B, uint32_t ipt, uint32_t* __restrict__ d_loc,
                                                                uint32_t* __restrict__ chunk_rows, unsigned long long* __restrict__ chunk_removed) {
    // a workgroup scans a chunk of SCAN_CHUNK * ipt buckets, every lane `ipt` consecutive ones (ipt = 1 up to 2^18 buckets; a
    // long-read sample at c = 100 has 4e5: at most 256 chunks whatever B, so that the second level fits one workgroup's LDS)
    __shared__ uint32_t s_wave[SCAN_CHUNK / 64];
    __shared__ unsigned long long s_rem[SCAN_CHUNK / 64];
    const uint32_t b0 = (blockIdx.x * SCAN_CHUNK + threadIdx.x) * ipt, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t v = 0;
    unsigned long long rem = 0;
    for (uint32_t i = 0; i < ipt && b0 + i < B; i++) { v += n_distinct[b0 + i]; rem += removed_b[b0 + i]; }
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= (uint32_t)d) x += y;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) rem += __shfl_xor(rem, d);
    if (lane == 63) s_wave[wave] = x;
    if (lane == 0) s_rem[wave] = rem;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (uint32_t w = 0; w < SCAN_CHUNK / 64; w++) { const uint32_t t = s_wave[w]; if (w < wave) base += t; tot += t; }
    uint32_t run = base + x - v;
    for (uint32_t i = 0; i < ipt && b0 + i < B; i++) { d_loc[b0 + i] = run; run += n_distinct[b0 + i]; }
    if (threadIdx.x == 0) {
        unsigned long long r = 0;
        for (uint32_t w = 0; w < SCAN_CHUNK / 64; w++) r += s_rem[w];
        chunk_rows[blockIdx.x] = tot;
        chunk_removed[blockIdx.x] = r;
    }
}
// out[rows before bucket b + i] = tmp[boff[b] + i] for i < n_distinct[b]; a workgroup walks buckets with its four wavefronts
// (one bucket holds ~50 rows).  Also fills the tail block the host reads (FinishTail).
__global__ __launch_bounds__(256) void table_compact_kernel(const uint64_t* __restrict__ tmp_k, const uint32_t* __restrict__ tmp_c,
                                                            const uint32_t* __restrict__ boff, const uint32_t* __restrict__ d_loc,
                                                            const uint32_t* __restrict__ chunk_rows, const unsigned long long* __restrict__ chunk_removed,
                                                            const uint32_t* __restrict__ n_distinct, uint32_t B, uint32_t ipt,
                                                            uint64_t* __restrict__ out_k, uint32_t* __restrict__ out_c,
                                                            const uint32_t* __restrict__ ovf_list, const uint32_t* __restrict__ mid_list,
                                                            const uint32_t* __restrict__ large_list, int skip_if_listed,
                                                            FinishTail* __restrict__ tail, const uint32_t* __restrict__ verdict,
                                                            const uint32_t* __restrict__ a10_words, const uint32_t* __restrict__ p_nv) {
    __shared__ uint32_t s_base[257];
    __shared__ uint32_t s_wave[4];
    __shared__ unsigned long long s_rem[4];
    const uint32_t chunk = SCAN_CHUNK * ipt, n_chunks = (B + chunk - 1) / chunk;        // <= 256: one chunk total per lane
    {
        const uint32_t v = threadIdx.x < n_chunks ? chunk_rows[threadIdx.x] : 0u;
        uint32_t tot = 0;
        const uint32_t ex = block_excl_sum<256>(v, s_wave, &tot);
        if (threadIdx.x < n_chunks) s_base[threadIdx.x] = ex;
        if (threadIdx.x == 0) s_base[n_chunks] = tot;
        if (blockIdx.x == 0) {                                                       // the tail block, once
            unsigned long long rem = threadIdx.x < n_chunks ? chunk_removed[threadIdx.x] : 0ull;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) rem += __shfl_xor(rem, d);
            if ((threadIdx.x & 63) == 0) s_rem[threadIdx.x >> 6] = rem;
            __syncthreads();
            if (threadIdx.x == 0) {
                tail->removed = s_rem[0] + s_rem[1] + s_rem[2] + s_rem[3];
                tail->n_seg = tot; tail->n_ovf = ovf_list[0]; tail->n_mid = mid_list[0]; tail->n_large = large_list[0];
                // the deferred seeding verdict and the filter pass's verdict words ride in the same block: one copy
                tail->verdict[0] = verdict ? verdict[0] : 0u; tail->verdict[1] = verdict ? verdict[1] : 0u;
                tail->a10_words[0] = a10_words ? a10_words[0] : 0u; tail->a10_words[1] = a10_words ? a10_words[1] : 0u;
                tail->n_found = *p_nv;
            }
        }
    }
    __syncthreads();
    // buckets are still waiting for the list-driven configurations: the host will come back after running them (a long-read
    // table has tens of millions of rows: copying it twice would cost more than the configurations themselves)
    if (skip_if_listed && (mid_list[0] | large_list[0])) return;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t b = blockIdx.x * 4 + wave; b < B; b += gridDim.x * 4) {
        const uint32_t n = n_distinct[b], s0 = boff[b], d = s_base[b / chunk] + d_loc[b];
        for (uint32_t i = lane; i < n; i += 64) { out_k[d + i] = tmp_k[s0 + i]; out_c[d + i] = tmp_c[s0 + i]; }
    }
}
// ---- buckets beyond the large configuration: their occurrences go through the device-wide path as one small sample --------
// sub_off[i] = occurrences of the listed buckets before bucket i (single workgroup; the list is short); sub_off[m] = total
__global__ __launch_bounds__(1024) void ovf_offsets_kernel(const uint32_t* __restrict__ ovf_list, const uint32_t* __restrict__ boff,
                                                           uint32_t* __restrict__ sub_off) {
    __shared__ uint32_t s_part[1024];
    const uint32_t m = ovf_list[0], tid = threadIdx.x;
    const uint32_t per = (m + 1023) / 1024;
    uint32_t sum = 0;
    for (uint32_t i = tid * per; i < min(m, (tid + 1) * per); i++) { const uint32_t b = ovf_list[1 + i]; sum += boff[b + 1] - boff[b]; }
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (uint32_t t = 0; t < 1024; t++) { const uint32_t v = s_part[t]; s_part[t] = run; run += v; }
        sub_off[m] = run;
    }
    __syncthreads();
    uint32_t run = s_part[tid];
    for (uint32_t i = tid * per; i < min(m, (tid + 1) * per); i++) {
        const uint32_t b = ovf_list[1 + i];
        sub_off[i] = run;
        run += boff[b + 1] - boff[b];
    }
}

// the occurrence indices of listed bucket i -> sub_idx[sub_off[i] ..): sorted afterwards, they are the listed buckets'
// occurrences in FILE order (what the device-wide path expects of its input)
__global__ __launch_bounds__(256) void ovf_indices_kernel(const uint32_t* __restrict__ ovf_list, const uint32_t* __restrict__ sub_off,
                                                          const uint32_t* __restrict__ boff, const uint32_t* __restrict__ perm,
                                                          uint32_t* __restrict__ sub_idx) {
    const uint32_t b = ovf_list[1 + blockIdx.x], first = boff[b], n = boff[b + 1] - first, o = sub_off[blockIdx.x];
    for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) sub_idx[o + j] = perm[first + j];
}
__global__ __launch_bounds__(256) void ovf_gather_kernel(const uint32_t* __restrict__ sorted_idx, uint32_t n, const OccRec* __restrict__ recs,
                                                         uint64_t* __restrict__ sub_hash, OccRec* __restrict__ sub_recs) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const OccRec r = recs[sorted_idx[j]];
    sub_hash[j] = r.hash;
    sub_recs[j] = r;
}

// the (k-mer, count) rows the device-wide path produced for listed bucket i go to the bucket's slots of the temporary table
__global__ __launch_bounds__(256) void ovf_patch_kernel(const uint32_t* __restrict__ ovf_list, BucketMap bm,
                                                        const uint64_t* __restrict__ sub_k, const uint32_t* __restrict__ sub_c,
                                                        uint32_t n_sub_out, const uint32_t* __restrict__ boff,
                                                        uint64_t* __restrict__ tmp_k, uint32_t* __restrict__ tmp_c,
                                                        uint32_t* __restrict__ n_distinct) {
    const uint32_t b = ovf_list[1 + blockIdx.x];
    auto lower = [&](uint64_t key) {   // first row with k-mer >= key
        uint32_t lo = 0, hi = n_sub_out;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (sub_k[mid] < key) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    // rows of bucket b = rows with k-mer in [smallest hash of bucket b, smallest hash of bucket b + 1) (inverse of bucket_of)
    __shared__ uint32_t s_lo, s_hi;
    if (threadIdx.x == 0) {
        s_lo = lower(bucket_lo_hash(b, bm.mult, bm.sh));
        s_hi = (b + 1 < bm.B) ? lower(bucket_lo_hash(b + 1, bm.mult, bm.sh)) : n_sub_out;
    }
    __syncthreads();
    const uint32_t lo = s_lo, n = s_hi - s_lo, d = boff[b];
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) { tmp_k[d + i] = sub_k[lo + i]; tmp_c[d + i] = sub_c[lo + i]; }
    if (threadIdx.x == 0) n_distinct[b] = n;
}

// The 256-slot launch: the instance that carries the lane body for the sample's mode (pairs or single-end, exact set or filter —
// the modes a sample can come in by default or by one flag); any other combination, a build with another workgroup size and the
// stage cuts of SYLPH_REPLAY_STAGE (which the lane body does not have) take replay_bucket alone.
void launch_replay(sylph_ctx* ctx, uint32_t B, const ReplayArgs& ra, bool paired, bool stage_cut) {
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(B), dim3(RTPB_SMALL), 0, ctx->stream, ra); };
    if constexpr (RTPB_SMALL == LANE_CAP) {
        if (!stage_cut) {
            if (paired && ra.dedup == DEDUP_EXACT) return go(bucket_replay_kernel<CAP_SMALL, RTPB_SMALL, lane_mode(true, DEDUP_EXACT)>);
            if (paired && ra.dedup == DEDUP_FILTER) return go(bucket_replay_kernel<CAP_SMALL, RTPB_SMALL, lane_mode(true, DEDUP_FILTER)>);
            if (!paired && ra.dedup == DEDUP_EXACT) return go(bucket_replay_kernel<CAP_SMALL, RTPB_SMALL, lane_mode(false, DEDUP_EXACT)>);
        }
    }
    go(bucket_replay_kernel<CAP_SMALL, RTPB_SMALL>);
}
// Which body a launch_replay of this map sends a bucket of n occurrences to (the kernel's own test, for the road counters)
bool lane_road(const BucketMap& bm, uint32_t n, bool paired, int dedup, bool stage_cut) {
    const bool instance = RTPB_SMALL == LANE_CAP && !stage_cut && (dedup == DEDUP_EXACT || (paired && dedup == DEDUP_FILTER));
    return instance && n >= 1 && n <= (uint32_t)LANE_CAP && bm.composite && bm.rank_bits[LANE_CFG];
}

uint32_t grid_of(uint64_t n, uint32_t tpb = 256) { return (uint32_t)((n + tpb - 1) / tpb); }

// The per-bucket words of a pass, carved out of one scratch buffer, B + 2 words each but the last two:
//   boff         boff[b] = first position of bucket b; boff[B] = number of valid occurrences
//   large_list   [0] = number of buckets queued for the large configuration, [1..] = ids
//   ovf_list     [0] = number of buckets beyond the large configuration, [1..] = ids
//   n_distinct, removed_b   per bucket; cleared by part_hist_kernel (n_zero words from n_distinct on)
//   d_off        table rows of the chunk's buckets before b (table_scan_kernel)
//   mid_list     buckets for the medium configuration (n <= CAP_MID, or a long k-mer segment)
//   chunk_rows (264 words) | chunk_removed (264 u64): the chunk totals of the table close
struct BucketWords {
    uint32_t *boff, *large_list, *ovf_list, *n_distinct, *removed_b, *d_off, *mid_list, *chunk_rows;
    unsigned long long* chunk_removed;
    uint32_t n_zero;
    static BucketWords carve(DevBuf& buf, uint32_t B) {
        const size_t each = (size_t)B + 2;
        buf.reserve(each * 4 * 7 + 264 * 4 + 264 * 8 + 16);
        uint32_t* const p = buf.as<uint32_t>();
        uint32_t* const rows = p + 7 * each + ((B & 1u) ? 1 : 0);       // (8-byte aligned: 7 * (B + 2) words is odd for odd B)
        return BucketWords{p, p + each, p + 2 * each, p + 3 * each, p + 4 * each, p + 5 * each, p + 6 * each, rows,
                           reinterpret_cast<unsigned long long*>(rows + 264), (uint32_t)each * 2};
    }
};

// One pass of finish_bucketed after the partition and the 256-slot launch: what its later steps share.
struct FinishPass {
    sylph_sketch* sk;
    sylph_ctx* ctx;
    uint32_t B;
    BucketWords w;
    ReplayArgs ra;
    FinishTail* d_tail;
    bool plain, deferred;
    FinishTail host{};           // the tail block as last read

    // removed counts, table offsets, compaction, and everything the host needs to know in one block (FinishTail)
    void close_table(int skip_if_listed) {
        // two levels: chunks of 1024 x ipt buckets (at most 256 of them), then the compaction, which scans the chunk totals itself
        const uint32_t ipt = (B + (1u << 18) - 1) >> 18;
        ScopedKernelTimer t(ctx, "replay");
        hipLaunchKernelGGL(table_scan_kernel, dim3((B + SCAN_CHUNK * ipt - 1) / (SCAN_CHUNK * ipt)), dim3(SCAN_CHUNK), 0, ctx->stream, w.n_distinct,
                           w.removed_b, B, ipt, w.d_off, w.chunk_rows, w.chunk_removed);
        hipLaunchKernelGGL(table_compact_kernel, dim3(std::min<uint32_t>((B + 3) / 4, 1u << 15)), dim3(256), 0, ctx->stream,
                           ra.tmp_k, ra.tmp_c, w.boff, w.d_off, w.chunk_rows, w.chunk_removed, w.n_distinct, B, ipt,
                           sk->out_k.as<uint64_t>(), sk->out_c.as<uint32_t>(), w.ovf_list, w.mid_list, w.large_list, skip_if_listed,
                           d_tail, deferred ? slot_meta_of(sk, sk->pend.n_blk).state_words : (const uint32_t*)nullptr,
                           sk->a10_marks == FilterMarks::Unread ? sk->a10_tail.as<uint32_t>() : (const uint32_t*)nullptr, ra.p_nv);
        SY_HIP(hipGetLastError());
    }
    void read_tail() {
        SY_HIP(hipMemcpyAsync(ctx->pinned, d_tail, sizeof host, hipMemcpyDeviceToHost, ctx->stream));
        SY_HIP(hipStreamSynchronize(ctx->stream));
        memcpy(&host, ctx->pinned, sizeof host);
        if (!ctx->pending.empty()) profile_collect(ctx);
    }
    // Road counters (tests and tools ask sylph_ctx_kernel_stats how many buckets took which body): from the bucket offsets, on the
    // host — the kernel keeps no count.  Only where the replay family is timed at all: a region that times the seeding kernel
    // alone (bench.py's quoted rate) pays no read-back.
    void count_roads() {
        if (!ctx->profile || plain || !(ctx->profile_only.empty() || ctx->profile_only.find(",replay,") != std::string::npos)) return;
        std::vector<uint32_t> h_boff((size_t)B + 1);
        ctx->d2h(h_boff.data(), w.boff, ((size_t)B + 1) * 4);
        uint64_t n_lane = 0, n_general = 0;
        for (uint32_t i = 0; i < B; i++) {
            const uint32_t n_b = h_boff[i + 1] - h_boff[i];
            if (lane_road(ra.bm, n_b, sk->paired != 0, ra.dedup, ra.dbg_stage != 0)) n_lane++;
            else if (n_b) n_general++;
        }
        ctx->stats["replay_lane"].launches += n_lane;
        ctx->stats["replay_general"].launches += n_general;
    }
    // Buckets the 256-slot configuration passed on (more than 256 occurrences, or a k-mer 96+ deep: abundant genomes).  The
    // list-driven configurations are launched only now, with grids that match the lists: launched speculatively with every
    // sample they are two dispatches of large-LDS workgroups that find nothing to do, but cannot even START beside another
    // stream's seeding kernel (which leaves 10 KiB of LDS per CU) — in the pipelined bench they held the stream up for 0.3 ms.
    void run_listed_configurations() {
        HostPhase ph(ctx, "finish(bucket): medium / large configurations");
        {
            ScopedKernelTimer t(ctx, "replay");
            if (plain) {
                if (host.n_large)
                    hipLaunchKernelGGL((bucket_count_list_kernel<CAP_LARGE, RTPB_LARGE>), dim3(std::min<uint32_t>(host.n_large, 1536u)),
                                       dim3(RTPB_LARGE), 0, ctx->stream, ra, w.large_list);
            } else {
                if (host.n_mid)
                    hipLaunchKernelGGL((bucket_replay_list_kernel<CAP_MID, RTPB_MID>), dim3(std::min<uint32_t>(host.n_mid, 1280u)),
                                       dim3(RTPB_MID), 0, ctx->stream, ra, w.mid_list);
                if (host.n_large)
                    hipLaunchKernelGGL((bucket_replay_list_kernel<CAP_LARGE, RTPB_LARGE>), dim3(std::min<uint32_t>(host.n_large, 512u)),
                                       dim3(RTPB_LARGE), 0, ctx->stream, ra, w.large_list);
            }
        }
        close_table(0);
        read_tail();
    }
    // Some buckets exceed even the large configuration (k-mers with thousands of occurrences: low-complexity reads, very abundant
    // genomes).  Only THEIR occurrences go through the device-wide path, as one small sample; its rows are patched into the buckets'
    // slots and the table is compacted again.  -> duplicates the device-wide path dropped.
    unsigned long long run_overflowing_buckets() {
        HostPhase ph(ctx, "finish(bucket): overflowing buckets through the device-wide path");
        const uint32_t m = host.n_ovf;
        DevBuf b_so(ctx), b_si(ctx), b_sh(ctx), b_sr(ctx), sub_k(ctx), sub_c(ctx);
        b_so.reserve(((size_t)m + 1) * 4);
        hipLaunchKernelGGL(ovf_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, w.ovf_list, w.boff, b_so.as<uint32_t>());
        uint32_t n_sub = 0;
        ctx->read_back(&n_sub, b_so.as<uint32_t>() + m, 4);
        b_si.reserve((size_t)n_sub * 8);            // indices | sorted indices
        b_sh.reserve((size_t)n_sub * 8);
        b_sr.reserve((size_t)n_sub * sizeof(OccRec));
        uint32_t* sub_idx = b_si.as<uint32_t>();
        uint32_t* sub_sorted = sub_idx + n_sub;
        hipLaunchKernelGGL(ovf_indices_kernel, dim3(m), dim3(256), 0, ctx->stream, w.ovf_list, b_so.as<uint32_t>(), w.boff, ra.perm, sub_idx);
        sort_keys_u32(ctx, sub_idx, sub_sorted, n_sub, 0, 32);       // ascending index = file order
        {
            ScopedKernelTimer t(ctx, "replay_overflow");   // (family of its own so that tests can see this path was taken)
            hipLaunchKernelGGL(ovf_gather_kernel, dim3(grid_of(n_sub)), dim3(256), 0, ctx->stream, sub_sorted, n_sub, ra.recs,
                               b_sh.as<uint64_t>(), b_sr.as<OccRec>());
        }
        uint64_t n_sub_out = 0, removed_sub = 0;
        generic_replay(ctx, b_sh.as<uint64_t>(), b_sr.as<OccRec>(), n_sub, sk->paired, sk->dedup_mode(), sub_k, sub_c, n_sub_out, removed_sub);
        {
            ScopedKernelTimer t(ctx, "replay");
            hipLaunchKernelGGL(ovf_patch_kernel, dim3(m), dim3(256), 0, ctx->stream, w.ovf_list, ra.bm, sub_k.as<uint64_t>(),
                               sub_c.as<uint32_t>(), (uint32_t)n_sub_out, w.boff, ra.tmp_k, ra.tmp_c, w.n_distinct);
        }
        close_table(0);
        read_tail();
        return removed_sub;
    }
};

}  // namespace

FinishOutcome finish_bucketed(sylph_sketch* sk) {
    sylph_ctx* ctx = sk->ctx;
    const Occurrences occ = sk->occurrences();
    const bool slotted = occ.slotted();                // the sample's one batch, still in its slots (reads.hip)
    // deferred verdict (sketch_session.h PendingSlots): the number of occurrences is not known on the host — geometry from the
    // expectation, capacities from the upper bound, every count the kernels need from device memory, the verdict read with the tail
    const bool deferred = occ.deferred();
    const uint32_t n_cap = occ.n_cap, n_all = occ.n_expect;
    sk->n_out = 0;
    sk->dup_removed = 0;
    if (n_cap == 0) return FinishOutcome::Done;
    if (sk->c < 2) return FinishOutcome::Declined;   // c = 1: valid hashes reach the top bit that marks invalid occurrences
    // bucket geometry: B = n / bucket_target equal hash ranges (replay_plan.h); one-word ranking keys leave room for the largest index
    const BucketMap bm = make_bucket_map(sk->c, n_all, ctx->bucket_target, occ.n_slots);
    const uint32_t B = bm.B;
    // partition geometry: F = 2^fine_bits buckets per coarse range (about 512 ranges), tiles of occurrences
    const PartGeom geom = part_geometry(B);
    // marker-less sample (sketch_session.h): hashes only, counted without occurrence records; tiny samples whose bucket range does
    // not fit the sub-range arithmetic get their records written and take the usual kernels
    if (!slotted && sk->n_plain && !(sk->n_plain == sk->n_occ && bm.composite)) materialise_plain_records(sk);
    const bool plain = !slotted && sk->n_plain != 0;
    // Run-time shape knobs.  SYLPH_HIP_PART_TILE_BLOCKS / SYLPH_HIP_PART_STAGE_PAIRS: seeding blocks per partition tile and pairs the scatter stages
    // in LDS for the slotted sample — round 6 had 16 / 4096 (36.7 KiB of LDS per scatter workgroup, which waits for room beside the seeding kernel).
    static const uint32_t tile_blocks = [] { const char* e = getenv("SYLPH_HIP_PART_TILE_BLOCKS"); return e ? (uint32_t)std::max(1, std::min(32, atoi(e))) : BLK_PER_TILE; }();
    // (2048 pairs: 16 KiB + the range counters, 20 KiB per workgroup; a tile holds ~3,000 occurrences, the rest goes out directly —
    //  pipelined exact set +0.4..0.9 % over 4096 on top of the lean replay, 1536 and 1024 within noise of it: profiles/r07_ab_tail.txt)
    static const uint32_t stage_pairs = [] { const char* e = getenv("SYLPH_HIP_PART_STAGE_PAIRS"); return e ? (uint32_t)std::max(256, std::min(8192, atoi(e))) : 2048u; }();
    PartIn in{};
    in.slotted = slotted ? 1 : 0;
    in.key_sh = bm.sh;
    uint32_t n_tiles;
    const OccRec* recs;
    if (slotted) {
        in.slot_key = sk->slot_key.as<uint32_t>();
        in.n_blk = sk->pend.n_blk;
        in.slot_cap = sk->pend.slot_cap;
        in.blk_count = slot_meta_of(sk, sk->pend.n_blk).blk_count;
        in.blk_per_tile = tile_blocks;
        in.stage_pairs = stage_pairs;
        n_tiles = (in.n_blk + tile_blocks - 1) / tile_blocks;
        recs = sk->slot_rec.as<OccRec>();
    } else {
        in.hash = sk->hash.as<uint64_t>();
        in.n_dense = n_all;
        in.tile_entries = (uint32_t)std::max<uint64_t>(4096, ((uint64_t)n_all + 65535) / 65536);   // at most 65,536 tiles
        n_tiles = (uint32_t)(((uint64_t)n_all + in.tile_entries - 1) / in.tile_entries);
        recs = sk->recs.as<OccRec>();
    }
    DevBuf &b_hist = ctx->scratch[0], &b_pairs = ctx->scratch[1], &b_perm = ctx->scratch[2], &b_tmpk = ctx->scratch[3],
           &b_tmpc = ctx->scratch[4], &b_small = ctx->scratch[5], &b_bk = ctx->scratch[6];
    b_hist.reserve(part_hist_words(geom, n_tiles) * 4);
    b_pairs.reserve((size_t)n_cap * 8);                                 // (bucket, occurrence index) pairs grouped by coarse range
    if (!plain) b_perm.reserve((size_t)n_cap * 4);
    DevBuf& b_sorted = ctx->scratch[7];                                 // marker-less: the hashes sorted by bucket
    if (plain) b_sorted.reserve((size_t)n_cap * 8);
    uint64_t* sorted_hash = plain ? b_sorted.as<uint64_t>() : nullptr;
    in.carry = plain ? 1 : 0;
    b_tmpk.reserve((size_t)n_cap * 8);
    b_tmpc.reserve((size_t)n_cap * 4);
    b_small.reserve(64);                                                // FinishTail (part_hist_kernel clears 16 words)
    const BucketWords w = BucketWords::carve(b_bk, B);
    sk->out_k.reserve((size_t)n_cap * 8);          // upper bound: distinct k-mers <= occurrences
    sk->out_c.reserve((size_t)n_cap * 4);
    // every launch below takes its sizes from device memory; the host synchronises ONCE, at the end (unless some buckets need
    // the list-driven configurations or the device-wide path)
    FinishPass p{sk, ctx, B, w, ReplayArgs{}, b_small.as<FinishTail>(), plain, deferred};
    ReplayArgs& ra = p.ra;
    if (plain) ra.hash = sorted_hash;
    else { ra.recs = recs; ra.perm = b_perm.as<uint32_t>(); }
    ra.boff = w.boff; ra.p_nv = w.boff + B;
    ra.paired = sk->paired; ra.dedup = sk->dedup_mode(); ra.cutoff = sk->paired ? 0u : SINGLE_CUTOFF; ra.bm = bm;
    ra.tmp_k = b_tmpk.as<uint64_t>(); ra.tmp_c = b_tmpc.as<uint32_t>(); ra.n_distinct = w.n_distinct; ra.removed_b = w.removed_b;
    ra.overflow = &p.d_tail->overflow;             // (an address on the device: not read here)
    ra.mid_list = w.mid_list; ra.large_list = w.large_list; ra.ovf_list = w.ovf_list;
    ra.dbg_stage = getenv("SYLPH_REPLAY_STAGE") ? atoi(getenv("SYLPH_REPLAY_STAGE")) : 0;
    {
        HostPhase ph(ctx, "finish(bucket): partition + LDS replay + compact");
        {
            ScopedKernelTimer t(ctx, "sort");   // the partition: what the library's radix sort of (bucket, index) pairs used to do
            launch_partition(ctx, in, bm, geom, n_tiles, n_all, b_hist.as<uint32_t>(), b_pairs.as<uint2>(), w.boff, b_perm.as<uint32_t>(), sorted_hash,
                             w.n_distinct, w.n_zero, b_small.as<uint32_t>(), w.large_list, w.ovf_list, w.mid_list);
        }
        {
            ScopedKernelTimer t(ctx, "replay");
            if (plain) hipLaunchKernelGGL((bucket_count_kernel<CAP_SMALL, RTPB_SMALL>), dim3(B), dim3(RTPB_SMALL), 0, ctx->stream, ra);
            else launch_replay(ctx, B, ra, sk->paired != 0, ra.dbg_stage != 0);
        }
    }
    p.close_table(1);
    p.read_tail();
    const FinishTail& host = p.host;
    // What the three answers mean for the sample is the finish loop's business (finish_plan.h); here they are only told apart, the
    // seeding verdict first: of a batch that was not one for the short-read kernel nothing else in the block means anything.
    if (deferred) {
        if (host.verdict[0] || host.verdict[1]) return FinishOutcome::SeedingBad;
        sk->pend.deferred = false;                 // the verdict is in: from here on an ordinary slotted sample ...
        sk->pend.n = host.n_found;                 // ... whose occurrence count is known (whoever flushes the slots to the dense arrays needs it)
    }
    if (!a10_verdict(sk, host.a10_words)) return FinishOutcome::MarksBad;   // filter dedup: the partitioned pass's marks (a10.hip)
    if (host.overflow) return FinishOutcome::Declined;   // inconsistent bounds (defensive)
    p.count_roads();
    // k-mers more than a thousand deep in a marker-less sample: it takes the usual kernels after all (their overflow path works on
    // records and on the index permutation)
    if (plain && host.n_ovf) return FinishOutcome::NeedsRecords;
    if (host.n_mid || host.n_large) {
        p.run_listed_configurations();
        if (host.overflow) return FinishOutcome::Declined;
    }
    unsigned long long removed_extra = 0;
    if (host.n_ovf) {
        if (ctx->finish_mode == 2 || host.n_ovf > 4096) return FinishOutcome::Declined;
        removed_extra = p.run_overflowing_buckets();
    }
    sk->n_out = host.n_seg;
    sk->dup_removed = host.removed + removed_extra;
    return FinishOutcome::Done;
}

}  // namespace sylph
