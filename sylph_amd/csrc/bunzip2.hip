// bunzip2.hip — bzip2 (.fastq.bz2 / .fasta.bz2, one stream or many) decoded ON THE DEVICE.
//
// The reference reads a bzip2 file through needletail -> libbz2 on the one thread that sketches the sample.  Here the COMPRESSED bytes
// travel and the device does the rest; the bookkeeping and the proof of it are bunzip2_plan.h, the host scaffold shared with inflate.hip
// is decode_host.h.  A bzip2 block is self-contained (no window reaches into the block before it), so the blocks are decoded side by
// side; what is left are the serial chains inside a block:
//
//   scan_kernel       every bit position of the file: the 48-bit block magic -> the CANDIDATES (true block starts + ~0)
//   decode_kernel     one WAVEFRONT per candidate: symbol map, selectors (MTF over the groups, kept in global memory), code lengths,
//                     libbz2's limit/base/perm tables in LDS (6.1 KB per wave); then the one chain that stays serial: Huffman symbols,
//                     RUNA/RUNB runs and the inverse MTF, wave-uniform (bit buffer and state in SGPRs, the 256-entry MTF list in four
//                     VGPRs, moved by a lane shift), the BWT column written 64 bytes at a time.  Reports where the block ended.
//   (host)            chain_step (ChainWalk / SliceWalk): which candidates are the streams' blocks; the stream CRCs
//   hist/cft/scatter  the LF mapping by a stable counting sort per block: 4 KiB chunk histograms, a scan over the chunks, then one
//                     wave per chunk ranks its bytes 64 at a time (8 ballots give the lanes with the same byte) and writes
//                     tt[LF(i)] = i << 8 | byte
//   walk1/rank/walk2  the inverse BWT cut among many walkers: one walker per sampled position (every 256th, and origPtr) follows tt to
//                     the next sampled position; the segments are ranked as a list (one thread per block, in LDS); a second walk
//                     writes every segment's bytes at its offset
//   rlefn/rlescan     the run-length decode as a scan: each 256-byte chunk's map "state in front -> (state behind, bytes out)" for
//                     the 5 states that matter, composed per block (bunzip2_plan.h RleFn) -> every chunk's state and output offset
//   rlewrite          the text, every block at its place in one buffer
//   crc_kernel        CRC-32/BZIP2 of 4 KiB pieces through a table in LDS, shifted to their place by polynomial arithmetic and XORed
//                     into the block's word; the host compares with the block CRCs the stream stores
//
// The candidates are decoded in batches of SYLPH_HIP_BUNZIP2_BATCH (1024) blocks: the scratch is bounded whatever the file's size.  Any
// doubt — a chain that breaks, a CRC that differs, a randomised block, bytes behind the last stream — returns SYLPH_ERR_FORMAT and
// nothing else happens: the caller decodes the file with libbz2 as before.
//
// Two roads run these phases (Bunzip2Phases).  sylph_bunzip2_files: the files whole, the text of all of them in one buffer.
// sylph_bunzip2_stream_*: ONE SLICE of every advancing file's compressed bytes per call, the text handed out window by window, in memory
// bounded by the slice; what a file carries from one call to the next, the cut and the sliced chain walk are bunzip2_stream_plan.h.
#include <algorithm>

#include "bunzip2_plan.h"
#include "bunzip2_stream_plan.h"
#include "decode_host.h"

// What a stream holds between two calls beside decode_host.h's StreamBase: every file's carry.  A bzip2 block needs nothing of the text
// in front of it.
struct sylph_bunzip2_stream : sylph::decode_host::StreamBase {
    using StreamBase::StreamBase;
    std::vector<sylph::bunzip2_stream_plan::Carry> carry = std::vector<sylph::bunzip2_stream_plan::Carry>(files.size());
};

namespace sylph {
namespace {

using namespace bunzip2_plan;
using namespace decode_host;

constexpr uint32_t PAD_BYTES = 64;                 // zero bytes behind the compressed bytes on the device
constexpr uint32_t CHUNK = 4096;                   // bytes per histogram chunk
constexpr uint32_t NCH = (MAX_BLOCK + CHUNK - 1) / CHUNK;
constexpr uint32_t SAMPLE = 256;                   // a walker starts at every SAMPLE-th position of a block (and at origPtr)
constexpr uint32_t MK = MAX_BLOCK / SAMPLE + 2;    // walkers per block at most
constexpr uint32_t NO_MARK = 0xFFFFFFFFu;
constexpr uint32_t RC = 256;                       // bytes per run-length chunk
constexpr uint32_t NRC = (MAX_BLOCK + RC - 1) / RC;
constexpr uint32_t RLE_W = 8;                      // words per run-length chunk: len[5], k_out, then its state and offset in front
constexpr uint32_t PIECE = 4096;                   // bytes per CRC piece

__device__ inline uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

// =================================================================================================================================
// scan: the block magic at every bit position
// =================================================================================================================================
// The bits of the upload that belong to one file: its whole bytes (sylph_bunzip2_files: one entry for all files, which lie back to back
// there) or one SLICE of them (the stream: every advancing file's slice begins at a multiple of 256 bytes, zero bytes between).  A
// candidate starts in [begin_bit, start_end_bit) and has its 48 bits in front of end_bit; a decoder reads no word behind end_bit's.
struct SliceBits { unsigned long long begin_bit, start_end_bit, end_bit; };

__global__ __launch_bounds__(256) void scan_kernel(const uint32_t* __restrict__ w, uint64_t n_words, const SliceBits* __restrict__ lim, uint32_t n_lim,
                                                   unsigned long long* __restrict__ out, uint32_t cap, uint32_t* __restrict__ count) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_words) return;
    // the one slice this word's bits may start a candidate of (slices do not share a word)
    uint64_t lo = 0, hi = 0, end = 0;
    for (uint32_t k = 0; k < n_lim; k++) {
        const SliceBits L = lim[k];
        if (i * 32 + 32 > L.begin_bit && i * 32 < L.start_end_bit) { lo = L.begin_bit; hi = L.start_end_bit; end = L.end_bit; }
    }
    if (lo == hi) return;
    const uint64_t a = ((uint64_t)bswap32(w[i]) << 32) | bswap32(w[i + 1]);     // (the buffer has PAD_BYTES of zeros behind)
    const uint64_t b = (uint64_t)bswap32(w[i + 2]) << 32;
    for (uint32_t o = 0; o < 32; o++) {
        const uint64_t win = o ? (a << o) | (b >> (64 - o)) : a;
        if ((win >> 16) == BLOCK_MAGIC) {
            const uint64_t bit = i * 32 + o;
            if (bit >= lo && bit < hi && bit + 48 <= end) {
                const uint32_t k = atomicAdd(count, 1u);
                if (k < cap) out[k] = bit;
            }
        }
    }
}

// =================================================================================================================================
// decode: one wavefront per candidate
// =================================================================================================================================
struct Bits {                                       // MSB-first bit reader; everything in it is wave-uniform
    const uint32_t* w;
    uint64_t n_words, next, pos;
    uint64_t buf;                                   // left-aligned
    uint32_t cnt;
    __device__ void refill() {                      // cnt <= 32
        const uint32_t v = next < n_words ? bswap32(uni(w[next])) : 0u;
        next++;
        buf |= (uint64_t)v << (32 - cnt);
        cnt += 32;
    }
    __device__ void init(const uint32_t* w_, uint64_t nw, uint64_t bit) {
        w = w_; n_words = nw; next = bit >> 5; buf = 0; cnt = 0; pos = bit;
        refill();
        refill();
        const uint32_t s = (uint32_t)(bit & 31);
        buf <<= s;
        cnt -= s;
    }
    __device__ uint32_t peek(uint32_t k) const { return (uint32_t)(buf >> (64 - k)); }   // 1 <= k <= cnt
    __device__ void skip(uint32_t k) { buf <<= k; cnt -= k; pos += k; }
    __device__ uint32_t get(uint32_t k) {           // 1 <= k <= 32
        if (cnt < k) refill();
        const uint32_t v = peek(k);
        skip(k);
        return v;
    }
};

constexpr int MAX_GROUPS = 6, MAX_ALPHA = 258, MAX_CODE_LEN = 23;

// The wavefront reads the bytes of ITS slice only (lim, as in scan_kernel): words behind the slice's last read as zero, and a block that
// is still going at the slice's last bit reports ST_ERR_OVERRUN there — never a bit of the other mate's slice.
__global__ __launch_bounds__(64) void decode_kernel(const uint32_t* __restrict__ words, const SliceBits* __restrict__ lim, uint32_t n_lim,
                                                    const unsigned long long* __restrict__ cands, uint8_t* __restrict__ ll_base,
                                                    uint8_t* __restrict__ sel_base, BlockReport* __restrict__ rep) {
    __shared__ int32_t s_limit[MAX_GROUPS][24], s_base[MAX_GROUPS][24], s_min[MAX_GROUPS];
    __shared__ uint16_t s_perm[MAX_GROUPS][MAX_ALPHA];
    __shared__ uint8_t s_len[MAX_GROUPS][MAX_ALPHA];
    __shared__ uint8_t s_seq[256];
    const uint32_t lane = threadIdx.x;
    const uint32_t c = blockIdx.x;
    uint8_t* ll = ll_base + (size_t)c * MAX_BLOCK;
    uint8_t* sel = sel_base + (size_t)c * MAX_SELECTORS;
    uint32_t st = ST_OK, crc = 0, rnd = 0, orig = 0, nb = 0, symbols = 0;
    const uint64_t start = cands[c];
    uint64_t n_bits = 0;                            // where the candidate's slice ends (wave-uniform; 0: no slice holds it)
    for (uint32_t k = 0; k < n_lim; k++) {
        const SliceBits L = lim[k];
        if (start >= L.begin_bit && start < L.start_end_bit) n_bits = L.end_bit;
    }
    const uint64_t n_words = (n_bits + 31) / 32;
    Bits b;
    b.init(words, n_words, start);
    {
        const uint64_t m = ((uint64_t)b.get(24) << 24) | b.get(24);
        if (m != BLOCK_MAGIC) { st = ST_ERR_MAGIC; goto done; }
        crc = b.get(32);
        rnd = b.get(1);
        orig = b.get(24);
        // ---- the symbol map: lane l owns byte values 4l .. 4l+3
        const uint32_t used16 = b.get(16);
        uint32_t mine = 0;
        for (uint32_t i = 0; i < 16; i++)
            if ((used16 >> (15 - i)) & 1) {
                const uint32_t w16 = b.get(16);
                if ((lane >> 2) == i) mine = w16;
            }
        uint32_t my_used = 0;
        for (uint32_t j = 0; j < 4; j++) my_used |= ((mine >> (15 - ((lane * 4 + j) & 15))) & 1u) << j;
        uint32_t incl = __popc(my_used);
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        const uint32_t n_in_use = uni(__shfl(incl, 63, 64));
        uint32_t at = incl - __popc(my_used);
        for (uint32_t j = 0; j < 4; j++)
            if ((my_used >> j) & 1) s_seq[at++] = (uint8_t)(lane * 4 + j);
        if (n_in_use == 0) { st = ST_ERR_HEADER; goto done; }
        const uint32_t alpha = n_in_use + 2;
        // ---- selectors, MTF-decoded over the groups
        const uint32_t n_groups = b.get(3);
        if (n_groups < 2 || n_groups > MAX_GROUPS) { st = ST_ERR_HEADER; goto done; }
        const uint32_t n_sel = b.get(15);
        if (n_sel < 1) { st = ST_ERR_HEADER; goto done; }
        if (n_sel > MAX_SELECTORS) { st = ST_ERR_SELECTORS; goto done; }
        uint32_t mtf = 0x543210u;
        for (uint32_t i = 0; i < n_sel; i++) {
            if (b.cnt < 8) b.refill();
            const uint32_t top = b.peek(8);
            const uint32_t j = (uint32_t)__builtin_clz(~(top << 24) | 0u);     // leading ones of the 8 bits (8 when all are set)
            if (j >= n_groups) { st = ST_ERR_HEADER; goto done; }
            b.skip(j + 1);
            const uint32_t v = (mtf >> (4 * j)) & 15u;
            mtf = (mtf & ~((1u << (4 * j + 4)) - 1)) | ((mtf & ((1u << (4 * j)) - 1)) << 4) | v;
            if (lane == 0) sel[i] = (uint8_t)v;
            if (b.pos > n_bits) { st = ST_ERR_OVERRUN; goto done; }
        }
        // ---- code lengths, delta-coded
        for (uint32_t t = 0; t < n_groups; t++) {
            int32_t curr = (int32_t)b.get(5);
            for (uint32_t i = 0; i < alpha; i++) {
                for (;;) {
                    if (curr < 1 || curr > 20) { st = ST_ERR_HEADER; goto done; }
                    if (!b.get(1)) break;
                    curr += b.get(1) ? -1 : 1;
                }
                if (lane == 0) s_len[t][i] = (uint8_t)curr;
            }
            if (b.pos > n_bits) { st = ST_ERR_OVERRUN; goto done; }
        }
        for (uint32_t i = lane; i < MAX_GROUPS * MAX_ALPHA; i += 64) (&s_perm[0][0])[i] = 0;
        __syncthreads();
        // ---- libbz2's decode tables (hbCreateDecodeTables), lane t for group t
        if (lane < n_groups) {
            const uint32_t t = lane;
            int32_t mn = 32, mx = 0;
            for (uint32_t i = 0; i < alpha; i++) { mn = min(mn, (int32_t)s_len[t][i]); mx = max(mx, (int32_t)s_len[t][i]); }
            int32_t pp = 0;
            for (int32_t l = mn; l <= mx; l++)
                for (uint32_t j = 0; j < alpha; j++)
                    if (s_len[t][j] == l) s_perm[t][pp++] = (uint16_t)j;
            int32_t base[24], limit[24];
            for (int i = 0; i < 24; i++) base[i] = limit[i] = 0;
            for (uint32_t i = 0; i < alpha; i++) base[s_len[t][i] + 1]++;
            for (int i = 1; i < MAX_CODE_LEN; i++) base[i] += base[i - 1];
            int32_t vec = 0;
            for (int32_t l = mn; l <= mx; l++) {
                vec += base[l + 1] - base[l];
                limit[l] = vec - 1;
                vec <<= 1;
            }
            for (int32_t l = mn + 1; l <= mx; l++) base[l] = ((limit[l - 1] + 1) << 1) - base[l];
            for (int i = 0; i < 24; i++) { s_limit[t][i] = limit[i]; s_base[t][i] = base[i]; }
            s_min[t] = mn;
        }
        __threadfence_block();
        __syncthreads();
        // ---- the MTF list: list[64 k + lane] in m[k]; it starts as the used byte values in order
        uint32_t m0 = s_seq[lane], m1 = s_seq[64 + lane], m2 = s_seq[128 + lane], m3 = s_seq[192 + lane];
        const uint32_t eob = n_in_use + 1;
        uint32_t group_no = 0, group_pos = 0, gsel = 0, gmin = 0;
        int32_t vlim = 0, vbase = 0;
        uint32_t es = 0, nrun = 1, stage = 0;
        bool first_group = true;
        auto flush_full = [&]() { ll[nb - 64 + lane] = (uint8_t)stage; };
        for (;;) {
            if (group_pos == 0) {
                if (!first_group) group_no++;
                first_group = false;
                if (group_no >= n_sel) { st = ST_ERR_CODE; goto done; }
                group_pos = 50;
                gsel = uni(sel[group_no]);
                vlim = lane < 24 ? s_limit[gsel][lane] : 0;
                vbase = lane < 24 ? s_base[gsel][lane] : 0;
                gmin = uni((uint32_t)s_min[gsel]);
            }
            group_pos--;
            if (b.cnt < 32) b.refill();
            uint32_t zn = gmin;
            int32_t zvec = (int32_t)b.peek(zn);
            for (;;) {
                if (zn > 20) { st = ST_ERR_CODE; goto done; }
                if (zvec <= __builtin_amdgcn_readlane(vlim, zn)) break;
                zn++;
                zvec = (int32_t)b.peek(zn);
            }
            b.skip(zn);
            const int32_t idx = zvec - __builtin_amdgcn_readlane(vbase, zn);
            if (idx < 0 || idx >= MAX_ALPHA) { st = ST_ERR_CODE; goto done; }
            const uint32_t sym = uni(s_perm[gsel][idx]);
            symbols++;
            if (b.pos > n_bits) { st = ST_ERR_OVERRUN; goto done; }
            if (sym <= 1) {                                     // RUNA / RUNB
                if (nrun >= 2u * 1024 * 1024) { st = ST_ERR_SIZE; goto done; }
                es += (sym + 1) * nrun;
                nrun <<= 1;
                continue;
            }
            if (es) {                                           // the run in front: es copies of the list's first byte
                if (nb + es > MAX_BLOCK) { st = ST_ERR_SIZE; goto done; }
                const uint32_t uc = __builtin_amdgcn_readlane(m0, 0);
                while (es) {
                    const uint32_t off = nb & 63, take = min(es, 64 - off);
                    if (lane >= off && lane < off + take) stage = uc;
                    nb += take;
                    es -= take;
                    if ((nb & 63) == 0) flush_full();
                }
                nrun = 1;
            }
            if (sym == eob) break;
            if (nb >= MAX_BLOCK) { st = ST_ERR_SIZE; goto done; }
            // inverse MTF of position nn
            const uint32_t nn = sym - 1, k = nn >> 6, l = nn & 63;
            const uint32_t v = k == 0 ? __builtin_amdgcn_readlane(m0, l) : k == 1 ? __builtin_amdgcn_readlane(m1, l)
                             : k == 2 ? __builtin_amdgcn_readlane(m2, l) : __builtin_amdgcn_readlane(m3, l);
            const uint32_t c1 = __builtin_amdgcn_readlane(m0, 63), c2 = __builtin_amdgcn_readlane(m1, 63), c3 = __builtin_amdgcn_readlane(m2, 63);
            if (k >= 3) { const uint32_t u = __shfl_up(m3, 1, 64); const uint32_t nv = lane == 0 ? c3 : u; if (k > 3 || lane <= l) m3 = nv; }
            if (k >= 2) { const uint32_t u = __shfl_up(m2, 1, 64); const uint32_t nv = lane == 0 ? c2 : u; if (k > 2 || lane <= l) m2 = nv; }
            if (k >= 1) { const uint32_t u = __shfl_up(m1, 1, 64); const uint32_t nv = lane == 0 ? c1 : u; if (k > 1 || lane <= l) m1 = nv; }
            {
                const uint32_t u = __shfl_up(m0, 1, 64);
                const uint32_t nv = lane == 0 ? v : u;
                if (k > 0 || lane <= l) m0 = nv;
            }
            if (lane == (nb & 63)) stage = v;
            nb++;
            if ((nb & 63) == 0) flush_full();
        }
        if (lane < (nb & 63)) ll[(nb & ~63u) + lane] = (uint8_t)stage;
        if (orig >= nb) st = ST_ERR_ORIG;
    }
done:
    if (lane == 0) {
        BlockReport r;
        r.end_bit = b.pos;
        r.status = st;
        r.n = nb;
        r.orig_ptr = orig;
        r.crc = crc;
        r.randomised = rnd;
        r.symbols = symbols;
        rep[c] = r;
    }
}

// =================================================================================================================================
// the inverse BWT
// =================================================================================================================================
struct Job {
    uint32_t slot, n, orig, out_len;   // out_len: filled by rlescan_kernel
    unsigned long long out_off;        // where the block's text goes
};

__global__ __launch_bounds__(256) void hist_kernel(const Job* __restrict__ jobs, const uint8_t* __restrict__ ll_base, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    const Job jb = jobs[blockIdx.y];
    const uint32_t ch = blockIdx.x, t = threadIdx.x;
    h[t] = 0;
    __syncthreads();
    const uint8_t* ll = ll_base + (size_t)jb.slot * MAX_BLOCK;
    const uint32_t a = ch * CHUNK, e = min(jb.n, a + CHUNK);
    for (uint32_t i = a + t; i < e; i += 256) atomicAdd(&h[ll[i]], 1u);
    __syncthreads();
    hist[((size_t)jb.slot * NCH + ch) * 256 + t] = h[t];
}

// per block: the chunks' histograms -> every chunk's first LF slot per byte value (in place)
__global__ __launch_bounds__(256) void cft_kernel(const Job* __restrict__ jobs, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s[256];
    const Job jb = jobs[blockIdx.x];
    const uint32_t v = threadIdx.x, nch = (jb.n + CHUNK - 1) / CHUNK;
    uint32_t* h = hist + (size_t)jb.slot * NCH * 256;
    uint32_t tot = 0;
    for (uint32_t ch = 0; ch < nch; ch++) tot += h[ch * 256 + v];
    s[v] = tot;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t o = v >= d ? s[v - d] : 0;
        __syncthreads();
        s[v] += o;
        __syncthreads();
    }
    uint32_t run = s[v] - tot;
    for (uint32_t ch = 0; ch < nch; ch++) {
        const uint32_t x = h[ch * 256 + v];
        h[ch * 256 + v] = run;
        run += x;
    }
}

// one wave per chunk: a stable rank of its bytes, 64 at a time -> tt[LF(i)] = i << 8 | byte
__global__ __launch_bounds__(256) void scatter_kernel(const Job* __restrict__ jobs, const uint8_t* __restrict__ ll_base, const uint32_t* __restrict__ hist,
                                                      uint32_t* __restrict__ tt_base) {
    __shared__ uint32_t run[4][256];
    const Job jb = jobs[blockIdx.y];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t ch = blockIdx.x * 4 + wv;
    const uint32_t a = ch * CHUNK, e = min(jb.n, a + CHUNK);
    if (a >= e) return;                                          // (whole waves leave: no barrier below)
    const uint32_t* h = hist + ((size_t)jb.slot * NCH + ch) * 256;
    for (uint32_t v = lane; v < 256; v += 64) run[wv][v] = h[v];
    const uint8_t* ll = ll_base + (size_t)jb.slot * MAX_BLOCK;
    uint32_t* tt = tt_base + (size_t)jb.slot * MAX_BLOCK;
    const uint64_t lt = (1ull << lane) - 1;
    for (uint32_t i0 = a; i0 < e; i0 += 64) {
        const uint32_t i = i0 + lane;
        const bool valid = i < e;
        const uint32_t v = valid ? ll[i] : 0u;
        uint64_t mask = __ballot(valid);
        for (uint32_t bit = 0; bit < 8; bit++) {
            const uint64_t bb = __ballot((v >> bit) & 1u);
            mask &= ((v >> bit) & 1u) ? bb : ~bb;
        }
        const uint32_t rank = __popcll(mask & lt);
        const uint32_t pos = valid ? run[wv][v] + rank : 0u;
        if (valid && pos < jb.n) tt[pos] = (i << 8) | v;
        if (valid && rank == 0) run[wv][v] += (uint32_t)__popcll(mask);
    }
}

__device__ inline uint32_t n_marks(uint32_t n, uint32_t orig) { return (n + SAMPLE - 1) / SAMPLE + (orig % SAMPLE ? 1u : 0u); }
__device__ inline uint32_t mark_of(uint32_t pos, uint32_t n, uint32_t orig) {
    return pos % SAMPLE == 0 ? pos / SAMPLE : (pos == orig ? (n + SAMPLE - 1) / SAMPLE : NO_MARK);
}
__device__ inline uint32_t mark_pos(uint32_t m, uint32_t n, uint32_t orig) { return m < (n + SAMPLE - 1) / SAMPLE ? m * SAMPLE : orig; }

// walker m: from its sampled position along tt to the next one -> succ[m], seg[m]
__global__ __launch_bounds__(256) void walk1_kernel(const Job* __restrict__ jobs, const uint32_t* __restrict__ tt_base, uint32_t* __restrict__ succ,
                                                    uint32_t* __restrict__ seg, uint32_t* __restrict__ jstat) {
    const Job jb = jobs[blockIdx.y];
    const uint32_t m = blockIdx.x * 256 + threadIdx.x;
    if (m >= n_marks(jb.n, jb.orig)) return;
    const uint32_t* tt = tt_base + (size_t)jb.slot * MAX_BLOCK;
    uint32_t pos = mark_pos(m, jb.n, jb.orig), len = 0, mk = NO_MARK;
    for (;;) {
        pos = tt[pos] >> 8;
        len++;
        if (pos >= jb.n || len > jb.n) { atomicOr(&jstat[blockIdx.y], 1u); return; }
        mk = mark_of(pos, jb.n, jb.orig);
        if (mk != NO_MARK) break;
    }
    succ[(size_t)jb.slot * MK + m] = mk;
    seg[(size_t)jb.slot * MK + m] = len;
}

// the segments ranked as a list from origPtr's walker: every walker's offset; one cycle through all of them covering the block, or the
// block is declined
__global__ __launch_bounds__(256) void rank_kernel(const Job* __restrict__ jobs, const uint32_t* __restrict__ succ, const uint32_t* __restrict__ seg,
                                                   uint32_t* __restrict__ offs, uint32_t* __restrict__ jstat) {
    __shared__ uint32_t s_succ[MK], s_off[MK];
    __shared__ uint32_t bad;
    const Job jb = jobs[blockIdx.x];
    const uint32_t K = n_marks(jb.n, jb.orig);
    const size_t base = (size_t)jb.slot * MK;
    if (threadIdx.x == 0) bad = jstat[blockIdx.x];
    for (uint32_t m = threadIdx.x; m < K; m += 256) { s_succ[m] = succ[base + m]; s_off[m] = NO_MARK; }
    __syncthreads();
    if (threadIdx.x == 0 && !bad) {
        uint32_t m = mark_of(jb.orig, jb.n, jb.orig), off = 0;
        for (uint32_t step = 0; step < K; step++) {
            if (m >= K || s_off[m] != NO_MARK) { bad = 1; break; }
            s_off[m] = off;
            off += seg[base + m];
            m = s_succ[m];
        }
        if (!bad && (m != mark_of(jb.orig, jb.n, jb.orig) || off != jb.n)) bad = 1;
        if (bad) jstat[blockIdx.x] |= 2u;
    }
    __syncthreads();
    if (bad) return;
    for (uint32_t m = threadIdx.x; m < K; m += 256) offs[base + m] = s_off[m];
}

// walker m again, writing its segment's bytes at its offset (over the BWT column, which is no longer needed)
__global__ __launch_bounds__(256) void walk2_kernel(const Job* __restrict__ jobs, const uint32_t* __restrict__ tt_base, const uint32_t* __restrict__ seg,
                                                    const uint32_t* __restrict__ offs, const uint32_t* __restrict__ jstat, uint8_t* __restrict__ pre_base) {
    const Job jb = jobs[blockIdx.y];
    const uint32_t m = blockIdx.x * 256 + threadIdx.x;
    if (jstat[blockIdx.y] || m >= n_marks(jb.n, jb.orig)) return;
    const uint32_t* tt = tt_base + (size_t)jb.slot * MAX_BLOCK;
    uint8_t* pre = pre_base + (size_t)jb.slot * MAX_BLOCK;
    const uint32_t len = seg[(size_t)jb.slot * MK + m], o = offs[(size_t)jb.slot * MK + m];
    uint32_t pos = mark_pos(m, jb.n, jb.orig);
    for (uint32_t t = 0; t < len; t++) {
        const uint32_t e = tt[pos];
        pre[o + t] = (uint8_t)e;
        pos = e >> 8;
    }
}

// =================================================================================================================================
// the run-length decode
// =================================================================================================================================
__global__ __launch_bounds__(256) void rlefn_kernel(const Job* __restrict__ jobs, const uint8_t* __restrict__ pre_base, const uint32_t* __restrict__ jstat,
                                                    uint32_t* __restrict__ rle) {
    const Job jb = jobs[blockIdx.y];
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    const uint32_t a = c * RC;
    if (jstat[blockIdx.y] || a >= jb.n) return;
    const RleFn f = rle_fn(pre_base + (size_t)jb.slot * MAX_BLOCK + a, min(RC, jb.n - a));
    uint32_t* o = rle + ((size_t)jb.slot * NRC + c) * RLE_W;
    for (int k = 0; k < 5; k++) o[k] = f.len[k];
    o[5] = f.k_out;
}

// per block: thread t composes a range of chunks for every state in front; thread 0 chains the ranges; every chunk gets its state
// and offset in front; the block's text length
__global__ __launch_bounds__(256) void rlescan_kernel(Job* __restrict__ jobs, const uint8_t* __restrict__ pre_base, uint32_t* __restrict__ rle,
                                                      uint32_t* __restrict__ jstat) {
    __shared__ uint32_t s_len[256][5], s_k[256], s_in_k[256], s_in_off[256];
    __shared__ uint32_t bad;
    Job& jb = jobs[blockIdx.x];
    const uint32_t t = threadIdx.x, n = jb.n;
    if (t == 0) bad = jstat[blockIdx.x];
    __syncthreads();
    if (bad) return;
    const uint8_t* pre = pre_base + (size_t)jb.slot * MAX_BLOCK;
    uint32_t* fn = rle + (size_t)jb.slot * NRC * RLE_W;
    const uint32_t nrc = (n + RC - 1) / RC, per = (nrc + 255) / 256;
    const uint32_t c0 = min(nrc, t * per), c1 = min(nrc, c0 + per);
    uint32_t kpack = 0;
    for (uint32_t k0 = 0; k0 < 5; k0++) {
        uint32_t k = k0, tot = 0;
        for (uint32_t c = c0; c < c1; c++) {
            const uint32_t* f = fn + (size_t)c * RLE_W;
            tot += f[k];
            const uint32_t ko = (f[5] >> (3 * k)) & 7;
            k = c + 1 < c1 ? rle_eff(ko, pre[min(n, (c + 1) * RC) - 1], pre[(c + 1) * RC]) : ko;
        }
        s_len[t][k0] = tot;
        kpack |= k << (3 * k0);
    }
    s_k[t] = kpack;
    __syncthreads();
    if (t == 0) {
        uint32_t k = 0, off = 0;
        for (uint32_t r = 0; r < 256; r++) {
            const uint32_t a0 = min(nrc, r * per), a1 = min(nrc, a0 + per);
            s_in_k[r] = k;
            s_in_off[r] = off;
            if (a0 == a1) continue;
            off += s_len[r][k];
            const uint32_t ko = (s_k[r] >> (3 * k)) & 7;
            k = a1 < nrc ? rle_eff(ko, pre[a1 * RC - 1], pre[a1 * RC]) : ko;
        }
        if (k == 4) { bad = 1; jstat[blockIdx.x] |= 4u; }        // a repeat count is due behind the block's last byte: libbz2 declines it
        jb.out_len = off;
    }
    __syncthreads();
    if (bad) return;
    uint32_t k = s_in_k[t], off = s_in_off[t];
    for (uint32_t c = c0; c < c1; c++) {
        uint32_t* f = fn + (size_t)c * RLE_W;
        f[6] = k;
        f[7] = off;
        off += f[k];
        const uint32_t ko = (f[5] >> (3 * k)) & 7;
        if (c + 1 < nrc) k = rle_eff(ko, pre[min(n, (c + 1) * RC) - 1], pre[(c + 1) * RC]);
    }
}

__global__ __launch_bounds__(256) void rlewrite_kernel(const Job* __restrict__ jobs, const uint8_t* __restrict__ pre_base, const uint32_t* __restrict__ rle,
                                                       uint8_t* __restrict__ text) {
    const Job jb = jobs[blockIdx.y];
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    const uint32_t a = c * RC;
    if (a >= jb.n) return;
    const uint8_t* pre = pre_base + (size_t)jb.slot * MAX_BLOCK;
    const uint32_t* f = rle + ((size_t)jb.slot * NRC + c) * RLE_W;
    rle_expand(pre + a, min(RC, jb.n - a), f[6], a ? pre[a - 1] : 0, text + jb.out_off + f[7]);
}

// =================================================================================================================================
// CRC-32/BZIP2 of every block's text
// =================================================================================================================================
__global__ __launch_bounds__(256) void crc_kernel(const Job* __restrict__ jobs, const uint8_t* __restrict__ text, const uint32_t* __restrict__ table,
                                                  const uint32_t* __restrict__ x2n, uint32_t* __restrict__ raw) {
    __shared__ uint32_t t[256];
    t[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const Job jb = jobs[blockIdx.y];
    const uint64_t a = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * PIECE;
    if (a >= jb.out_len) return;
    const uint64_t e = a + PIECE < jb.out_len ? a + PIECE : (uint64_t)jb.out_len;
    const uint8_t* p = text + jb.out_off;
    uint32_t reg = 0;
    for (uint64_t i = a; i < e; i++) reg = (reg << 8) ^ t[(reg >> 24) ^ p[i]];
    atomicXor(&raw[blockIdx.y], crc_shift(x2n, reg, jb.out_len - e));
}

// =================================================================================================================================
// host
// =================================================================================================================================
uint32_t batch_size() {
    if (const char* e = getenv("SYLPH_HIP_BUNZIP2_BATCH")) { const long v = atol(e); if (v >= 1) return (uint32_t)std::min<long>(v, 1 << 16); }
    return 1024;
}

// The device phases of both roads (sylph_bunzip2_files: the files whole; sylph_bunzip2_stream_next: one slice per advancing file), in
// the order they run.  The candidates are decoded in batches, in bit order, and the chains are walked as their reports come in: each
// turn finishes the chain blocks of the batch in hand, then decodes the next batch.  The scratch does not depend on the file.
struct PendingBlock { size_t cand; uint32_t n, file; };     // a chain block of the batch in hand: its candidate, BWT bytes, file
struct Bunzip2Phases {
    sylph_ctx* ctx;
    hipStream_t s;
    uint64_t total = 0, n_words = 0;                    // bytes of the upload, and the words that hold them
    std::vector<SliceBits> lim;                         // whose bits they are
    DevBuf d_in{ctx}, d_lim{ctx}, d_cand{ctx}, d_count{ctx}, d_ll{ctx}, d_sel{ctx}, d_rep{ctx}, d_tt{ctx}, d_hist{ctx}, d_succ{ctx}, d_seg{ctx}, d_offs{ctx}, d_rle{ctx},
        d_jobs{ctx}, d_jstat{ctx}, d_raw{ctx}, d_tab{ctx}, d_x2n{ctx};
    std::vector<uint64_t> cand;                         // sorted candidate bits
    uint32_t B = 1;                                     // candidates per batch
    uint32_t x2n[64];
    std::vector<BlockReport> rep;                       // per candidate; those of [0, have) are known
    size_t have = 0, batch_first = 0, done_blocks = 0;
    std::vector<Job> jobs;                              // the chain blocks of the batch in hand
    std::vector<uint32_t> stored_crc;                   // ... and the CRCs their headers store
    uint32_t max_len = 0;                               // the longest of their texts

    explicit Bunzip2Phases(sylph_ctx* c) : ctx(c), s(c->stream) {}

    uint64_t scratch_bytes() const {
        uint64_t b = 0;
        for (const DevBuf* d : {&d_in, &d_lim, &d_cand, &d_count, &d_ll, &d_sel, &d_rep, &d_tt, &d_hist, &d_succ, &d_seg, &d_offs, &d_rle, &d_jobs, &d_jstat, &d_raw, &d_tab, &d_x2n})
            b += d->cap;
        return b;
    }

    // ---- room for the compressed bytes (the caller uploads them, zero from the last one to PAD_BYTES behind the last whole word)
    uint8_t* input(uint64_t bytes) {
        total = bytes;
        n_words = (bytes + 3) / 4;
        d_in.reserve(n_words * 4 + PAD_BYTES);
        return (uint8_t*)d_in.p;
    }

    // ---- the candidates: every block magic whose bits lie in one entry of `lim`
    void find_candidates(const char* phase) {
        d_lim.reserve(std::max<size_t>(lim.size(), 1) * sizeof(SliceBits));
        if (!lim.empty()) ctx->h2d(d_lim.p, lim.data(), lim.size() * sizeof(SliceBits));
        const uint32_t cap = (uint32_t)std::min<uint64_t>(total / 8 + 64, 0xFFFFFFF0ull);
        d_cand.reserve((size_t)cap * 8);
        d_count.reserve(4);
        {
            ScopedKernelTimer kt(ctx, "bunzip2_scan");
            HostPhase hp(ctx, phase);
            SY_HIP(hipMemsetAsync(d_count.p, 0, 4, s));
            if (n_words) {
                hipLaunchKernelGGL(scan_kernel, dim3((uint32_t)((n_words + 255) / 256)), dim3(256), 0, s, d_in.as<uint32_t>(), n_words, d_lim.as<SliceBits>(),
                                   (uint32_t)lim.size(), d_cand.as<unsigned long long>(), cap, d_count.as<uint32_t>());
                SY_HIP(hipGetLastError());
            }
            cand = fetch_candidates(ctx, d_cand.p, d_count.as<uint32_t>(), cap, "more block magics than the candidate list holds");
        }
        if (!cand.empty()) ctx->h2d(d_cand.p, cand.data(), cand.size() * 8);
        rep.resize(cand.size());
        B = std::max<uint32_t>(1, std::min<uint32_t>(batch_size(), std::max<uint32_t>((uint32_t)cand.size(), 1)));
    }

    void upload_crc_tables() {
        uint32_t table[256];
        crc_x2n_table(x2n);
        crc_byte_table(table);
        d_x2n.reserve(sizeof(x2n));
        d_tab.reserve(sizeof(table));
        ctx->h2d(d_x2n.p, x2n, sizeof(x2n));
        ctx->h2d(d_tab.p, table, sizeof(table));
    }

    // ---- the chain blocks of the batch in hand: inverse BWT (LF mapping, walks) and the run-length functions -> every block's length
    void invert_batch(const std::vector<PendingBlock>& pend) {
        const uint32_t J = (uint32_t)pend.size();
        jobs.resize(J);
        stored_crc.resize(J);
        for (uint32_t j = 0; j < J; j++) {
            jobs[j] = Job{(uint32_t)(pend[j].cand - batch_first), pend[j].n, rep[pend[j].cand].orig_ptr, 0, 0};
            stored_crc[j] = rep[pend[j].cand].crc;
        }
        d_jobs.reserve((size_t)J * sizeof(Job));
        d_jstat.reserve((size_t)J * 4);
        d_raw.reserve((size_t)J * 4);
        d_hist.reserve((size_t)B * NCH * 256 * 4);
        d_tt.reserve((size_t)B * MAX_BLOCK * 4);
        d_succ.reserve((size_t)B * MK * 4);
        d_seg.reserve((size_t)B * MK * 4);
        d_offs.reserve((size_t)B * MK * 4);
        d_rle.reserve((size_t)B * NRC * RLE_W * 4);
        ctx->h2d(d_jobs.p, jobs.data(), (size_t)J * sizeof(Job));
        SY_HIP(hipMemsetAsync(d_jstat.p, 0, (size_t)J * 4, s));
        Job* dj = d_jobs.as<Job>();
        {
            ScopedKernelTimer kt(ctx, "bunzip2_bwt");
            HostPhase hp(ctx, "bunzip2: LF mapping");
            hipLaunchKernelGGL(hist_kernel, dim3(NCH, J), dim3(256), 0, s, dj, d_ll.as<uint8_t>(), d_hist.as<uint32_t>());
            hipLaunchKernelGGL(cft_kernel, dim3(J), dim3(256), 0, s, dj, d_hist.as<uint32_t>());
            hipLaunchKernelGGL(scatter_kernel, dim3((NCH + 3) / 4, J), dim3(256), 0, s, dj, d_ll.as<uint8_t>(), d_hist.as<uint32_t>(), d_tt.as<uint32_t>());
            SY_HIP(hipGetLastError());
        }
        {
            ScopedKernelTimer kt(ctx, "bunzip2_walk");
            HostPhase hp(ctx, "bunzip2: walks");
            hipLaunchKernelGGL(walk1_kernel, dim3((MK + 255) / 256, J), dim3(256), 0, s, dj, d_tt.as<uint32_t>(), d_succ.as<uint32_t>(), d_seg.as<uint32_t>(),
                               d_jstat.as<uint32_t>());
            hipLaunchKernelGGL(rank_kernel, dim3(J), dim3(256), 0, s, dj, d_succ.as<uint32_t>(), d_seg.as<uint32_t>(), d_offs.as<uint32_t>(), d_jstat.as<uint32_t>());
            hipLaunchKernelGGL(walk2_kernel, dim3((MK + 255) / 256, J), dim3(256), 0, s, dj, d_tt.as<uint32_t>(), d_seg.as<uint32_t>(), d_offs.as<uint32_t>(),
                               d_jstat.as<uint32_t>(), d_ll.as<uint8_t>());
            SY_HIP(hipGetLastError());
        }
        {
            ScopedKernelTimer kt(ctx, "bunzip2_rle");
            HostPhase hp(ctx, "bunzip2: run lengths");
            hipLaunchKernelGGL(rlefn_kernel, dim3((NRC + 255) / 256, J), dim3(256), 0, s, dj, d_ll.as<uint8_t>(), d_jstat.as<uint32_t>(), d_rle.as<uint32_t>());
            hipLaunchKernelGGL(rlescan_kernel, dim3(J), dim3(256), 0, s, dj, d_ll.as<uint8_t>(), d_rle.as<uint32_t>(), d_jstat.as<uint32_t>());
            SY_HIP(hipGetLastError());
        }
        std::vector<uint32_t> jstat(J);
        ctx->d2h(jstat.data(), d_jstat.p, (size_t)J * 4);
        ctx->d2h(jobs.data(), d_jobs.p, (size_t)J * sizeof(Job));
        max_len = 0;
        for (uint32_t j = 0; j < J; j++) {
            if (jstat[j]) throw FormatDecline{"block " + std::to_string(done_blocks + j) + ": inverse BWT / run lengths do not add up (" + std::to_string(jstat[j]) + ")"};
            max_len = std::max(max_len, jobs[j].out_len);
        }
    }

    // ---- every block of the batch is written at the place the caller gave it (Job::out_off, in `text`)
    void write_batch_text(uint8_t* text) {
        const uint32_t J = (uint32_t)jobs.size();
        ctx->h2d(d_jobs.p, jobs.data(), (size_t)J * sizeof(Job));
        ScopedKernelTimer kt(ctx, "bunzip2_rle");
        HostPhase hp(ctx, "bunzip2: text");
        hipLaunchKernelGGL(rlewrite_kernel, dim3((NRC + 255) / 256, J), dim3(256), 0, s, d_jobs.as<Job>(), d_ll.as<uint8_t>(), d_rle.as<uint32_t>(), text);
        SY_HIP(hipGetLastError());
    }

    // ---- CRC-32/BZIP2 of every block of the batch, against the one its header stores
    void check_batch_crcs(const uint8_t* text) {
        const uint32_t J = (uint32_t)jobs.size();
        std::vector<uint32_t> raw(J);
        {
            ScopedKernelTimer kt(ctx, "bunzip2_crc");
            HostPhase hp(ctx, "bunzip2: crc");
            SY_HIP(hipMemsetAsync(d_raw.p, 0, (size_t)J * 4, s));
            const uint32_t gx = (uint32_t)(((uint64_t)max_len + (uint64_t)PIECE * 256 - 1) / ((uint64_t)PIECE * 256));
            if (gx) {
                hipLaunchKernelGGL(crc_kernel, dim3(gx, J), dim3(256), 0, s, d_jobs.as<Job>(), text, d_tab.as<uint32_t>(), d_x2n.as<uint32_t>(), d_raw.as<uint32_t>());
                SY_HIP(hipGetLastError());
            }
            ctx->d2h(raw.data(), d_raw.p, (size_t)J * 4);
        }
        for (uint32_t j = 0; j < J; j++) {
            const uint32_t stored = stored_crc[j], got = crc_finish(x2n, raw[j], jobs[j].out_len);
            if (got != stored) {
                char msg[160];
                snprintf(msg, sizeof(msg), "block %zu: CRC %08x, the stream says %08x", done_blocks + j, got, stored);
                throw FormatDecline{msg};
            }
        }
        done_blocks += J;
    }

    // ---- the next batch of candidates: one wavefront each, the BWT columns and the reports
    void decode_next_batch() {
        const uint32_t cnt = (uint32_t)std::min<size_t>(B, cand.size() - have);
        if (!cnt) throw FormatDecline{"the chain needs a candidate that is not there"};
        batch_first = have;
        d_ll.reserve((size_t)B * MAX_BLOCK);
        d_sel.reserve((size_t)B * MAX_SELECTORS);
        d_rep.reserve((size_t)B * sizeof(BlockReport));
        {
            ScopedKernelTimer kt(ctx, "bunzip2_decode");
            HostPhase hp(ctx, "bunzip2: decode");
            hipLaunchKernelGGL(decode_kernel, dim3(cnt), dim3(64), 0, s, d_in.as<uint32_t>(), d_lim.as<SliceBits>(), (uint32_t)lim.size(),
                               d_cand.as<unsigned long long>() + batch_first, d_ll.as<uint8_t>(), d_sel.as<uint8_t>(), d_rep.as<BlockReport>());
            SY_HIP(hipGetLastError());
        }
        ctx->d2h(rep.data() + batch_first, d_rep.p, (size_t)cnt * sizeof(BlockReport));
        have += cnt;
    }
};

// sylph_bunzip2_files: the files whole, back to back; one chain through all of them; the whole text in one buffer that grows
struct Bunzip2Call : Bunzip2Phases {
    sylph_inflated* t;
    const Segments segs;
    ChainWalk walk;
    size_t taken = 0;                                   // chain blocks handed to the phases so far
    std::vector<uint64_t> blk_off, blk_len;             // every chain block's text
    TextBuf text{"hipMalloc (bzip2 text)"};
    uint64_t used = 0;

    Bunzip2Call(sylph_inflated* t_, Segments&& g) : Bunzip2Phases(t_->ctx), t(t_), segs(std::move(g)) {}

    void upload() {
        upload_segments(ctx, input(segs.total()), segs, PAD_BYTES);
        lim.assign(1, SliceBits{0, total * 8, total * 8});
    }

    // ---- every block of the batch gets its place behind the text so far
    void place_batch() {
        const size_t first = blk_off.size();
        for (Job& jb : jobs) {
            jb.out_off = used;
            blk_off.push_back(used);
            blk_len.push_back(jb.out_len);
            used += jb.out_len;
        }
        text.grow(used, blk_off[first], s);
    }

    // ---- the handle: the text, the counts, every file's range (a file's blocks are consecutive in the chain)
    void fill_handle() {
        SY_HIP(hipMemsetAsync(text.text() + used, 0, 256, s));
        t->buf = text.release();
        t->n = used;
        t->n_members = walk.n_streams;
        t->n_blocks = walk.blocks.size();
        t->n_candidates = have;
        t->n_host_members = 0;
        t->files.assign(segs.ptr.size(), {0, 0});
        uint64_t at = 0;
        size_t bi = 0;
        for (uint32_t f = 0; f < segs.ptr.size(); f++) {
            const uint64_t begin = at;
            while (bi < walk.blocks.size() && walk.blocks[bi].file == f) { at = blk_off[bi] + blk_len[bi]; bi++; }
            t->files[f] = {begin, at};
        }
    }
};

void bunzip2_impl(sylph_inflated* t, const void* const* bzs, const uint64_t* n_bytes, uint32_t n_files) {
    sylph_ctx* ctx = t->ctx;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard dg(ctx->device);
    Segments segs = segments_of(bzs, n_bytes, n_files);
    for (uint32_t i = 0; i < n_files; i++) {
        if (!n_bytes[i]) throw FormatDecline{"file " + std::to_string(i) + " is empty"};
        if (!stream_level(segs.ptr[i], n_bytes[i], 0)) throw FormatDecline{"file " + std::to_string(i) + " does not begin with a bzip2 stream header"};
    }
    if (segs.total() >= ctx->bunzip2_whole_max_bytes) throw FormatDecline{"more bzip2 bytes than \"bunzip2_whole_max_bytes\" allows in one piece"};
    Bunzip2Call c(t, std::move(segs));
    c.upload();
    c.find_candidates("bunzip2: scan");
    c.upload_crc_tables();
    c.walk.start(&c.segs, &c.cand);
    c.text.grow(std::max<uint64_t>(c.total * 5, 1u << 20), 0, c.s);
    std::vector<PendingBlock> pend;
    for (;;) {
        const bool fin = c.walk.step(c.rep.data(), c.have);
        if (!c.walk.why.empty()) throw FormatDecline{c.walk.why};
        if (c.walk.blocks.size() > c.taken) {
            pend.clear();
            for (; c.taken < c.walk.blocks.size(); c.taken++) pend.push_back(PendingBlock{c.walk.blocks[c.taken].cand, c.walk.blocks[c.taken].n, c.walk.blocks[c.taken].file});
            c.invert_batch(pend);
            c.place_batch();
            c.write_batch_text(c.text.text());
            c.check_batch_crcs(c.text.text());
        }
        if (fin) break;
        c.decode_next_batch();
    }
    c.fill_handle();
    SY_HIP(hipStreamSynchronize(c.s));
}

// =================================================================================================================================
// the stream: the same phases over one slice per advancing file (bookkeeping: bunzip2_stream_plan.h)
// =================================================================================================================================
using namespace bunzip2_stream_plan;

struct StreamCall : Bunzip2Phases {
    sylph_bunzip2_stream* st;
    sylph_inflated* t;
    const uint8_t* advance;
    const uint64_t* keep_from;
    struct FileSlice { uint32_t file; SliceCut sc; uint64_t off; size_t cand_lo = 0, cand_hi = 0; };   // off: where the slice's bytes lie in the upload
    std::vector<FileSlice> slices;                  // in file order
    std::vector<int> slice_of_file;
    std::vector<std::vector<uint64_t>> cand_bits;   // per slice: its candidates, in bits of the FILE
    std::vector<SliceWalk> walks;                   // per slice
    std::vector<PendingBlock> pend;
    TextBuf text{"hipMalloc (bzip2 window)"};
    std::vector<uint64_t> kept, text_off;           // per file: kept bytes of the previous window; where the file's window begins
    std::vector<uint32_t> tails;                    // files whose kept tail has a place and is not copied yet
    uint32_t cur = 0;                               // the file whose window is being laid out (those before it are closed)
    bool cur_open = false;
    uint64_t used = 0;

    StreamCall(sylph_bunzip2_stream* st_, sylph_inflated* t_, const uint8_t* adv, const uint64_t* keep)
        : Bunzip2Phases(st_->ctx), st(st_), t(t_), advance(adv), keep_from(keep) {}

    uint32_t n_files() const { return st->n_files(); }

    void plan_slices() {
        const uint32_t F = n_files();
        kept = kept_tails(st, keep_from, "sylph_bunzip2_stream");
        text_off.assign(F + 1, 0);
        slice_of_file.assign(F, -1);
        uint64_t at = 0;
        for (uint32_t f = 0; f < F; f++) {
            if ((advance && !advance[f]) || st->carry[f].finished) continue;
            const SliceCut sc = slice_cut(st->carry[f], st->n_bytes[f], st->slice_bytes);
            at = slice_begin(at);
            slice_of_file[f] = (int)slices.size();
            slices.push_back(FileSlice{f, sc, at});
            at += sc.end - sc.pos;
        }
        uint8_t* in = input(at);
        HostPhase hp(ctx, "bunzip2 stream: upload");
        SY_HIP(hipMemsetAsync(in, 0, n_words * 4 + PAD_BYTES, s));
        lim.clear();
        for (const FileSlice& fs : slices) {
            if (fs.sc.end > fs.sc.pos) ctx->h2d(in + fs.off, st->files[fs.file] + fs.sc.pos, (size_t)(fs.sc.end - fs.sc.pos));
            // (a block that starts at or behind the cut is the next slice's: it is neither looked for nor decoded here)
            const uint64_t starts = fs.sc.cut < st->n_bytes[fs.file] ? fs.sc.cut : fs.sc.end;
            lim.push_back(SliceBits{fs.off * 8, (fs.off + (starts - fs.sc.pos)) * 8, (fs.off + (fs.sc.end - fs.sc.pos)) * 8});
        }
    }

    // every slice's candidates in bits of its file, and its walk from the file's carry
    void start_walks() {
        cand_bits.assign(slices.size(), {});
        walks.assign(slices.size(), SliceWalk{});
        for (size_t si = 0; si < slices.size(); si++) {
            FileSlice& fs = slices[si];
            const int64_t shift = (int64_t)(fs.sc.pos * 8) - (int64_t)(fs.off * 8);
            fs.cand_lo = (size_t)(std::lower_bound(cand.begin(), cand.end(), lim[si].begin_bit) - cand.begin());
            fs.cand_hi = (size_t)(std::lower_bound(cand.begin(), cand.end(), lim[si].end_bit) - cand.begin());
            for (size_t i = fs.cand_lo; i < fs.cand_hi; i++) cand_bits[si].push_back((uint64_t)((int64_t)cand[i] + shift));
            walks[si].start(st->files[fs.file], st->n_bytes[fs.file], fs.file, st->carry[fs.file], fs.sc, &cand_bits[si], shift);
        }
    }

    // follow every slice's chain as far as the reports in hand allow -> pend: the blocks that joined, in file order.  true: all walked.
    bool walk_chains() {
        pend.clear();
        bool all = true;
        for (size_t si = 0; si < slices.size(); si++) {
            const FileSlice& fs = slices[si];
            SliceWalk& w = walks[si];
            const size_t before = w.blocks.size();
            w.step(rep.data() + fs.cand_lo, std::min(std::max(have, fs.cand_lo), fs.cand_hi) - fs.cand_lo);
            if (!w.why.empty()) throw FormatDecline{"file " + std::to_string(fs.file) + ": " + w.why};
            for (size_t i = before; i < w.blocks.size(); i++) pend.push_back(PendingBlock{fs.cand_lo + w.blocks[i].cand, w.blocks[i].n, fs.file});
            all = all && w.ended;
        }
        return all;
    }

    // ---- where everything goes in the window's text: per file, the kept tail of its previous window, then the slice's blocks.  A file's
    // window begins where the one before it ends, so it is laid out once every earlier file's chain is walked — which it is before a
    // report of its own can be there: the candidates are decoded in bit order, and file i's slice lies in front of file i + 1's.
    void place_batch() {
        const uint32_t F = n_files();
        const uint64_t before = used;
        size_t j = 0;
        while (cur < F) {
            if (!cur_open) {
                text_off[cur] = used;
                if (kept[cur]) tails.push_back(cur);
                used += kept[cur];
                cur_open = true;
            }
            for (; j < pend.size() && pend[j].file == cur; j++) { jobs[j].out_off = used; used += jobs[j].out_len; }
            if (slice_of_file[cur] >= 0 && !walks[slice_of_file[cur]].ended) break;
            text_off[++cur] = used;
            cur_open = false;
        }
        SY_REQUIRE(j == pend.size(), "sylph_bunzip2_stream_next: a block of file %u came in front of its file's window", j < pend.size() ? pend[j].file : 0u);
        text.grow(std::max<uint64_t>(used, 1), before, s);
        for (uint32_t f : tails) SY_HIP(hipMemcpyAsync(text.text() + text_off[f], st->prev_text[f] + keep_from[f], kept[f], hipMemcpyDeviceToDevice, s));
        tails.clear();
    }

    void fill_handle() {
        SY_HIP(hipMemsetAsync(text.text() + used, 0, 256, s));
        t->n = used;
        t->n_candidates = have;
        t->n_host_members = 0;
        t->files.clear();
        for (uint32_t f = 0; f < n_files(); f++) t->files.push_back({text_off[f], text_off[f + 1]});
        for (size_t si = 0; si < slices.size(); si++) {
            t->n_blocks += walks[si].blocks.size();
            t->n_members += walks[si].next.pos.n_streams - st->carry[slices[si].file].pos.n_streams;
        }
    }

    // ---- what the next call needs: every advanced file's carry
    void commit() {
        for (size_t si = 0; si < slices.size(); si++) {
            st->carry[slices[si].file] = walks[si].next;
            st->n_slices++;
        }
        uint64_t kept_all = 0;
        for (uint64_t k : kept) kept_all += k;
        st->text_bytes += used - kept_all;
        st->peak_scratch = std::max(st->peak_scratch, scratch_bytes());
        st->peak_window = std::max(st->peak_window, used);
    }
};

void stream_next_impl(sylph_bunzip2_stream* st, sylph_inflated* t, const uint8_t* advance, const uint64_t* keep_from) {
    sylph_ctx* ctx = st->ctx;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard dg(ctx->device);
    StreamCall c(st, t, advance, keep_from);
    // (on every way out — a decline included — the stream is idle before the scratch goes back to the pool; destroyed before `c`)
    struct Done { hipStream_t st; ~Done() { (void)hipStreamSynchronize(st); } } done{ctx->stream};
    c.plan_slices();
    if (!c.slices.empty()) {
        c.find_candidates("bunzip2 stream: scan");
        c.upload_crc_tables();
        c.start_walks();
        uint64_t guess = 0;
        for (const auto& fs : c.slices) guess += (fs.sc.cut - fs.sc.pos) * 5;
        for (uint64_t k : c.kept) guess += k;
        c.text.grow(std::max<uint64_t>(guess, 1u << 20), 0, c.s);
    }
    for (;;) {
        const bool all = c.walk_chains();
        if (!c.pend.empty()) c.invert_batch(c.pend);
        else c.jobs.clear();
        c.place_batch();
        if (!c.pend.empty()) {
            c.write_batch_text(c.text.text());
            c.check_batch_crcs(c.text.text());
        }
        if (all) break;
        c.decode_next_batch();
    }
    c.fill_handle();
    c.commit();
    t->buf = c.text.release();
    SY_HIP(hipStreamSynchronize(ctx->stream));
    remember_window(st, t, c.text_off);
}

}  // namespace
}  // namespace sylph

using namespace sylph;

extern "C" {

int sylph_bunzip2_files(sylph_ctx* ctx, const void* const* bz, const uint64_t* n_bytes, uint32_t n_files, int mem, sylph_inflated** out) {
    return decode_entry("sylph_bunzip2", true, ctx, bz, n_bytes, n_files, mem, out, bunzip2_impl);
}

int sylph_bunzip2(sylph_ctx* ctx, const void* bz, uint64_t n_bytes, int mem, sylph_inflated** out) {
    return sylph_bunzip2_files(ctx, &bz, &n_bytes, 1, mem, out);
}

int sylph_bunzip2_stream_open(sylph_ctx* ctx, const void* const* bz, const uint64_t* n_bytes, uint32_t n_files, int mem, uint64_t slice_bytes,
                              sylph_bunzip2_stream** out) {
    if (const int rc = stream_open_args("sylph_bunzip2_stream", ctx, bz, n_bytes, n_files, mem, out)) return rc;
    for (uint32_t i = 0; i < n_files; i++)
        if (!bunzip2_plan::stream_level((const uint8_t*)bz[i], n_bytes[i], 0)) { set_error("sylph_bunzip2_stream_open: declined: file %u does not begin with a bzip2 stream header", i); return SYLPH_ERR_FORMAT; }
    sylph_bunzip2_stream* st = nullptr;
    const int rc = guarded([&] {
        if (!slice_bytes) slice_bytes = ctx->bunzip2_slice_bytes ? ctx->bunzip2_slice_bytes : bunzip2_stream_plan::DEFAULT_SLICE;
        st = new sylph_bunzip2_stream(ctx, bz, n_bytes, n_files, std::max<uint64_t>(slice_bytes, bunzip2_stream_plan::MIN_SLICE));
    });
    if (rc != SYLPH_OK) { delete st; return rc; }
    ctx->refs.fetch_add(1);
    *out = st;
    return SYLPH_OK;
}

int sylph_bunzip2_stream_next(sylph_bunzip2_stream* st, const uint8_t* advance, const uint64_t* keep_from, sylph_inflated** window, uint8_t* finished) {
    return stream_next_entry("sylph_bunzip2_stream", st, advance, keep_from, window, finished, stream_next_impl);
}

int sylph_bunzip2_stream_info(const sylph_bunzip2_stream* st, uint64_t* n_slices, uint64_t* text_bytes, uint64_t* peak_scratch_bytes, uint64_t* peak_window_bytes) {
    return stream_info(st, n_slices, text_bytes, peak_scratch_bytes, peak_window_bytes);
}

void sylph_bunzip2_stream_destroy(sylph_bunzip2_stream* st) {
    stream_destroy(st, [](sylph_bunzip2_stream*) {});
}

}  // extern "C"
