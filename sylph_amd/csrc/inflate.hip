// inflate.hip — gzip (.fastq.gz / .fasta.gz, single-member, multi-member and BGZF) inflated ON THE DEVICE.
//
// The reference reads its normal input — gzip files (README.md:51; sketch.rs:780-781, :906 through needletail -> flate2) — with one
// thread per file: ~0.4 Gbp/s.  Rounds 4-5 inflated on the host with all parse threads (host/pgunzip.cpp): 1.6-2.0 Gbp/s per
// command on the GPU box, the slowest road of the feed although compressed bytes (0.4 B per base) are the cheapest thing to move
// over PCIe.  Here the COMPRESSED bytes travel and the device does the rest (bookkeeping and the proof of it: inflate_plan.h; the host
// scaffold shared with bunzip2.hip: decode_host.h):
//
//   scan1_kernel      every bit position of the file: "BTYPE = dynamic, HLIT/HDIST in range, the code-length code is complete"
//                     (one 17-bit test + a Kraft sum over the 3-bit lengths from a 512-entry LDS table) -> ~0.1 % survive
//   scan2_kernel      one lane per survivor: the header's 258-316 code lengths decoded through a per-lane 7-bit table; both codes
//                     complete (or zlib's single-code exception), an end-of-block code -> the CANDIDATES (true block starts + ~0)
//   decode_kernel     one WAVEFRONT per candidate: the block's Huffman tables built in LDS by the 64 lanes (canonical arithmetic,
//                     10-bit / 8-bit roots, codes beyond the root decoded by first-code comparison — no second-level tables:
//                     3.4 KB of LDS per wave), symbols decoded wave-uniformly (bit buffer and state live in SGPRs; the compressed
//                     words in two VGPRs read with v_readlane; one VGPR as a 64-entry table of 1-3 literal runs), output through
//                     an LDS ring of the last 4 Ki cells: matches are copied by all lanes, from the ring where they reach.  Output:
//                     16-bit cells — a byte, or 256 + w = "byte w of the 32 KiB in front of this block", which nobody knows yet.
//                     The wave runs on through stored / fixed blocks and stops in front of the next dynamic header or behind
//                     a final block, and reports where.
//   (host)            chain_walk: which candidates are the stream, where their bytes go, the members' trailers
//   winfn_kernel      per group of ~sqrt(K) chain blocks, sequentially inside the group: block k's window as a FUNCTION of the
//                     group's first window (32 Ki cells: a byte or a reference into that window), both in LDS (128 KB of the 160)
//   winchain_kernel   the groups' first windows, one after the other (one workgroup, 32 KiB look-ups per group)
//   translate_kernel  all blocks side by side: the block's real window composed in LDS, cells -> bytes in their place in the text
//   crc_kernel        CRC-32 of the text: 64 bytes per lane through slicing-by-4 tables in LDS, the lanes' registers shifted to their
//                     place by polynomial arithmetic (crc32 is linear over GF(2)) and XORed into the member's word; the host
//                     compares with the trailers
//
// Any doubt — a chain that breaks, an output that does not fit its region, a CRC or ISIZE that differs, no room on the device —
// returns SYLPH_ERR_FORMAT / SYLPH_ERR_NOMEM and nothing else happens: the caller inflates with zlib as before.
//
// Two roads run these phases (InflatePhases).  sylph_inflate_files: the files whole, one chain, the text of all of them in one buffer.
// sylph_inflate_stream_*: ONE SLICE of every advancing file's compressed bytes per call, one chain per slice entered with the window its
// file's earlier slices left, the text handed out window by window, in memory bounded by the slice; what a file carries from one call
// to the next, the cut and the sliced chain walk are inflate_stream_plan.h.
#include <zlib.h>

#include <algorithm>

#include "decode_host.h"
#include "inflate_plan.h"
#include "inflate_stream_plan.h"

// What a stream holds between two calls beside decode_host.h's StreamBase: every file's carry and its last 32 KiB of text (two buffers
// per file, taking turns).
struct sylph_inflate_stream : sylph::decode_host::StreamBase {
    using StreamBase::StreamBase;
    uint64_t ratio = 0;                           // cells per compressed byte of a candidate's region
    std::vector<sylph::inflate_stream_plan::Carry> carry = std::vector<sylph::inflate_stream_plan::Carry>(files.size());
    uint8_t* win = nullptr;                       // [n_files][2][WINDOW]
    std::vector<uint8_t> win_cur = std::vector<uint8_t>(files.size(), 0);   // which of a file's two buffers is current
};

namespace sylph {
namespace {

using namespace inflate_plan;
using namespace decode_host;

constexpr int LIT_ROOT = 10, DIST_ROOT = 8, PRE_ROOT = 7;
constexpr uint32_t T_LONG = 0xFFFFu;
constexpr uint32_t REGION_RATIO = 16;       // cells a candidate may write per compressed byte up to the next candidate ...
constexpr uint32_t REGION_SLACK = 1024;     // ... plus this
constexpr uint64_t GZ_PAD_WORDS = 1024;     // zero words behind the compressed bytes (a header parsed at the very end reads < 600 bytes on)

// =================================================================================================================================
// scan, stage 1: the cheap test at every bit position
// =================================================================================================================================
constexpr int SCAN_TPB = 256;
constexpr uint32_t SCAN_STAGE = 4096;       // staged hits per workgroup before a flush (>= SCAN_TPB * 8 + what a flush leaves)

__global__ __launch_bounds__(SCAN_TPB) void scan1_kernel(const uint32_t* __restrict__ gzw, uint64_t byte_lo, uint64_t byte_hi, uint64_t* __restrict__ out,
                                                         unsigned long long* __restrict__ n_out, uint64_t cap) {
    __shared__ uint8_t kraft[512];
    __shared__ uint64_t stage[SCAN_STAGE];
    __shared__ uint32_t stage_n;
    __shared__ unsigned long long gbase;
    for (uint32_t i = threadIdx.x; i < 512; i += SCAN_TPB) {
        uint32_t s = 0;
        for (int f = 0; f < 3; f++) { const uint32_t v = (i >> (3 * f)) & 7; if (v) s += 128u >> v; }
        kraft[i] = (uint8_t)s;                                                // <= 192
    }
    if (threadIdx.x == 0) stage_n = 0;
    __syncthreads();
    const uint64_t span = byte_hi - byte_lo;
    for (uint64_t base = (uint64_t)blockIdx.x * SCAN_TPB; base < span; base += (uint64_t)gridDim.x * SCAN_TPB) {
        const uint64_t b = byte_lo + base + threadIdx.x;
        if (b < byte_hi) {
            const uint64_t wi = b >> 2;
            const uint32_t d0 = gzw[wi], d1 = gzw[wi + 1], d2 = gzw[wi + 2], d3 = gzw[wi + 3];
            const uint32_t s0 = (uint32_t)(b & 3) * 8;
#pragma unroll
            for (uint32_t sh = 0; sh < 8; sh++) {
                const uint32_t s = s0 + sh;                                   // 0 .. 31
                const uint32_t h0 = __builtin_amdgcn_alignbit(d1, d0, s);
                // BTYPE == 2 (bits 1-2 = 0,1), HLIT <= 29, HDIST <= 29
                if (((h0 >> 1) & 3) != 2 || ((h0 >> 3) & 31) > 29 || ((h0 >> 8) & 31) > 29) continue;
                const uint32_t h1 = __builtin_amdgcn_alignbit(d2, d1, s), h2 = __builtin_amdgcn_alignbit(d3, d2, s);
                const uint32_t hclen = ((h0 >> 13) & 15) + 4;
                uint64_t c = ((((uint64_t)h1 << 32) | h0) >> 17) | ((uint64_t)h2 << 47);
                c &= (1ull << (3 * hclen)) - 1;
                uint32_t sum = 0;
#pragma unroll
                for (int j = 0; j < 7; j++) sum += kraft[(uint32_t)(c >> (9 * j)) & 511];
                if (sum != 128) continue;
                const uint32_t at = atomicAdd(&stage_n, 1u);
                stage[at] = b * 8 + sh;
            }
        }
        __syncthreads();
        const uint32_t m = stage_n;                                           // (uniform: everybody reads the same word between two barriers)
        __syncthreads();
        if (m > SCAN_STAGE - SCAN_TPB * 8) {
            if (threadIdx.x == 0) { gbase = atomicAdd(n_out, (unsigned long long)m); stage_n = 0; }
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < m; i += SCAN_TPB)
                if (gbase + i < cap) out[gbase + i] = stage[i];
            __syncthreads();
        }
    }
    __syncthreads();
    const uint32_t m = stage_n;
    if (threadIdx.x == 0 && m) gbase = atomicAdd(n_out, (unsigned long long)m);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < m; i += SCAN_TPB)
        if (gbase + i < cap) out[gbase + i] = stage[i];
}

// =================================================================================================================================
// scan, stage 2: one lane per survivor, the whole header
// =================================================================================================================================
struct LaneBits {                                  // per-lane bit reader over the dword stream
    const uint32_t* w;
    uint64_t acc, wpos;
    uint32_t cnt;
    __device__ __forceinline__ void init(const uint32_t* words, uint64_t bitpos) {
        w = words;
        wpos = bitpos >> 5;
        const uint32_t s = (uint32_t)bitpos & 31;
        acc = (uint64_t)(w[wpos++] >> s);
        cnt = 32 - s;
        refill();
    }
    __device__ __forceinline__ void refill() { if (cnt <= 32) { acc |= (uint64_t)w[wpos++] << cnt; cnt += 32; } }
    __device__ __forceinline__ uint32_t take(uint32_t k) { const uint32_t v = (uint32_t)acc & ((1u << k) - 1); acc >>= k; cnt -= k; return v; }
    __device__ __forceinline__ uint64_t bitpos() const { return wpos * 32 - cnt; }
};

__device__ __constant__ uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

constexpr int SCAN2_TPB = 128;
__global__ __launch_bounds__(SCAN2_TPB) void scan2_kernel(const uint32_t* __restrict__ gzw, uint64_t n_bits, const uint64_t* __restrict__ in,
                                                          const unsigned long long* __restrict__ n_in_p, uint64_t in_cap, uint64_t* __restrict__ out,
                                                          unsigned long long* __restrict__ n_out, uint64_t cap) {
    __shared__ uint8_t pre[SCAN2_TPB][128 + 4];    // (+4: the lanes' tables start in different banks)
    const uint64_t n_in = (uint64_t)min((unsigned long long)*n_in_p, (unsigned long long)in_cap);
    const uint64_t i = (uint64_t)blockIdx.x * SCAN2_TPB + threadIdx.x;
    if (i >= n_in) return;
    const uint64_t p = in[i];
    LaneBits b;
    b.init(gzw, p);
    b.take(3);
    const uint32_t hlit = b.take(5) + 257, hdist = b.take(5) + 1, hclen = b.take(4) + 4;
    uint64_t clp = 0;                               // the 19 code lengths of the code-length code, 3 bits each, by symbol
    for (uint32_t j = 0; j < hclen; j++) { b.refill(); clp |= (uint64_t)b.take(3) << (3 * CL_ORDER[j]); }
    // canonical codes of the code-length code (complete: stage 1 checked the Kraft sum) into the lane's 128-entry table
    uint8_t* tab = pre[threadIdx.x];
    {
        uint32_t code = 0;
        for (uint32_t l = 1; l <= 7; l++) {
            for (uint32_t s = 0; s < 19; s++) {
                if (((clp >> (3 * s)) & 7) != l) continue;
                const uint32_t rev = __brev(code) >> (32 - l);
                for (uint32_t k = rev; k < 128; k += 1u << l) tab[k] = (uint8_t)(s << 3 | l);
                code++;
            }
            code <<= 1;
        }
    }
    const uint32_t total = hlit + hdist;
    uint32_t idx = 0, prev = 0, kl = 0, kd = 0, nzl = 0, nzd = 0, l1 = 0, d1 = 0, eob = 0;
    bool ok = true;
    while (idx < total) {
        b.refill();
        const uint32_t e = tab[(uint32_t)b.acc & 127];
        b.take(e & 7);
        const uint32_t sym = e >> 3;
        uint32_t val, rep;
        if (sym < 16) { val = sym; rep = 1; }
        else if (sym == 16) { if (idx == 0) { ok = false; break; } val = prev; rep = 3 + b.take(2); }
        else if (sym == 17) { val = 0; rep = 3 + b.take(3); }
        else { val = 0; rep = 11 + b.take(7); }
        if (idx + rep > total) { ok = false; break; }
        if (val) {
            const uint32_t nl = idx >= hlit ? 0 : min(rep, hlit - idx), nd = rep - nl;
            kl += nl << (15 - val); nzl += nl; if (val == 1) l1 += nl;
            kd += nd << (15 - val); nzd += nd; if (val == 1) d1 += nd;
            if (idx <= 256 && 256 < idx + rep) eob = val;
        }
        prev = val;
        idx += rep;
    }
    if (!ok || b.bitpos() > n_bits || eob == 0) return;
    if (kl > 32768 || (kl < 32768 && !(nzl == 1 && l1 == 1))) return;          // zlib inflate_table: incomplete only for a single 1-bit code
    if (nzd && (kd > 32768 || (kd < 32768 && !(nzd == 1 && d1 == 1)))) return;
    const unsigned long long at = atomicAdd(n_out, 1ull);
    if (at < cap) out[at] = p;
}

// =================================================================================================================================
// decode: one wavefront per candidate
// =================================================================================================================================
constexpr uint32_t FLUSH = 1024;     // cells of a block leaving the LDS ring for global memory at a time (DecodeOut)
// RING: cells of a block kept in LDS — 4096, or 2048 when the file has more blocks than wavefronts fit beside each other with the larger ring
template <uint32_t RING>
struct WaveTables {
    uint16_t lit[1 << LIT_ROOT];          // sym << 4 | len;  0 = no code;  T_LONG = longer than the root
    uint16_t dist[1 << DIST_ROOT];        // (the code-length code is built here first, 7-bit root)
    uint16_t lit_sorted[288];
    uint16_t dist_sorted[32];
    uint16_t lit_first[16], lit_count[16], lit_off[16];
    uint16_t dist_first[16], dist_count[16], dist_off[16];
    uint8_t lens[320 + 64];
    uint8_t plens[20 + 64];
    uint32_t lit_maxlen, dist_maxlen;
    alignas(16) uint16_t ring[RING + 64];   // (+64: where the lanes that have nothing to write write — see DUMMY below)
    uint32_t stream[256];
};

// Everything the decoding wavefront keeps — bit buffer, positions, counts, the symbol just decoded — is the same in all 64 lanes, and it
// has to live in SGPRs for the loop to run on the scalar unit: a value that came out of LDS or global memory is "divergent" to the
// compiler until it has been through v_readfirstlane, and one divergent value in a loop condition drags the whole state into VGPRs
// behind exec masks (the first build of this file: 7,900 lines of s_and_saveexec).
struct WaveBits {                                  // the same reader, but everything in it is wave-uniform (SGPRs)
    const uint32_t* w;
    uint64_t acc, wpos, wlimit, cbase;
    uint32_t cnt;
    bool over;
    // The stream's words [cbase - 64, cbase + 128) lie in an LDS buffer of 256 words (word i at [i & 255]); the 64 words behind them wait
    // in a VGPR, loaded one chunk — 256 compressed bytes, one coalesced load — ahead of their use.  Both readers take their words there:
    // this one a word per refill (a scalar load per refill put a trip to memory, ~1-2 thousand cycles with nothing else to do, into the
    // chain of every ten literals), the window step three words per lane.
    uint32_t nxt;
    uint32_t* stream;
    uint64_t at;                                   // !synced: the position (acc / cnt / wpos are stale: the window step moves `at` alone)
    bool synced;
    __device__ __forceinline__ uint64_t position() const { return synced ? wpos * 32 - cnt : at; }
    __device__ __forceinline__ void move_to(uint64_t bitpos) {            // (the window step: no word is fetched for the scalar reader)
        at = bitpos;
        synced = false;
        if ((long long)((bitpos >> 5) - cbase) >= 64) next_chunk();
    }
    __device__ __forceinline__ void sync() { if (!synced) seek(at); }
    __device__ __forceinline__ void init(const uint32_t* words, uint64_t bitpos, uint64_t limit_words) {
        const uint32_t lane = threadIdx.x & 63;
        w = words;
        wlimit = limit_words;
        over = false;
        wpos = bitpos >> 5;
        cbase = wpos & ~(uint64_t)63;
        stream[(cbase + lane) & 255] = w[cbase + lane];
        stream[(cbase + 64 + lane) & 255] = w[cbase + 64 + lane];
        nxt = w[cbase + 128 + lane];
        const uint32_t s = (uint32_t)bitpos & 31;
        acc = (uint64_t)(word() >> s);
        cnt = 32 - s;
        synced = true;
        at = 0;
        refill();
    }
    __device__ __forceinline__ void next_chunk() {
        const uint32_t lane = threadIdx.x & 63;
        stream[(cbase + 128 + lane) & 255] = nxt;
        cbase += 64;
        nxt = w[cbase + 128 + lane];
    }
    __device__ __forceinline__ uint32_t word() {                          // the stream's word wpos; wpos moves on
        const uint32_t v = uni(stream[wpos & 255]);
        wpos++;
        if ((long long)(wpos - cbase) >= 64) next_chunk();
        return v;
    }
    // continue at another bit position: at most two words behind the words already taken, less than a chunk ahead of them
    __device__ __forceinline__ void seek(uint64_t bitpos) {
        wpos = bitpos >> 5;
        if ((long long)(wpos - cbase) >= 64) next_chunk();
        const uint32_t s = (uint32_t)bitpos & 31;
        acc = (uint64_t)(word() >> s);
        cnt = 32 - s;
        synced = true;
        refill();
    }
    __device__ __forceinline__ void refill() {
        if (cnt <= 32) {
            if (wpos >= wlimit) { over = true; wpos++; }
            else acc |= (uint64_t)word() << cnt;
            cnt += 32;
        }
    }
    __device__ __forceinline__ uint32_t peek(uint32_t k) const { return (uint32_t)acc & ((1u << k) - 1); }
    __device__ __forceinline__ void drop(uint32_t k) { acc >>= k; cnt -= k; }
    __device__ __forceinline__ uint32_t take(uint32_t k) { const uint32_t v = peek(k); drop(k); return v; }
    __device__ __forceinline__ uint64_t bitpos() const { return wpos * 32 - cnt; }
};

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint64_t lanemask_lt() { return (1ull << (threadIdx.x & 63)) - 1; }

// Canonical code from lens[0, nsym): sorted symbols, first code / count / offset per length, the root table.  kind: 0 = the
// code-length code (must be complete), 1 = literal/length, 2 = distance (zlib inflate_table: an incomplete code is fine only when
// it is a single 1-bit code; a distance code with no code at all is fine).  Wave-uniform result.
__device__ bool build_code_raw(const uint8_t* lens, uint32_t nsym, uint32_t root, uint16_t* tab, uint16_t* sorted, uint16_t* first, uint16_t* count,
                           uint16_t* off, uint32_t* maxlen_out, int kind) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t used = 0;
    // (every loop of this kernel counts in wave-uniform steps and tests the lane inside: a loop whose induction variable depends on the
    //  lane has, for the compiler, an exit that lanes may take at different times — and everything behind it stops being uniform)
    for (uint32_t base = 0; base < nsym; base += 64)
        if (base + lane < nsym) used |= 1u << lens[base + lane];
    used = uni(wave_or(used)) & ~1u;
    uint32_t run = 0, code = 0, prev_count = 0, maxlen = 0;
    int left = 1;
    bool over = false;
    for (uint32_t L = 1; L <= 15; L++) {
        const uint32_t off_l = run;
        if (used >> L & 1) {
            for (uint32_t base = 0; base < nsym; base += 64) {
                const uint32_t s = base + lane;
                const bool hit = s < nsym && lens[s] == L;
                const uint64_t mask = __ballot(hit);
                if (hit) sorted[run + __popcll(mask & lanemask_lt())] = (uint16_t)s;
                run += __popcll(mask);
            }
            maxlen = L;
        }
        const uint32_t c = run - off_l;
        code = (code + prev_count) << 1;
        prev_count = c;
        left = (left << 1) - (int)c;
        if (left < 0) over = true;
        if (lane == 0) { first[L] = (uint16_t)code; count[L] = (uint16_t)c; off[L] = (uint16_t)off_l; }
    }
    *maxlen_out = maxlen;
    __syncthreads();
    if (over) return false;
    if (run == 0) { if (kind != 2) return false; }
    else if (left > 0 && (kind == 0 || maxlen != 1)) return false;
    const uint32_t top = min(root, maxlen);
    for (uint32_t base = 0; base < (1u << root); base += 64) {
        const uint32_t idx = base + lane;
        const uint32_t r = __brev(idx) >> (32 - root);
        uint32_t e = maxlen > root ? T_LONG : 0;
        for (uint32_t L = 1; L <= top; L++) {
            const uint32_t d = (r >> (root - L)) - first[L];
            if (d < count[L]) { e = (uint32_t)sorted[off[L] + d] << 4 | L; break; }
        }
        tab[idx] = (uint16_t)e;
    }
    __syncthreads();
    return true;
}

// (the value a call returns is divergent to the compiler, whatever the callee computes: one v_readfirstlane says what it is)
__device__ __forceinline__ bool build_code(const uint8_t* lens, uint32_t nsym, uint32_t root, uint16_t* tab, uint16_t* sorted, uint16_t* first, uint16_t* count,
                                           uint16_t* off, uint32_t* maxlen_out, int kind) {
    return uni(build_code_raw(lens, nsym, root, tab, sorted, first, count, off, maxlen_out, kind) ? 1u : 0u) != 0;
}

// a code longer than the root: first-code comparison, lengths root+1 .. maxlen.  -> sym << 4 | len, or 0
__device__ __forceinline__ uint32_t decode_long(uint32_t bits, uint32_t root, uint32_t maxlen, const uint16_t* sorted, const uint16_t* first,
                                                const uint16_t* count, const uint16_t* off) {
    const uint32_t r = __brev(bits);
    for (uint32_t L = root + 1; L <= maxlen; L++) {
        const uint32_t d = (r >> (32 - L)) - uni(first[L]);
        if (d < uni(count[L])) return uni(sorted[uni(off[L]) + d]) << 4 | L;
    }
    return 0;
}

// DUMMY: a store that only some lanes make is written as a store every lane makes, the idle ones into a pad behind the array — an
// `if (lane < c)` is a divergent branch, and LLVM's uniformity analysis marks every phi of the block where its two sides meet as
// divergent; when that block is also where a loop's `continue` / `break` paths meet, the loop's exit stops being uniform and all of its
// state moves into VGPRs behind exec masks (found with opt -passes='print<uniformity>').
// Where a block's cells go: the last RING of them live in an LDS ring, and whole chunks of FLUSH cells leave for the candidate's
// region in global memory behind the wave (two 16-byte stores per lane).  A copy whose source lies inside the ring — distance +
// length <= RING — is LDS reads and writes, ~100 cycles; only a copy from further back loads from global memory (its source left
// the ring at least a chunk ago, so the stores are issued; the same wave's loads see them).  The first version kept nothing on the
// chip and every match waited for the acknowledgement of all earlier stores and for its own load — vmcnt counts both —, ~5,000
// cycles per match: 35 ms for a block of 16 K matches, whatever the literals cost.
// (DecodeJob — one candidate for a wavefront — and where its region lies: inflate_plan.h)
// the spill arena behind the candidates' regions: SPILL_SLOTS regions of SPILL_CELLS cells, handed out by an atomic counter (next)
struct Spill { unsigned long long base; uint32_t slots; };
constexpr uint32_t SPILL_CELLS = 1u << 20, SPILL_SLOTS = 96;

template <uint32_t RING>
struct DecodeOut {                       // n, flushed, cap: wave-uniform
    static constexpr uint32_t RING_MASK = RING - 1;
    uint16_t* out;
    uint16_t* ring;
    uint32_t n, flushed, cap;
    bool dry;                            // the region is full: the rest of the block is decoded for its length and its end only (room())
    __device__ __forceinline__ void flush_chunk() {
        if (!dry) {
            const uint32_t lane = threadIdx.x & 63;
            const uint4* src = reinterpret_cast<const uint4*>(ring + ((flushed + lane * 16) & RING_MASK));
            uint4* dst = reinterpret_cast<uint4*>(out + region + flushed + lane * 16);
            const uint4 a = src[0], b = src[1];
            dst[0] = a;
            dst[1] = b;
        }
        flushed += FLUSH;
    }
    // k more cells: false = not even countable (a block of 4 Gi cells).  A block that outgrows its region — a header-like bit pattern
    // inside it cut the region short (one in ~4,000 blocks of a FASTQ file), or it deflates better than REGION_RATIO — MOVES, once, to a
    // region of SPILL_CELLS cells of the spill arena (what it has written so far goes with it: whole chunks, 16 bytes per lane and
    // step); a block that outgrows that too, or finds the arena empty, goes on DRY: it still reports where it ends and how long it is,
    // and the host has it decoded once more into a region of exactly that size.
    uint32_t* spill_next;
    unsigned long long spill_base;
    uint32_t spill_slots;
    bool moved;
    unsigned long long region;
    __device__ __forceinline__ bool room(uint32_t k) {
        if (n + k > cap && !dry) {
            uint32_t slot = ~0u;
            if (!moved && n + k <= SPILL_CELLS) {
                if ((threadIdx.x & 63) == 0) slot = atomicAdd(spill_next, 1u);
                slot = uni(slot);
            }
            if (slot < spill_slots) {
                const unsigned long long to = spill_base + (unsigned long long)slot * SPILL_CELLS;
                for (uint32_t at = 0; at < flushed; at += 64 * 8) {
                    const uint32_t i = at + (threadIdx.x & 63) * 8;
                    if (i < flushed) *reinterpret_cast<uint4*>(out + to + i) = *reinterpret_cast<const uint4*>(out + region + i);
                }
                region = to;
                cap = SPILL_CELLS;
                moved = true;
            } else dry = true;
        }
        return n + k <= 0xFFFFFF00u;
    }
    __device__ __forceinline__ void advance(uint32_t k) {
        n += k;
        while (n - flushed >= FLUSH) flush_chunk();
    }
    __device__ __forceinline__ void finish() {
        for (uint32_t base = flushed; base < n && !dry; base += 64) {
            const uint32_t i = base + (threadIdx.x & 63);
            if (i < n) out[region + i] = ring[i & RING_MASK];
        }
        flushed = n;
    }
};

template <uint32_t RING>
__global__ __launch_bounds__(64) void decode_kernel(const uint32_t* __restrict__ gzw, uint64_t n_words_all, const DecodeJob* __restrict__ jobs, uint16_t* __restrict__ cells,
                                                    Spill spill, uint32_t* __restrict__ spill_next, BlockResult* __restrict__ res) {
    constexpr uint32_t RING_MASK = RING - 1;
    __shared__ WaveTables<RING> T;
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    const DecodeJob job = jobs[k];
    // the words this block may read: all of the launch's, or (a slice of the stream, which ends where another file's slice begins) fewer
    const uint64_t n_words = job.limit_words ? min((uint64_t)job.limit_words, n_words_all) : n_words_all;
    const uint64_t start = job.start_bit;
    const uint64_t region = job.region;
    DecodeOut<RING> o;
    o.out = cells;                                  // (the whole buffer: a block's cells begin at o.region — which the block may change, room())
    o.ring = T.ring;
    o.n = 0; o.flushed = 0;
    o.cap = job.cap;
    o.dry = false;
    o.spill_base = spill.base;
    o.spill_slots = spill.slots;
    o.spill_next = spill_next;
    o.moved = false;
    o.region = region;
    const bool have_window = job.have_window != 0;
    WaveBits b;
    b.stream = T.stream;
    b.init(gzw, start, n_words);
    uint32_t status = ST_NONE, flags = 0;
    uint64_t end_bit = 0;
    bool first_block = true;
    uint32_t n_sym = 0, n_far = 0;
    uint64_t t_build = 0;

    const uint64_t t_start = __builtin_readcyclecounter();
    for (;;) {
        if (status != ST_NONE) break;
        b.refill();
        const uint64_t header_at = b.bitpos();
        const uint32_t bfinal = b.peek(1), btype = (b.peek(3) >> 1);
        if (!first_block && btype == 2) { status = ST_NEXT_DYNAMIC; end_bit = header_at; break; }
        first_block = false;
        b.drop(3);
        if (btype == 3) { status = ST_ERR_CODE; break; }
        if (btype == 0) {
            b.drop(b.cnt & 7);                                                 // to the byte boundary
            b.refill();
            const uint32_t len = b.take(16);
            b.refill();
            const uint32_t nlen = b.take(16);
            if (b.over || (len ^ 0xFFFFu) != nlen) { status = ST_ERR_STORED; break; }
            const uint64_t from = b.bitpos() >> 3;
            if (from + len > n_words * 4) { status = ST_ERR_OVERRUN; break; }
            if (!o.room(len)) { status = ST_OVERFLOW; break; }
            const uint8_t* gzb = reinterpret_cast<const uint8_t*>(gzw);
            for (uint32_t base = 0; base < len; base += 64) {
                o.ring[base + lane < len ? (o.n + lane) & RING_MASK : RING + lane] = gzb[from + min(base + lane, len - 1)];
                o.advance(min(64u, len - base));
            }
            b.init(gzw, (from + len) * 8, n_words);
        } else {
            const uint64_t t_b0 = __builtin_readcyclecounter();
            if (btype == 2) {
                b.refill();
                const uint32_t hlit = b.take(5) + 257, hdist = b.take(5) + 1, hclen = b.take(4) + 4;
                if (hlit > 286 || hdist > 30) { status = ST_ERR_CODE; break; }
                T.plens[lane < 19 ? lane : 20 + lane] = 0;   // (no branch on the lane: DUMMY)
                __syncthreads();
                for (uint32_t i = 0; i < hclen; i++) {
                    b.refill();
                    const uint32_t v = b.take(3);
                    T.plens[lane == 0 ? (uint32_t)CL_ORDER[i] : 20 + lane] = (uint8_t)v;
                }
                __syncthreads();
                uint32_t pre_max;
                if (b.over || !build_code(T.plens, 19, PRE_ROOT, T.dist, T.dist_sorted, T.dist_first, T.dist_count, T.dist_off, &pre_max, 0)) {
                    status = b.over ? ST_ERR_OVERRUN : ST_ERR_CODE;
                    break;
                }
                const uint32_t total = hlit + hdist;
                uint32_t i = 0, prev = 0;
                bool bad = false;
                while (i < total) {
                    b.refill();
                    const uint32_t e = uni(T.dist[b.peek(PRE_ROOT)]);
                    if (e == 0) { bad = true; break; }
                    b.drop(e & 15);
                    const uint32_t sym = e >> 4;
                    uint32_t val, rep;
                    if (sym < 16) { val = sym; rep = 1; }
                    else if (sym == 16) { if (i == 0) { bad = true; break; } val = prev; rep = 3 + b.take(2); }
                    else if (sym == 17) { val = 0; rep = 3 + b.take(3); }
                    else { val = 0; rep = 11 + b.take(7); }
                    if (i + rep > total) { bad = true; break; }
                    for (uint32_t jb = 0; jb < rep; jb += 64) T.lens[jb + lane < rep ? i + jb + lane : 320 + lane] = (uint8_t)val;
                    prev = val;
                    i += rep;
                }
                __syncthreads();
                if (bad || b.over || uni(T.lens[256]) == 0) { status = b.over ? ST_ERR_OVERRUN : ST_ERR_CODE; break; }
                if (!build_code(T.lens, hlit, LIT_ROOT, T.lit, T.lit_sorted, T.lit_first, T.lit_count, T.lit_off, &T.lit_maxlen, 1) ||
                    !build_code(T.lens + hlit, hdist, DIST_ROOT, T.dist, T.dist_sorted, T.dist_first, T.dist_count, T.dist_off, &T.dist_maxlen, 2)) {
                    status = ST_ERR_CODE;
                    break;
                }
            } else {
                for (uint32_t sb = 0; sb < 288; sb += 64) {
                    const uint32_t s = sb + lane;
                    if (s < 288) T.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
                }
                if (lane < 32) T.lens[288 + lane] = 5;
                __syncthreads();
                build_code(T.lens, 288, LIT_ROOT, T.lit, T.lit_sorted, T.lit_first, T.lit_count, T.lit_off, &T.lit_maxlen, 1);
                build_code(T.lens + 288, 32, DIST_ROOT, T.dist, T.dist_sorted, T.dist_first, T.dist_count, T.dist_off, &T.dist_maxlen, 2);
            }
            const uint32_t lit_max = uni(T.lit_maxlen), dist_max = uni(T.dist_maxlen);
            t_build += __builtin_readcyclecounter() - t_b0;
            // ---- the block's symbols
            // THE WINDOW STEP.  A wavefront that decodes one symbol at a time spends 300 cycles on a literal and 1,500 on a match, whatever
            // the instruction count: every turn is a chain of dependent scalar instructions, taken branches and trips to the LDS, each
            // waited for with nothing else to do (profiles/r06_inflate_steps.txt).  So the 64 lanes decode the 64 BIT POSITIONS behind the
            // stream's position at once — lane j: "if a symbol started j bits from here, which one, how long, how many bits" (its own three
            // words of the stream, one look-up in each table) — and the wave then walks the chain of true starts with v_readlane (bits used
            // by the symbol at 0 lead to the next start, ...), four scalar instructions per symbol.  The cells the walked symbols produce
            // (at most 64 per step) are dealt to the lanes, literals written, copies resolved in rounds — a round gives every cell whose
            // source lies in front of the first unresolved one its value: one round unless a copy reads what this step wrote.  What the
            // step cannot take — a code longer than the table's root, a copy of more than 64 cells, the last bits of the stream — is left
            // to the one-symbol path behind it, which also reports the errors.
            bool eob = false;
            const uint64_t limit_bits = n_words * 32;
            while (!eob && status == ST_NONE) {
                n_sym++;
                uint32_t taken = 0;
                const uint64_t p = b.position();
                if (p + 256 <= limit_bits) {
                    // lane j: the symbols that would start at bit p + j and at bit p + 64 + j (a window of 128 bit positions per step: the
                    // LDS round trips of a step are what it costs, and both positions' look-ups travel together)
                    const uint64_t pj = p + lane;
                    const uint32_t wj = (uint32_t)(pj >> 5), sj = (uint32_t)pj & 31;
                    const uint32_t d0 = T.stream[wj & 255], d1 = T.stream[(wj + 1) & 255], d2 = T.stream[(wj + 2) & 255], d3 = T.stream[(wj + 3) & 255],
                                   d4 = T.stream[(wj + 4) & 255];
                    const uint32_t xa0 = __builtin_amdgcn_alignbit(d1, d0, sj), xa1 = __builtin_amdgcn_alignbit(d2, d1, sj);
                    const uint32_t xb0 = __builtin_amdgcn_alignbit(d3, d2, sj), xb1 = __builtin_amdgcn_alignbit(d4, d3, sj);
                    const uint32_t ea1 = T.lit[xa0 & ((1u << LIT_ROOT) - 1)], eb1 = T.lit[xb0 & ((1u << LIT_ROOT) - 1)];
                    // -> walk word (bits | cells << 6 | end-of-block << 13 | not-for-this-step << 14) and what a cell needs of its symbol
                    //    (cells << 7 | literal << 14 | (the literal's byte, or the distance) << 15; the first cell's 7 bits come from the walk)
                    auto decode_at = [&](uint32_t x0, uint32_t x1, uint32_t e1, uint32_t& walk, uint32_t& about) {
                        const uint32_t l1 = e1 & 15, sy = e1 >> 4;
                        const bool is_lit = sy < 256, is_eob = sy == 256, is_len = sy > 256;
                        // (a length code's extra bits and distance: computed by every lane, kept by the lanes that saw one — no branch on the lane)
                        const uint32_t ls = is_len ? sy - 257 : 0;
                        const uint32_t leb = ls < 8 || ls >= 28 ? 0u : (ls - 4) >> 2;
                        const uint32_t lbase = ls < 8 ? 3 + ls : ls >= 28 ? 258u : 3 + ((4 + (ls & 3)) << leb);
                        const uint64_t x = ((uint64_t)x1 << 32 | x0) >> l1;
                        const uint32_t len = lbase + ((uint32_t)x & ((1u << leb) - 1));
                        const uint32_t y = (uint32_t)(x >> leb);
                        const uint32_t e2 = T.dist[y & ((1u << DIST_ROOT) - 1)];
                        const uint32_t l2 = e2 & 15, dsy = e2 >> 4;
                        const uint32_t deb = dsy < 4 ? 0u : min((dsy - 2) >> 1, 13u);
                        const uint32_t dbase = dsy < 4 ? 1 + dsy : 1 + ((2 + (dsy & 1)) << deb);
                        const bool bad = e1 == T_LONG || e1 == 0 || sy > 285 || (is_len && (e2 == T_LONG || e2 == 0 || dsy >= 30 || len > 64));
                        const uint32_t bits = is_len ? l1 + leb + l2 + deb : l1;
                        const uint32_t cells = is_len ? len : is_lit ? 1u : 0u;
                        about = cells << 7 | (is_lit ? 1u << 14 : 0u) | (is_lit ? sy : dbase + ((y >> l2) & ((1u << deb) - 1))) << 15;
                        walk = bits | cells << 6 | (is_eob ? 1u << 13 : 0u) | (bad ? 1u << 14 : 0u);
                    };
                    uint32_t walk_a, about_a, walk_b, about_b;
                    decode_at(xa0, xa1, ea1, walk_a, about_a);
                    decode_at(xb0, xb1, eb1, walk_b, about_b);
                    // the chain of symbol starts, from position 0; owner of cell c = the last walked symbol whose first cell is <= c
                    uint32_t pos = 0, total = 0, owner = 0, first_a = 0, first_b = 0;
                    while (pos < 128) {
                        const uint32_t w1 = pos < 64 ? __builtin_amdgcn_readlane(walk_a, pos) : __builtin_amdgcn_readlane(walk_b, pos - 64);
                        const uint32_t c = (w1 >> 6) & 127;
                        if ((w1 >> 14) || total + c > 64) break;
                        owner = lane >= total ? pos : owner;
                        first_a = lane == pos ? total : first_a;
                        first_b = lane + 64 == pos ? total : first_b;
                        total += c;
                        taken++;
                        pos += w1 & 63;
                        if (w1 >> 13 & 1) { eob = true; break; }
                    }
                    if (taken) {
                        if (!o.room(total)) { status = ST_OVERFLOW; break; }
                        const uint32_t from_a = __shfl(about_a | first_a, owner & 63), from_b = __shfl(about_b | first_b, owner & 63);
                        const uint32_t mine_about = owner < 64 ? from_a : from_b;
                        const uint32_t my_first = mine_about & 127, my_len = (mine_about >> 7) & 127, my_val = mine_about >> 15;
                        const bool mine = lane < total, my_lit = (mine_about >> 14 & 1) != 0;
                        const uint32_t i = lane - my_first;                  // my cell's index in its symbol; my_val: its distance
                        const int src = (int)(o.n + my_first) - (int)my_val + (int)(my_val >= my_len ? i : my_val == 1 ? 0u : i % max(my_val, 1u));
                        const bool is_copy = mine && !my_lit;
                        if (__ballot(is_copy && src < 0)) {
                            if (!have_window || __ballot(is_copy && src < -(int)WINDOW)) { status = ST_ERR_DISTANCE; break; }
                            flags |= 1;
                        }
                        const bool far = is_copy && src >= 0 && (int)(o.n + lane) - src > (int)(RING - 128);
                        n_far += __ballot(far) ? 1u : 0u;
                        // literals now; copies in rounds
                        o.ring[mine && my_lit ? (o.n + lane) & RING_MASK : RING + lane] = (uint16_t)my_val;
                        uint64_t pending = __ballot(is_copy);
                        while (pending) {
                            const uint32_t frontier = o.n + (uint32_t)__builtin_ctzll(pending);   // every cell in front of it has its value
                            const bool can = is_copy && (pending >> lane & 1) && src < (int)frontier;
                            const uint32_t at = (uint32_t)max(src, 0);
                            uint16_t v = o.ring[at & RING_MASK];
                            if (__ballot(can && far) && !o.dry) { const uint16_t g = o.out[o.region + (far ? at : 0u)]; v = far ? g : v; }
                            o.ring[can ? (o.n + lane) & RING_MASK : RING + lane] = src < 0 ? (uint16_t)(256 + WINDOW + src) : v;
                            pending &= ~__ballot(can);
                        }
                        o.advance(total);
                        b.move_to(p + pos);
                    }
                }
                if (taken || eob || status != ST_NONE) continue;
                // ---- one symbol, the slow way
                b.sync();
                b.refill();
                uint32_t e = uni(T.lit[b.peek(LIT_ROOT)]);
                if (e == T_LONG) e = uni(decode_long((uint32_t)b.acc, LIT_ROOT, lit_max, T.lit_sorted, T.lit_first, T.lit_count, T.lit_off));
                if (e == 0) { status = ST_ERR_CODE; break; }
                b.drop(e & 15);
                const uint32_t sym = e >> 4;
                if (sym < 256) {
                    if (!o.room(1)) { status = ST_OVERFLOW; break; }
                    o.ring[lane == 0 ? o.n & RING_MASK : RING + lane] = (uint16_t)sym;
                    o.advance(1);
                    continue;
                }
                if (sym == 256) { eob = true; continue; }
                const uint32_t s = sym - 257;
                if (s >= 29) { status = ST_ERR_CODE; break; }
                uint32_t len;
                if (s < 8) len = 3 + s;
                else if (s == 28) len = 258;
                else { const uint32_t eb = (s - 4) >> 2; len = 3 + ((4 + (s & 3)) << eb) + b.take(eb); }
                b.refill();
                uint32_t de = uni(T.dist[b.peek(DIST_ROOT)]);
                if (de == T_LONG) de = uni(decode_long((uint32_t)b.acc, DIST_ROOT, dist_max, T.dist_sorted, T.dist_first, T.dist_count, T.dist_off));
                if (de == 0) { status = ST_ERR_CODE; break; }
                b.drop(de & 15);
                const uint32_t ds = de >> 4;
                if (ds >= 30) { status = ST_ERR_CODE; break; }
                uint32_t dist;
                if (ds < 4) dist = 1 + ds;
                else { const uint32_t eb = (ds - 2) >> 1; dist = 1 + ((2 + (ds & 1)) << eb) + b.take(eb); }
                if (b.over) { status = ST_ERR_OVERRUN; break; }
                if (dist > o.n) {
                    if (!have_window || dist - o.n > WINDOW) { status = ST_ERR_DISTANCE; break; }
                    flags |= 1;
                }
                if (!o.room(len)) { status = ST_OVERFLOW; break; }
                // sources: cell n - dist + (i mod dist) for i < len — all of them in front of n, whatever the overlap
                const int src0 = (int)o.n - (int)dist;
                const bool near = dist + len <= RING;
                n_far += near ? 0u : 1u;
                for (uint32_t base = 0; base < len; base += 64) {
                    const uint32_t i = min(base + lane, len - 1);
                    const int src = src0 + (int)(dist >= len ? i : dist == 1 ? 0u : i % dist);
                    const uint32_t at = (uint32_t)max(src, 0);
                    // (two loads and a select of the VALUES: a select between an LDS and a global POINTER becomes a flat load whose
                    //  aperture test hipcc 7.2 cannot select — "Illegal instruction detected: V_CMP_NE_U32 0, $src_shared_base")
                    const bool from_ring = near || o.dry;
                    const uint16_t in_ring = o.ring[at & RING_MASK];
                    uint16_t got = in_ring;
                    if (!from_ring) got = *const_cast<const volatile uint16_t*>(&o.out[o.region + at]);   // (volatile: not to be merged with the load above)
                    o.ring[base + lane < len ? (o.n + i) & RING_MASK : RING + lane] = src < 0 ? (uint16_t)(256 + WINDOW + src) : got;
                }
                o.advance(len);
            }
            b.sync();
            if (status != ST_NONE) break;
            if (b.over) { status = ST_ERR_OVERRUN; break; }
        }
        if (bfinal) { status = ST_FINAL; end_bit = b.bitpos(); }
    }
    o.finish();
    if (lane == 0) {
        BlockResult r;
        r.end_bit = end_bit;
        r.n_out = o.n;
        r.status = status;
        r.flags = flags | (o.dry ? 2u : 0u);
        r.pad = 0;
        r.region = o.region;
        r.stats[0] = n_sym;
        r.stats[1] = n_far;
        r.stats[2] = (uint32_t)(t_build >> 10);
        r.stats[3] = (uint32_t)((__builtin_readcyclecounter() - t_start) >> 10);
        res[k] = r;
    }
}

// =================================================================================================================================
// windows
// =================================================================================================================================
struct PlanBlock {                      // one chain block, as the device needs it
    const uint16_t* cells;              // its region of cells (in the first pass's buffer, or in the buffer of the blocks decoded again)
    unsigned long long out_off;
    uint32_t n_out;
    uint32_t flags;
};

constexpr int WIN_TPB = 1024;
// group g = chain blocks [g * G, min(K, (g + 1) * G)).  S (in LDS, 2 x 32 Ki cells): the window in front of the current block as a
// function of the window in front of the group's first block.  sfn[k] receives the S of block k, ffn[g] the one behind the group.
__global__ __launch_bounds__(WIN_TPB) void winfn_kernel(const PlanBlock* __restrict__ plan, uint32_t K, uint32_t G, uint16_t* __restrict__ sfn,
                                                        uint16_t* __restrict__ ffn) {
    extern __shared__ uint16_t S[];     // [2][WINDOW]
    const uint32_t g = blockIdx.x, k0 = g * G, k1 = min(K, k0 + G);
    uint16_t* cur = S;
    uint16_t* nxt = S + WINDOW;
    for (uint32_t j = threadIdx.x; j < WINDOW; j += WIN_TPB) cur[j] = (uint16_t)(256 + j);
    __syncthreads();
    for (uint32_t k = k0; k < k1; k++) {
        uint16_t* dst = sfn + (uint64_t)k * WINDOW;
        for (uint32_t j = threadIdx.x; j < WINDOW; j += WIN_TPB) dst[j] = cur[j];
        const uint32_t t = plan[k].n_out;
        const uint16_t* c = plan[k].cells;
        if (t >= WINDOW) {
            const uint16_t* tail = c + (t - WINDOW);
            for (uint32_t j = threadIdx.x; j < WINDOW; j += WIN_TPB) {
                const uint16_t v = tail[j];
                nxt[j] = v < 256 ? v : cur[v - 256];
            }
        } else {
            const uint32_t keep = WINDOW - t;                                   // the older window, moved down
            for (uint32_t j = threadIdx.x; j < WINDOW; j += WIN_TPB) {
                if (j < keep) nxt[j] = cur[j + t];
                else { const uint16_t v = c[j - keep]; nxt[j] = v < 256 ? v : cur[v - 256]; }
            }
        }
        __syncthreads();
        uint16_t* sw = cur; cur = nxt; nxt = sw;
    }
    uint16_t* dst = ffn + (uint64_t)g * WINDOW;
    for (uint32_t j = threadIdx.x; j < WINDOW; j += WIN_TPB) dst[j] = cur[j];
}

// the real window in front of every group, one group after the other
// (entry: the 32 KiB in front of the chain's first block — the text the stream's earlier slices gave this file; null = nothing)
__global__ __launch_bounds__(WIN_TPB) void winchain_kernel(const uint16_t* __restrict__ ffn, uint32_t n_groups, uint8_t* __restrict__ rwin,
                                                           const uint8_t* __restrict__ entry) {
    __shared__ uint8_t R[2][WINDOW];
    uint8_t* cur = R[0];
    uint8_t* nxt = R[1];
    for (uint32_t j = threadIdx.x; j < WINDOW; j += WIN_TPB) cur[j] = entry ? entry[j] : (uint8_t)0;
    __syncthreads();
    for (uint32_t g = 0; g < n_groups; g++) {
        uint8_t* dst = rwin + (uint64_t)g * WINDOW;
        const uint16_t* f = ffn + (uint64_t)g * WINDOW;
        for (uint32_t j = threadIdx.x; j < WINDOW; j += WIN_TPB) {
            dst[j] = cur[j];
            const uint16_t v = f[j];
            nxt[j] = v < 256 ? (uint8_t)v : cur[v - 256];
        }
        __syncthreads();
        uint8_t* sw = cur; cur = nxt; nxt = sw;
    }
}

// the window behind a slice: the last 32 KiB of (the window in front of it ++ the n_new bytes it gave)
__global__ __launch_bounds__(WIN_TPB) void window_tail_kernel(const uint8_t* __restrict__ old_win, const uint8_t* __restrict__ fresh, uint64_t n_new,
                                                              uint8_t* __restrict__ new_win) {
    for (uint32_t j = blockIdx.x * WIN_TPB + threadIdx.x; j < WINDOW; j += gridDim.x * WIN_TPB) {
        const uint64_t back = WINDOW - j;                                        // byte j lies `back` bytes in front of the end
        new_win[j] = back <= n_new ? fresh[n_new - back] : old_win[j + n_new];
    }
}

// =================================================================================================================================
// cells -> bytes
// =================================================================================================================================
constexpr int TR_TPB = 256;
__global__ __launch_bounds__(TR_TPB) void translate_kernel(const PlanBlock* __restrict__ plan, uint32_t G,
                                                           const uint16_t* __restrict__ sfn, const uint8_t* __restrict__ rwin, uint8_t* __restrict__ text) {
    __shared__ uint8_t W[WINDOW];
    const uint32_t k = blockIdx.x;
    const PlanBlock pb = plan[k];
    if (pb.flags & 1) {
        const uint16_t* s = sfn + (uint64_t)k * WINDOW;
        const uint8_t* r = rwin + (uint64_t)(k / G) * WINDOW;
        for (uint32_t j = threadIdx.x; j < WINDOW; j += TR_TPB) { const uint16_t v = s[j]; W[j] = v < 256 ? (uint8_t)v : r[v - 256]; }
        __syncthreads();
    }
    const uint16_t* c = pb.cells;
    uint8_t* o = text + pb.out_off;
    const uint32_t n = pb.n_out;
    // byte-wise up to the first 4-byte boundary of the text, then four cells -> one dword per lane
    const uint32_t head = min(n, (uint32_t)((4 - (pb.out_off & 3)) & 3));
    if (threadIdx.x < head) { const uint16_t v = c[threadIdx.x]; o[threadIdx.x] = v < 256 ? (uint8_t)v : W[v - 256]; }
    const uint32_t quads = (n - head) / 4;
    for (uint32_t q = threadIdx.x; q < quads; q += TR_TPB) {
        const uint16_t* cq = c + head + 4 * q;
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) { const uint16_t v = cq[j]; w |= (uint32_t)(v < 256 ? (uint8_t)v : W[v - 256]) << (8 * j); }
        *reinterpret_cast<uint32_t*>(o + head + 4 * q) = w;
    }
    const uint32_t done = head + 4 * quads;
    if (threadIdx.x < n - done) { const uint16_t v = c[done + threadIdx.x]; o[done + threadIdx.x] = v < 256 ? (uint8_t)v : W[v - 256]; }
}

// =================================================================================================================================
// CRC-32
// =================================================================================================================================
constexpr int CRC_TPB = 256;
constexpr uint32_t CRC_LANE = 64;                       // bytes per lane and step
constexpr uint32_t CRC_STEP = 64 * CRC_LANE;            // bytes per wavefront and step: 4 KiB
constexpr uint32_t CRC_SPAN = 16 * CRC_STEP;            // bytes per wavefront: 64 KiB
// member_end[m]: ascending end offsets of the members in the text.  raw[m] ^= (register of a piece, started at 0) shifted by the
// bytes between the piece's end and the member's end.  A wavefront walks 64 KiB in steps of 4 KiB: every lane takes the register
// of its 64 bytes through the slicing tables and multiplies it by x^(8 * bytes behind it in the step) — a constant per lane —, the
// 64 products are XORed across the wave, and the step joins the wave's running register (one more multiplication by a constant);
// the expensive shift by an arbitrary distance (crc_shift: ~30 multiplications) happens once per span, or where a member ends.
// Steps that hold a member boundary (one in sixteen for BGZF) or the text's ragged end go lane by lane.
__global__ __launch_bounds__(CRC_TPB) void crc_kernel(const uint8_t* __restrict__ text, uint64_t total, const unsigned long long* __restrict__ member_end,
                                                      uint32_t n_members, const uint32_t* __restrict__ x2n_g, uint32_t* __restrict__ raw) {
    __shared__ uint32_t T[4][256];
    __shared__ uint32_t x2n[64];
    __shared__ uint32_t lane_k[64];                     // x^(8 * 64 * (63 - lane))
    for (uint32_t i = threadIdx.x; i < 256; i += CRC_TPB) {
        uint32_t c = i;
        for (int b = 0; b < 8; b++) c = (c & 1) ? (c >> 1) ^ CRC_POLY : c >> 1;
        T[0][i] = c;
    }
    if (threadIdx.x < 64) x2n[threadIdx.x] = x2n_g[threadIdx.x];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 256; i += CRC_TPB) {
        const uint32_t c1 = (T[0][i] >> 8) ^ T[0][T[0][i] & 0xFF];
        const uint32_t c2 = (c1 >> 8) ^ T[0][c1 & 0xFF];
        const uint32_t c3 = (c2 >> 8) ^ T[0][c2 & 0xFF];
        T[1][i] = c1; T[2][i] = c2; T[3][i] = c3;
    }
    if (threadIdx.x < 64) lane_k[threadIdx.x] = crc_x8n(x2n, (uint64_t)CRC_LANE * (63 - threadIdx.x));
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (CRC_TPB / 64) + (threadIdx.x >> 6);
    const uint64_t span0 = wave * CRC_SPAN;
    if (span0 >= total) return;
    const uint64_t span1 = min(total, span0 + CRC_SPAN);
    const uint32_t k_step = crc_x8n(x2n, CRC_STEP), k_mine = lane_k[lane];
    // the member that holds span0: the first whose end lies behind it
    uint32_t lo = 0, hi = n_members - 1;
    while (lo < hi) { const uint32_t mid = (lo + hi) / 2; if (member_end[mid] > span0) hi = mid; else lo = mid + 1; }
    uint32_t m = lo;
    uint32_t acc = 0;                                   // the wave's running register over [acc_from, pos), all of it inside member m
    bool have = false;
    for (uint64_t pos = span0; pos < span1; pos += CRC_STEP) {
        while (member_end[m] <= pos) m++;
        const uint64_t m_end = member_end[m];
        if (pos + CRC_STEP <= span1 && pos + CRC_STEP <= m_end) {
            const uint4* p = reinterpret_cast<const uint4*>(text + pos + (uint64_t)lane * CRC_LANE);
            uint32_t reg = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint4 v = p[q];
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    reg ^= w[j];
                    reg = T[3][reg & 0xFF] ^ T[2][(reg >> 8) & 0xFF] ^ T[1][(reg >> 16) & 0xFF] ^ T[0][reg >> 24];
                }
            }
            uint32_t x = crc_multmodp(k_mine, reg);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) x ^= __shfl_xor(x, o);
            acc = (have ? crc_multmodp(k_step, acc) : 0) ^ x;
            have = true;
            if (pos + CRC_STEP == m_end) {              // the member ends with this step: its word takes what the wave holds, unshifted
                if (lane == 0) atomicXor(&raw[m], acc);
                have = false;
                acc = 0;
            }
            continue;
        }
        // a member ends inside this step, or the text does: first what the wave holds, then lane by lane
        if (have) {
            if (lane == 0) atomicXor(&raw[m], crc_shift(x2n, acc, m_end - pos));
            have = false;
            acc = 0;
        }
        uint64_t q = pos + (uint64_t)lane * CRC_LANE;
        const uint64_t q_end = min(span1, q + CRC_LANE);
        uint32_t mm = m;
        while (q < q_end) {
            while (member_end[mm] <= q) mm++;
            const uint64_t e = member_end[mm];
            const uint64_t stop = min(q_end, e);
            uint32_t reg = 0;
            for (; q < stop; q++) reg = T[0][(reg ^ text[q]) & 0xFF] ^ (reg >> 8);
            atomicXor(&raw[mm], crc_shift(x2n, reg, e - stop));
        }
    }
    if (have && lane == 0) atomicXor(&raw[m], crc_shift(x2n, acc, member_end[m] - span1));
}

// =================================================================================================================================
// host
// =================================================================================================================================
struct Raw {                            // plain hipMalloc / hipFree: GBs of scratch per call must not stay in the context's pool
    void* p = nullptr;
    size_t cap = 0;
    ~Raw() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    void alloc(size_t bytes) {
        release();
        bytes = std::max<size_t>(bytes, 256);
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); throw HipError{e, "hipMalloc (inflate scratch)", __FILE__, __LINE__}; }
        cap = bytes;
    }
    void reserve(size_t bytes) { if (bytes > cap) alloc(bytes + bytes / 8); }      // contents are not kept
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
// What a call needs beside the text it returns: 16 x 2 B of cells per compressed byte and 64 KB per block — 13 GB for a 1 Gbp pair.
// ONE set per device and PROCESS, whichever context calls (the calls of a device take turns: a decode launch fills the chip anyway), kept
// between calls: allocating and freeing it per sample cost nothing on an idle box and, sporadically, a SECOND per sample beside another
// process that holds HBM (bench.py's own situation: profiles/r06_gz_e2e_trace.txt, "hold") — and a set per context would multiply it by
// the 16 engines of a `profile`.  A set that grew beyond SCRATCH_KEEP (an unusually large file) is freed behind its call.
constexpr size_t SCRATCH_KEEP = 20ull << 30;
struct InflateScratch {
    Raw gz, c1, c2, cnt, cells, res, jobs, plan, sfn, ffn, rwin, mend, x2n, raw;
    size_t bytes() const { return gz.cap + c1.cap + c2.cap + cnt.cap + cells.cap + res.cap + jobs.cap + plan.cap + sfn.cap + ffn.cap + rwin.cap + mend.cap + x2n.cap + raw.cap; }
    void release() { for (Raw* r : {&gz, &c1, &c2, &cnt, &cells, &res, &jobs, &plan, &sfn, &ffn, &rwin, &mend, &x2n, &raw}) r->release(); }
};
constexpr int MAX_DEVICES = 64;
struct DeviceScratch { std::mutex mu; InflateScratch s; };
DeviceScratch& device_scratch(int device) {
    static DeviceScratch* all = new DeviceScratch[MAX_DEVICES];      // (never destroyed: the process's HIP runtime may be gone by then)
    return all[std::min(std::max(device, 0), MAX_DEVICES - 1)];
}

// a small member through zlib (gzip wrapper: zlib checks CRC and ISIZE itself)
bool zlib_member(const uint8_t* gz, size_t n, size_t p, size_t* end, std::vector<uint8_t>& out) {
    constexpr size_t MAX_OUT = 1u << 20, MAX_IN = 1u << 18;
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, 16 + MAX_WBITS) != Z_OK) return false;
    out.resize(MAX_OUT);
    zs.next_in = const_cast<Bytef*>(gz + p);
    zs.avail_in = (uInt)std::min<size_t>(n - p, MAX_IN);
    zs.next_out = out.data();
    zs.avail_out = (uInt)MAX_OUT;
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END;
    if (ok) { *end = p + zs.total_in; out.resize(zs.total_out); }
    inflateEnd(&zs);
    return ok;
}

// one wavefront per job over the compressed words in S.gz (the spill arena's counter: S.cnt, word 2)
void launch_decode_jobs(sylph_ctx* ctx, InflateScratch& S, uint64_t n_words, const DecodeJob* jobs, uint32_t n_jobs, uint16_t* out_cells, const Spill& sp,
                        BlockResult* out) {
    hipStream_t s = ctx->stream;
    int n_cu = 256;
    (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device);
    uint32_t* const spill_next = reinterpret_cast<uint32_t*>(S.cnt.as<unsigned long long>() + 2);
    // the larger ring while all blocks' wavefronts fit on the chip beside each other with it (LDS: ~13 KB per wavefront -> 12 per CU)
    if (n_jobs <= (uint32_t)n_cu * 12 && !getenv("SYLPH_HIP_INFLATE_SMALL_RING"))
        hipLaunchKernelGGL(decode_kernel<4096>, dim3(n_jobs), dim3(64), 0, s, S.gz.as<uint32_t>(), n_words, jobs, out_cells, sp, spill_next, out);
    else
        hipLaunchKernelGGL(decode_kernel<2048>, dim3(n_jobs), dim3(64), 0, s, S.gz.as<uint32_t>(), n_words, jobs, out_cells, sp, spill_next, out);
    SY_HIP(hipGetLastError());
}

// A device's turn at its scratch: one inflate per device at a time.  On every way out — a decline included — the stream is idle before
// the next call may touch the scratch, and a set that outgrew SCRATCH_KEEP is freed.
struct ScratchTurn {
    DeviceScratch& ds;
    hipStream_t stream;
    std::lock_guard<std::mutex> turn;
    explicit ScratchTurn(sylph_ctx* ctx) : ds(device_scratch(ctx->device)), stream(ctx->stream), turn(ds.mu) {}
    ~ScratchTurn() { (void)hipStreamSynchronize(stream); if (ds.s.bytes() > SCRATCH_KEEP) ds.s.release(); }
};

// Cells a candidate's region holds per compressed byte: from the files' ISIZE where it can (bench.py's mate file: 5.3 -> 9: 7 GB of
// cells for a 1 Gbp pair instead of 12.7 — less to allocate, and less for the process to hand back when it ends).
// (SYLPH_HIP_INFLATE_REGION_RATIO: the tests' way to make every block outgrow its region)
uint64_t region_ratio(const Segments& files) {
    const char* rr_env = getenv("SYLPH_HIP_INFLATE_REGION_RATIO");
    return rr_env ? std::max(1, std::min(64, atoi(rr_env))) : region_ratio_from_isize(files, REGION_RATIO);
}

// The device phases of both roads (sylph_inflate_files: the files whole, one chain; sylph_inflate_stream_next: one slice per advancing
// file, one chain per slice), in the order they run.  Whose bytes the upload holds, the blocks the chains enter at, the walk, and what
// the CRC registers are compared with are the road's.
struct InflatePhases {
    sylph_ctx* ctx;
    hipStream_t s;
    InflateScratch& S;
    uint64_t n = 0, n_words = 0;                    // bytes of the upload, and the words that hold them
    std::vector<uint64_t> cand;                     // sorted candidate bits of the upload
    uint32_t K = 0;
    std::vector<DecodeJob> jobs;                    // per candidate: the first pass
    CellsLayout cells{};
    std::vector<BlockResult> res;                   // per candidate
    Raw cells2;                                     // the cells of the blocks decoded again
    RedoPlan redo;
    std::vector<PlanBlock> plan;                    // per chain block
    TextBuf text;
    uint64_t scratch = 0;                           // bytes of scratch this call asked for
    uint32_t x2n[64];

    InflatePhases(sylph_ctx* c, InflateScratch& S_, const char* text_what) : ctx(c), s(c->stream), S(S_), text(text_what) { crc_x2n_table(x2n); }

    void need(Raw& r, size_t bytes) { r.reserve(bytes); scratch += bytes; }

    // ---- candidates among the bytes [byte_lo, n) (trailers and later headers are scanned too: no harm, and members end anywhere).  The
    // road then adds the blocks its chains enter at, whatever their type (enter_at), and closes the list.
    void scan(uint64_t byte_lo, const char* phase) {
        const uint64_t cap1 = n / 8 + 4096, cap2 = n / 64 + 4096;
        need(S.c1, cap1 * 8);
        need(S.c2, cap2 * 8);
        need(S.cnt, 64);
        SY_HIP(hipMemsetAsync(S.cnt.p, 0, 64, s));
        unsigned long long* cnt = S.cnt.as<unsigned long long>();
        ScopedKernelTimer kt(ctx, "inflate_scan");
        HostPhase hp(ctx, phase);
        const uint32_t grid = (uint32_t)std::min<uint64_t>((n - byte_lo + SCAN_TPB - 1) / SCAN_TPB, 256 * 16);
        hipLaunchKernelGGL(scan1_kernel, dim3(std::max(grid, 1u)), dim3(SCAN_TPB), 0, s, S.gz.as<uint32_t>(), byte_lo, n, S.c1.as<uint64_t>(), cnt, cap1);
        SY_HIP(hipGetLastError());
        unsigned long long n1 = 0;
        ctx->read_back(&n1, cnt, 8);
        if (n1 > cap1) throw FormatDecline{"more header-like bit positions than the scan has room for"};
        if (n1) {
            hipLaunchKernelGGL(scan2_kernel, dim3((uint32_t)((n1 + SCAN2_TPB - 1) / SCAN2_TPB)), dim3(SCAN2_TPB), 0, s, S.gz.as<uint32_t>(), n * 8, S.c1.as<uint64_t>(),
                               cnt, cap1, S.c2.as<uint64_t>(), cnt + 1, cap2);
            SY_HIP(hipGetLastError());
        }
        cand = fetch_candidates(ctx, S.c2.p, cnt + 1, cap2, "more block-start candidates than the scan has room for");
    }
    void enter_at(uint64_t bit) { cand.insert(std::lower_bound(cand.begin(), cand.end(), bit), bit); }
    void close_candidates() {
        cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
        if (cand.size() >= (1ull << 31)) throw FormatDecline{"too many candidates"};
        K = (uint32_t)cand.size();
    }

    // ---- decode every candidate into its region (`jobs`, filled by the road: `ratio` cells per compressed byte up to the next candidate
    // of the span_bytes scanned, + REGION_SLACK)
    void decode_first_pass(uint64_t span_bytes, uint64_t ratio, const char* phase) {
        res.assign(K, BlockResult{});
        if (!K) return;
        cells = cells_layout(span_bytes, K, ratio, REGION_SLACK, SPILL_SLOTS, SPILL_CELLS);
        need(S.cells, cells.total * 2);
        need(S.res, (size_t)K * sizeof(BlockResult));
        need(S.jobs, (size_t)K * sizeof(DecodeJob));
        SY_HIP(hipMemsetAsync(S.cnt.as<unsigned long long>() + 2, 0, 8, s));      // the spill arena's counter
        {
            ScopedKernelTimer kt(ctx, "inflate_decode");
            HostPhase hp(ctx, phase);
            ctx->h2d(S.jobs.p, jobs.data(), (size_t)K * sizeof(DecodeJob));
            launch_decode_jobs(ctx, S, n_words, S.jobs.as<DecodeJob>(), K, S.cells.as<uint16_t>(), Spill{cells.spill_base, SPILL_SLOTS}, S.res.as<BlockResult>());
        }
        ctx->d2h(res.data(), S.res.p, (size_t)K * sizeof(BlockResult));
    }

    // ---- blocks of the chains that outgrew their region (BlockResult::flags bit 1): once more, each into a region of exactly its size,
    // with the window and the limit of its first pass
    void decode_outgrown(const std::vector<ChainBlock>& blocks, const char* phase) {
        redo = redo_plan(blocks, cand.data());
        const size_t J = redo.jobs.size();
        if (!J) return;
        for (size_t q = 0; q < J; q++) {
            const DecodeJob& first = jobs[blocks[redo.which[q]].cand];
            redo.jobs[q].have_window = first.have_window;
            redo.jobs[q].limit_words = first.limit_words;
        }
        ScopedKernelTimer kt(ctx, "inflate_decode");
        HostPhase hp(ctx, phase);
        Raw d_jobs2, d_res2;
        cells2.alloc((redo.cells + 64) * 2);
        d_jobs2.alloc(J * sizeof(DecodeJob));
        d_res2.alloc(J * sizeof(BlockResult));
        scratch += cells2.cap + d_jobs2.cap + d_res2.cap;
        ctx->h2d(d_jobs2.p, redo.jobs.data(), J * sizeof(DecodeJob));
        launch_decode_jobs(ctx, S, n_words, d_jobs2.as<DecodeJob>(), (uint32_t)J, cells2.as<uint16_t>(), Spill{0, 0}, d_res2.as<BlockResult>());
        std::vector<BlockResult> res2(J);
        ctx->d2h(res2.data(), d_res2.p, J * sizeof(BlockResult));
        for (size_t q = 0; q < J; q++) {
            const BlockResult& a = res[blocks[redo.which[q]].cand];
            const BlockResult& b2 = res2[q];
            if (b2.status != a.status || b2.n_out != a.n_out || b2.end_bit != a.end_bit || (b2.flags & 2))
                throw FormatDecline{"a block decoded a second time came out differently"};
        }
    }

    // ---- where every chain block's cells lie and where its bytes go; room for the windows of n_groups groups (chain_groups, summed
    // over the chains) if a block refers to one — a BGZF file's never do, and KB * 64 KB for it would be gigabytes
    static uint32_t chain_groups(uint32_t kb) { const uint32_t G = window_group(kb); return (kb + G - 1) / G; }
    void plan_blocks(const std::vector<ChainBlock>& blocks, uint64_t n_groups) {
        const size_t KB = blocks.size();
        plan.resize(KB);
        bool any_window = false;
        for (size_t i = 0; i < KB; i++) {
            const ChainBlock& cb = blocks[i];
            plan[i].cells = redo.region[i] != ~0ull ? cells2.as<uint16_t>() + redo.region[i] : S.cells.as<uint16_t>() + res[cb.cand].region;
            plan[i].out_off = cb.out_off;
            plan[i].n_out = cb.n_out;
            plan[i].flags = cb.flags;
            any_window |= (cb.flags & 1) != 0;
        }
        need(S.plan, KB * sizeof(PlanBlock));
        ctx->h2d(S.plan.p, plan.data(), KB * sizeof(PlanBlock));
        if (!any_window) return;
        need(S.sfn, KB * WINDOW * 2);
        need(S.ffn, (size_t)n_groups * WINDOW * 2);
        need(S.rwin, (size_t)n_groups * WINDOW);
    }

    // ---- the text of chain blocks [b0, b0 + kb), one chain whose groups begin at group g0: the windows resolved down the chain in
    // groups, from prev_window (null: none) in front of its first block; cells -> bytes
    void resolve_chain(uint32_t b0, uint32_t kb, uint64_t g0, const uint8_t* prev_window, const char* windows_phase, const char* translate_phase) {
        const uint32_t G = window_group(kb), NG = chain_groups(kb);
        uint16_t* sfn = S.sfn.as<uint16_t>() + (uint64_t)b0 * WINDOW;
        uint16_t* ffn = S.ffn.as<uint16_t>() + g0 * WINDOW;
        uint8_t* rwin = S.rwin.as<uint8_t>() + g0 * WINDOW;
        if (std::any_of(plan.begin() + b0, plan.begin() + b0 + kb, [](const PlanBlock& pb) { return (pb.flags & 1) != 0; })) {
            ScopedKernelTimer kt(ctx, "inflate_windows");
            HostPhase hp(ctx, windows_phase);
            static std::once_flag once;
            std::call_once(once, [] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(winfn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, WINDOW * 4); });
            hipLaunchKernelGGL(winfn_kernel, dim3(NG), dim3(WIN_TPB), WINDOW * 4, s, S.plan.as<PlanBlock>() + b0, kb, G, sfn, ffn);
            SY_HIP(hipGetLastError());
            hipLaunchKernelGGL(winchain_kernel, dim3(1), dim3(WIN_TPB), 0, s, ffn, NG, rwin, prev_window);
            SY_HIP(hipGetLastError());
        }
        ScopedKernelTimer kt(ctx, "inflate_translate");
        HostPhase hp(ctx, translate_phase);
        hipLaunchKernelGGL(translate_kernel, dim3(kb), dim3(TR_TPB), 0, s, S.plan.as<PlanBlock>() + b0, G, sfn, rwin, text.text());
        SY_HIP(hipGetLastError());
    }

    // ---- CRC-32 over the first `total` bytes of the text, cut at the ascending offsets m_end: the raw register of every piece
    std::vector<uint32_t> crc_raw(const std::vector<unsigned long long>& m_end, uint64_t total, const char* phase) {
        const uint32_t NM = (uint32_t)m_end.size();
        need(S.mend, (size_t)NM * 8);
        need(S.x2n, 256);
        need(S.raw, (size_t)NM * 4);
        std::vector<uint32_t> raw(NM);
        {
            ScopedKernelTimer kt(ctx, "inflate_crc");
            HostPhase hp(ctx, phase);
            ctx->h2d(S.mend.p, m_end.data(), (size_t)NM * 8);
            ctx->h2d(S.x2n.p, x2n, 256);
            SY_HIP(hipMemsetAsync(S.raw.p, 0, (size_t)NM * 4, s));
            if (total) {
                const uint64_t waves = (total + CRC_SPAN - 1) / CRC_SPAN;
                hipLaunchKernelGGL(crc_kernel, dim3((uint32_t)((waves + CRC_TPB / 64 - 1) / (CRC_TPB / 64))), dim3(CRC_TPB), 0, s, text.text(), total,
                                   S.mend.as<unsigned long long>(), NM, S.x2n.as<uint32_t>(), S.raw.as<uint32_t>());
                SY_HIP(hipGetLastError());
            }
        }
        ctx->d2h(raw.data(), S.raw.p, (size_t)NM * 4);
        return raw;
    }
};

// sylph_inflate_files.  Several files in one call are ONE stream of gzip members to everything below (`cat a.gz b.gz` is a gzip file):
// their bytes lie back to back on the device, one scan, one decode launch, one chain — the two mates of a pair share the latency of a
// block's wavefront (~15 ms whatever the file's size) instead of paying it one after the other.
struct InflateCall : InflatePhases {
    sylph_inflated* t;
    const Segments segs;
    const uint64_t body0;                           // the first member's first deflate byte (cand[0] = body0 * 8)
    std::vector<std::vector<uint8_t>> host_bytes;   // per Chain::host piece
    Chain chain;

    InflateCall(sylph_inflated* t_, InflateScratch& S_, Segments&& g)
        : InflatePhases(t_->ctx, S_, "hipMalloc (inflated text)"), t(t_), segs(std::move(g)), body0(member_body(segs.ptr[0], (size_t)segs.base[1], 0)) {
        n = segs.total();
        n_words = (n + 3) / 4;
    }

    // ---- the compressed bytes, padded with zero words
    void upload() {
        need(S.gz, (n_words + GZ_PAD_WORDS) * 4);
        HostPhase hp(ctx, "inflate: upload");
        upload_segments(ctx, S.gz.as<uint8_t>(), segs, GZ_PAD_WORDS * 4);
    }

    void find_candidates() {
        scan(body0, "inflate: scan");
        enter_at(body0 * 8);                        // the stream's first block
        close_candidates();
        t->n_candidates = K;
    }

    void decode_candidates() {
        const uint64_t ratio = region_ratio(segs);
        jobs.resize(K);
        for (uint32_t i = 0; i < K; i++) jobs[i] = decode_job(i, cand.data(), K, body0, n, ratio, REGION_SLACK);
        decode_first_pass(n - body0, ratio, "inflate: decode");
        if (getenv("SYLPH_HIP_INFLATE_STATS")) print_stats();
    }

    void print_stats() const {
        uint64_t sym = 0, far = 0, tb = 0, tt = 0, tmax = 0, cells_out = 0, moved_n = 0, dry_n = 0;
        for (const BlockResult& r : res) {
            sym += r.stats[0]; far += r.stats[1]; tb += r.stats[2]; tt += r.stats[3]; tmax = std::max<uint64_t>(tmax, r.stats[3]); cells_out += r.n_out;
            moved_n += r.region >= cells.spill_base; dry_n += (r.flags & 2) != 0;
        }
        fprintf(stderr, "[sylph_hip inflate] %llu candidates moved to the spill arena, %llu ran dry\n", (unsigned long long)moved_n, (unsigned long long)dry_n);
        fprintf(stderr, "[sylph_hip inflate] %u candidates: %llu symbol-loop turns, %llu copies from global memory, %llu cells; per wave: %.0f k-cycles mean (%.0f on headers + tables), %llu max\n",
                K, (unsigned long long)sym, (unsigned long long)far, (unsigned long long)cells_out, (double)tt / K, (double)tb / K, (unsigned long long)tmax);
    }

    // ---- the chain: which candidates are the stream, the members, every file's range in the text
    void walk_chain() {
        chain = chain_walk(segs, cand, res.data(), [&](size_t p, size_t* end, uint64_t* n_out) {
            std::vector<uint8_t> o;
            const size_t si = segs.find(p), gb = segs.base[si];
            if (!zlib_member(segs.ptr[si], segs.base[si + 1] - gb, p - gb, end, o)) return false;
            *end += gb;
            *n_out = o.size();
            if (!o.empty()) host_bytes.push_back(std::move(o));
            return true;
        });
        if (!chain.why.empty()) throw FormatDecline{chain.why};
        t->n_blocks = chain.blocks.size();
        t->n_members = chain.members.size();
        t->n_host_members = 0;
        for (const Member& m : chain.members) t->n_host_members += m.on_host;
        t->n = chain.total;
        t->files.assign(segs.ptr.size(), {~0ull, 0});
        for (const Member& m : chain.members) {                   // a file's text: from its first member's first byte to its last member's end
            auto& f = t->files[m.file];
            f.first = std::min<uint64_t>(f.first, m.out_begin);
            f.second = std::max<uint64_t>(f.second, m.out_end);
        }
        for (auto& f : t->files) if (f.first == ~0ull) throw FormatDecline{"a file without a gzip member"};
    }

    void decode_outgrown() {
        InflatePhases::decode_outgrown(chain.blocks, "inflate: decode again");
        t->n_redone = redo.jobs.size();
    }

    // ---- the text: the host's pieces copied in; the one chain's blocks, with no window in front of the first
    void write_text() {
        const uint32_t KB = (uint32_t)chain.blocks.size();
        text.grow(chain.total, 0, s);
        SY_HIP(hipMemsetAsync(text.text() + chain.total, 0, 256, s));
        for (size_t i = 0; i < chain.host.size(); i++) ctx->h2d(text.text() + chain.host[i].out_off, host_bytes[i].data(), host_bytes[i].size());
        if (!KB) return;
        plan_blocks(chain.blocks, chain_groups(KB));
        resolve_chain(0, KB, 0, nullptr, "inflate: windows", "inflate: translate");
    }

    // ---- CRC-32 of every member the device decoded, against its trailer (a chain without a block is zlib's alone, and checked)
    void check_crcs() {
        if (chain.blocks.empty()) return;
        const uint32_t NM = (uint32_t)chain.members.size();
        std::vector<unsigned long long> m_end(NM);
        for (uint32_t i = 0; i < NM; i++) m_end[i] = chain.members[i].out_end;
        const std::vector<uint32_t> raw = crc_raw(m_end, chain.total, "inflate: crc");
        for (uint32_t i = 0; i < NM; i++) {
            const Member& m = chain.members[i];
            if (m.on_host) continue;
            const uint32_t got = crc_finish(x2n, raw[i], m.out_end - m.out_begin);
            if (got != m.crc) {
                char msg[128];
                snprintf(msg, sizeof(msg), "member %u: CRC-32 %08x, the trailer says %08x", i, got, m.crc);
                throw FormatDecline{msg};
            }
        }
    }
};

void inflate_impl(sylph_inflated* t, const void* const* gzs, const uint64_t* n_bytes, uint32_t n_files) {
    sylph_ctx* ctx = t->ctx;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard dg(ctx->device);
    Segments segs = segments_of(gzs, n_bytes, n_files);
    for (uint32_t i = 0; i < n_files; i++)
        if (!member_body(segs.ptr[i], (size_t)n_bytes[i], 0)) throw FormatDecline{"not a gzip file"};
    if (segs.total() >= SYLPH_INFLATE_WHOLE_MAX_BYTES) throw FormatDecline{"3 GiB of gzip bytes or more: the host reader takes them"};
    if (segs.total() >= ctx->inflate_whole_max_bytes) throw FormatDecline{"more gzip bytes than \"inflate_whole_max_bytes\" allows in one piece"};
    ScratchTurn turn(ctx);
    InflateCall c(t, turn.ds.s, std::move(segs));
    c.upload();
    c.find_candidates();
    c.decode_candidates();
    c.walk_chain();
    c.decode_outgrown();
    c.write_text();
    c.check_crcs();
    t->buf = c.text.release();
    SY_HIP(hipStreamSynchronize(ctx->stream));      // the scratch is freed on the way out
}

// =================================================================================================================================
// the stream: the same phases over one slice per advancing file (bookkeeping: inflate_stream_plan.h)
// =================================================================================================================================
using namespace inflate_stream_plan;

struct StreamCall : InflatePhases {
    sylph_inflate_stream* st;
    sylph_inflated* t;
    const uint8_t* advance;
    const uint64_t* keep_from;
    struct FileSlice { uint32_t file; SliceCut sc; uint64_t off; };      // off: where the slice's bytes lie in the upload
    std::vector<FileSlice> slices;
    std::vector<uint64_t> entries;                  // per slice: entry_bit
    std::vector<SliceWalk> walks;                   // per slice
    std::vector<std::vector<std::vector<uint8_t>>> host_bytes;   // per slice, per host piece
    std::vector<ChainBlock> blocks;                 // all slices' chain blocks, out_off in the window's text
    std::vector<uint32_t> first_block;              // per slice: its first block in `blocks` (+ one behind the last)
    std::vector<uint64_t> kept, text_off;           // per file: kept bytes of the previous window; where the file's window begins
    uint64_t total = 0;

    StreamCall(sylph_inflate_stream* st_, sylph_inflated* t_, InflateScratch& S_, const uint8_t* adv, const uint64_t* keep)
        : InflatePhases(st_->ctx, S_, "hipMalloc (inflated window)"), st(st_), t(t_), advance(adv), keep_from(keep) {}

    uint32_t n_files() const { return st->n_files(); }

    void plan_slices(uint64_t slice_bytes) {
        slices.clear();
        uint64_t at = 0;
        for (uint32_t f = 0; f < n_files(); f++) {
            if ((advance && !advance[f]) || st->carry[f].finished) continue;
            const SliceCut sc = slice_cut(st->carry[f], st->n_bytes[f], slice_bytes);
            at = slice_begin(at);
            slices.push_back(FileSlice{f, sc, at});
            at += sc.end - sc.pos;
        }
        n = at;
        n_words = (n + 3) / 4;
    }

    void upload() {
        need(S.gz, (n_words + GZ_PAD_WORDS) * 4);
        HostPhase hp(ctx, "inflate stream: upload");
        SY_HIP(hipMemsetAsync(S.gz.p, 0, (n_words + GZ_PAD_WORDS) * 4, s));
        for (const FileSlice& fs : slices)
            if (fs.sc.end > fs.sc.pos) ctx->h2d(S.gz.as<uint8_t>() + fs.off, st->files[fs.file] + fs.sc.pos, (size_t)(fs.sc.end - fs.sc.pos));
    }

    // the bit of the upload where the slice's chain enters a block nobody may have found: the file's very first block, whatever its
    // type, or the block the carry stands in front of.  ~0: none.
    uint64_t entry_bit(const FileSlice& fs) const {
        const Carry& c = st->carry[fs.file];
        uint64_t file_bit;
        if (c.in_member) file_bit = c.bit;
        else if (c.bit == 0) {
            const size_t body = member_body(st->files[fs.file], (size_t)st->n_bytes[fs.file], 0);
            if (!body || body >= fs.sc.end) return ~0ull;
            file_bit = (uint64_t)body * 8;
        } else return ~0ull;
        return file_bit - fs.sc.pos * 8 + fs.off * 8;
    }

    void find_candidates() {
        scan(0, "inflate stream: scan");
        entries.clear();
        for (const FileSlice& fs : slices) {
            entries.push_back(entry_bit(fs));
            if (entries.back() != ~0ull) enter_at(entries.back());
        }
        close_candidates();
        t->n_candidates += K;
    }

    // the slice that holds byte `b` of the upload (the last one that begins at or in front of it)
    size_t slice_of(uint64_t b) const {
        size_t i = 0;
        while (i + 1 < slices.size() && slices[i + 1].off <= b) i++;
        return i;
    }

    void decode_candidates() {
        jobs.resize(K);
        for (uint32_t i = 0; i < K; i++) {
            DecodeJob j = decode_job(i, cand.data(), K, 0, n, st->ratio, REGION_SLACK);
            const size_t si = slice_of(cand[i] >> 3);
            const FileSlice& fs = slices[si];
            j.limit_words = (fs.off + (fs.sc.end - fs.sc.pos) + 3) / 4;       // (the zero bytes behind a slice are nobody's input)
            j.have_window = cand[i] == entries[si] ? (st->carry[fs.file].have_window ? 1u : 0u) : 1u;
            jobs[i] = j;
        }
        decode_first_pass(n, st->ratio, "inflate stream: decode");
    }

    // -> false: a slice's first block did not fit (the caller doubles the slice)
    bool walk_chains() {
        walks.clear();
        host_bytes.assign(slices.size(), {});
        for (size_t si = 0; si < slices.size(); si++) {
            const FileSlice& fs = slices[si];
            const uint8_t* gz = st->files[fs.file];
            const uint64_t fn = st->n_bytes[fs.file], lo = fs.off * 8, hi = (fs.off + (fs.sc.end - fs.sc.pos)) * 8;
            const int64_t shift = (int64_t)(fs.sc.pos * 8) - (int64_t)lo;
            std::vector<uint64_t> bits;
            std::vector<uint32_t> res_of;
            for (auto it = std::lower_bound(cand.begin(), cand.end(), lo); it != cand.end() && *it < hi; ++it) {
                bits.push_back((uint64_t)((int64_t)*it + shift));
                res_of.push_back((uint32_t)(it - cand.begin()));
            }
            walks.push_back(slice_walk(gz, fn, st->carry[fs.file], fs.sc, bits, res_of.data(), res.data(), shift, [&](size_t p, size_t* end, uint64_t* n_out) {
                std::vector<uint8_t> o;
                if (!zlib_member(gz, (size_t)fn, p, end, o)) return false;
                *n_out = o.size();
                if (!o.empty()) host_bytes[si].push_back(std::move(o));
                return true;
            }));
            if (!walks.back().why.empty()) throw FormatDecline{walks.back().why};
            if (walks.back().grow) return false;
        }
        return true;
    }

    // ---- where everything goes in the window's text: per file, the kept tail of its previous window, then the slice's new bytes
    void lay_out_text() {
        const uint32_t F = n_files();
        kept = kept_tails(st, keep_from, "sylph_inflate_stream");
        text_off.assign(F + 1, 0);
        std::vector<uint64_t> fresh(F, 0);
        for (size_t si = 0; si < slices.size(); si++) fresh[slices[si].file] = walks[si].total;
        for (uint32_t f = 0; f < F; f++) text_off[f + 1] = text_off[f] + kept[f] + fresh[f];
        total = text_off[F];
        blocks.clear();
        first_block.clear();
        for (size_t si = 0; si < slices.size(); si++) {
            first_block.push_back((uint32_t)blocks.size());
            const uint64_t base = text_off[slices[si].file] + kept[slices[si].file];
            for (ChainBlock cb : walks[si].blocks) { cb.out_off += base; blocks.push_back(cb); }
        }
        first_block.push_back((uint32_t)blocks.size());
        t->n = total;
        t->files.clear();
        for (uint32_t f = 0; f < F; f++) t->files.push_back({text_off[f], text_off[f + 1]});
        t->n_blocks = blocks.size();
        for (const SliceWalk& w : walks) for (const SliceMember& m : w.members) { t->n_members++; t->n_host_members += m.on_host; }
    }

    void decode_outgrown() {
        InflatePhases::decode_outgrown(blocks, "inflate stream: decode again");
        t->n_redone = redo.jobs.size();
    }

    // ---- the text: the kept tails and the host's pieces copied in; every slice's chain has its own groups, and the window its file's
    // earlier slices left in front of its first block
    void write_text() {
        const uint32_t KB = (uint32_t)blocks.size();
        text.grow(total, 0, s);
        SY_HIP(hipMemsetAsync(text.text() + total, 0, 256, s));
        for (uint32_t f = 0; f < n_files(); f++)
            if (kept[f]) SY_HIP(hipMemcpyAsync(text.text() + text_off[f], st->prev_text[f] + keep_from[f], kept[f], hipMemcpyDeviceToDevice, s));
        for (size_t si = 0; si < slices.size(); si++) {
            const uint64_t base = text_off[slices[si].file] + kept[slices[si].file];
            for (size_t i = 0; i < walks[si].host.size(); i++)
                ctx->h2d(text.text() + base + walks[si].host[i].out_off, host_bytes[si][i].data(), host_bytes[si][i].size());
        }
        if (!KB) return;
        uint64_t n_groups = 0;
        for (size_t si = 0; si < slices.size(); si++) if (first_block[si + 1] > first_block[si]) n_groups += chain_groups(first_block[si + 1] - first_block[si]);
        plan_blocks(blocks, n_groups);
        uint64_t g0 = 0;
        for (size_t si = 0; si < slices.size(); si++) {
            const uint32_t b0 = first_block[si], kb = first_block[si + 1] - b0, f = slices[si].file;
            if (!kb) continue;
            resolve_chain(b0, kb, g0, st->win + ((uint64_t)f * 2 + st->win_cur[f]) * WINDOW, "inflate stream: windows", "inflate stream: translate");
            g0 += chain_groups(kb);
        }
    }

    // ---- CRC-32: the pieces crc_kernel sees tile the window's text — per file its kept bytes (nobody's), then the slice's members, the
    // first of which may have begun in an earlier slice (its register is continued) and the last of which may end in a later one
    void check_crcs() {
        struct Piece { uint64_t end; int slice, member; };
        std::vector<Piece> pieces;
        std::vector<int> slice_of_file(n_files(), -1);
        for (size_t si = 0; si < slices.size(); si++) slice_of_file[slices[si].file] = (int)si;
        for (uint32_t f = 0; f < n_files(); f++) {
            if (kept[f]) pieces.push_back(Piece{text_off[f] + kept[f], -1, -1});
            const int si = slice_of_file[f];
            if (si < 0) continue;
            for (size_t m = 0; m < walks[si].members.size(); m++) pieces.push_back(Piece{text_off[f] + kept[f] + walks[si].members[m].out_end, si, (int)m});
        }
        const uint32_t NM = (uint32_t)pieces.size();
        std::vector<uint32_t> raw(NM, 0);
        if (total && NM && !blocks.empty()) {
            std::vector<unsigned long long> m_end(NM);
            for (uint32_t i = 0; i < NM; i++) m_end[i] = pieces[i].end;
            raw = crc_raw(m_end, total, "inflate stream: crc");
        }
        for (uint32_t i = 0; i < NM; i++) {
            if (pieces[i].slice < 0) continue;
            SliceWalk& w = walks[pieces[i].slice];
            const SliceMember& m = w.members[pieces[i].member];
            if (m.on_host) continue;
            const uint64_t n_new = m.out_end - m.out_begin;
            const uint32_t reg = crc_continue(x2n, m.crc_before, raw[i], n_new);
            if (!m.ends) { w.next.crc_raw = reg; continue; }
            const uint32_t got = crc_finish(x2n, reg, m.len_before + n_new);
            if (got != m.crc) {
                char msg[160];
                snprintf(msg, sizeof(msg), "file %u, member ending at text byte %llu of the window: CRC-32 %08x, the trailer says %08x", slices[pieces[i].slice].file,
                         (unsigned long long)pieces[i].end, got, m.crc);
                throw FormatDecline{msg};
            }
        }
    }

    // ---- what the next call needs: every advanced file's last 32 KiB of text and its carry
    void commit() {
        for (size_t si = 0; si < slices.size(); si++) {
            const uint32_t f = slices[si].file;
            const uint64_t n_new = walks[si].total;
            if (n_new) {
                uint8_t* base = st->win + (uint64_t)f * 2 * WINDOW;
                hipLaunchKernelGGL(window_tail_kernel, dim3(WINDOW / WIN_TPB), dim3(WIN_TPB), 0, s, base + (uint64_t)st->win_cur[f] * WINDOW,
                                   text.text() + text_off[f] + kept[f], n_new, base + (uint64_t)(st->win_cur[f] ^ 1) * WINDOW);
                SY_HIP(hipGetLastError());
                st->win_cur[f] ^= 1;
            }
            st->carry[f] = walks[si].next;
            st->n_slices++;
            st->text_bytes += n_new;
        }
        st->peak_scratch = std::max(st->peak_scratch, scratch);
        st->peak_window = std::max(st->peak_window, total);
    }
};

void stream_next_impl(sylph_inflate_stream* st, sylph_inflated* t, const uint8_t* advance, const uint64_t* keep_from) {
    sylph_ctx* ctx = st->ctx;
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard dg(ctx->device);
    ScratchTurn turn(ctx);                                         // the device's one scratch, for this call and not between calls
    uint64_t slice_bytes = st->slice_bytes;
    for (uint32_t attempt = 0;; attempt++) {
        StreamCall c(st, t, turn.ds.s, advance, keep_from);
        t->n_candidates = 0;
        c.plan_slices(slice_bytes);
        if (!c.slices.empty()) {
            c.upload();
            c.find_candidates();
            c.decode_candidates();
            if (!c.walk_chains()) {
                if (attempt >= MAX_GROW) throw FormatDecline{"a deflate block does not fit the slice, however often it was doubled"};
                SY_HIP(hipStreamSynchronize(ctx->stream));
                slice_bytes *= 2;
                continue;
            }
        }
        c.lay_out_text();
        c.decode_outgrown();
        c.write_text();
        c.check_crcs();
        c.commit();
        t->buf = c.text.release();
        SY_HIP(hipStreamSynchronize(ctx->stream));
        remember_window(st, t, c.text_off);
        return;
    }
}

}  // namespace
}  // namespace sylph

using namespace sylph;

extern "C" {

int sylph_inflate_files(sylph_ctx* ctx, const void* const* gz, const uint64_t* n_bytes, uint32_t n_files, int mem, sylph_inflated** out) {
    return decode_entry("sylph_inflate", false, ctx, gz, n_bytes, n_files, mem, out, inflate_impl);
}

int sylph_inflate(sylph_ctx* ctx, const void* gz, uint64_t n_bytes, int mem, sylph_inflated** out) {
    return sylph_inflate_files(ctx, &gz, &n_bytes, 1, mem, out);
}

int sylph_inflate_stream_open(sylph_ctx* ctx, const void* const* gz, const uint64_t* n_bytes, uint32_t n_files, int mem, uint64_t slice_bytes,
                              sylph_inflate_stream** out) {
    if (const int rc = stream_open_args("sylph_inflate_stream", ctx, gz, n_bytes, n_files, mem, out)) return rc;
    for (uint32_t i = 0; i < n_files; i++)
        if (!inflate_plan::member_body((const uint8_t*)gz[i], (size_t)n_bytes[i], 0)) { set_error("sylph_inflate_stream_open: declined: not a gzip file"); return SYLPH_ERR_FORMAT; }
    sylph_inflate_stream* st = nullptr;
    const int rc = guarded([&] {
        std::lock_guard<std::mutex> lock(ctx->mu);
        DeviceGuard dg(ctx->device);
        if (!slice_bytes) slice_bytes = ctx->inflate_slice_bytes ? ctx->inflate_slice_bytes : inflate_stream_plan::DEFAULT_SLICE;
        st = new sylph_inflate_stream(ctx, gz, n_bytes, n_files, std::max<uint64_t>(slice_bytes, inflate_stream_plan::MIN_SLICE));
        st->ratio = region_ratio(segments_of(gz, n_bytes, n_files));
        const hipError_t e = hipMalloc((void**)&st->win, (size_t)n_files * 2 * WINDOW);
        if (e != hipSuccess) { st->win = nullptr; (void)hipGetLastError(); throw HipError{e, "hipMalloc (inflate stream windows)", __FILE__, __LINE__}; }
        SY_HIP(hipMemsetAsync(st->win, 0, (size_t)n_files * 2 * WINDOW, ctx->stream));
    });
    if (rc != SYLPH_OK) {
        if (st) { std::lock_guard<std::mutex> lock(ctx->mu); DeviceGuard dg(ctx->device); if (st->win) (void)hipFree(st->win); delete st; }
        return rc;
    }
    ctx->refs.fetch_add(1);
    *out = st;
    return SYLPH_OK;
}

int sylph_inflate_stream_next(sylph_inflate_stream* st, const uint8_t* advance, const uint64_t* keep_from, sylph_inflated** window, uint8_t* finished) {
    return stream_next_entry("sylph_inflate_stream", st, advance, keep_from, window, finished, stream_next_impl);
}

int sylph_inflate_stream_info(const sylph_inflate_stream* st, uint64_t* n_slices, uint64_t* text_bytes, uint64_t* peak_scratch_bytes, uint64_t* peak_window_bytes) {
    return stream_info(st, n_slices, text_bytes, peak_scratch_bytes, peak_window_bytes);
}

void sylph_inflate_stream_destroy(sylph_inflate_stream* st) {
    stream_destroy(st, [](sylph_inflate_stream* g) { if (g->win) (void)hipFree(g->win); });
}

int sylph_inflated_file(const sylph_inflated* t, uint32_t i, const void** dev_text, uint64_t* n_bytes) {
    if (!t || i >= t->files.size()) { set_error("sylph_inflated_file: no such file"); return SYLPH_ERR_INVALID; }
    if (dev_text) *dev_text = t->text() + t->files[i].first;
    if (n_bytes) *n_bytes = t->files[i].second - t->files[i].first;
    return SYLPH_OK;
}

int sylph_inflated_text(const sylph_inflated* t, const void** dev_text, uint64_t* n_bytes) {
    if (!t) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    if (dev_text) *dev_text = t->text();
    if (n_bytes) *n_bytes = t->n;
    return SYLPH_OK;
}

int sylph_inflated_info(const sylph_inflated* t, uint64_t* n_members, uint64_t* n_blocks, uint64_t* n_candidates, uint64_t* n_host_members,
                        uint64_t* n_decoded_again) {
    if (!t) { set_error("null argument"); return SYLPH_ERR_INVALID; }
    if (n_members) *n_members = t->n_members;
    if (n_blocks) *n_blocks = t->n_blocks;
    if (n_candidates) *n_candidates = t->n_candidates;
    if (n_host_members) *n_host_members = t->n_host_members;
    if (n_decoded_again) *n_decoded_again = t->n_redone;
    return SYLPH_OK;
}

int sylph_inflated_read(sylph_inflated* t, uint64_t first, uint64_t n, void* host_out) {
    return guarded([&] {
        SY_REQUIRE(t && (host_out || n == 0), "null argument");
        SY_REQUIRE(first <= t->n && n <= t->n - first, "sylph_inflated_read: bytes [%llu, +%llu) of %llu", (unsigned long long)first, (unsigned long long)n,
                   (unsigned long long)t->n);
        if (!n) return;
        std::lock_guard<std::mutex> lock(t->ctx->mu);
        DeviceGuard dg(t->ctx->device);
        t->ctx->d2h(host_out, t->text() + first, n);
    });
}

void sylph_inflated_destroy(sylph_inflated* t) {
    if (!t) return;
    sylph_ctx* ctx = t->ctx;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        DeviceGuard dg(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);       // kernels that read the text may still be queued
        if (t->buf) (void)hipFree(t->buf);
        delete t;
    }
    ctx_unref(ctx);
}

}  // extern "C"
