// text_lines.h — the lines of a text found on the device, shared by fastq.hip and fasta.hip: the newlines of a lane's 16 bytes of the
// aligned stream (one 16-byte load per lane, exact SWAR byte test; a tile is 4 KiB) and, behind an exclusive scan of the tiles' newline
// counts, the start of every line.  Each including translation unit gets its own copy of the kernel.
#pragma once
#include "common.h"
#include "device_common.h"

namespace sylph {
namespace {

constexpr int FQ_TPB = 256, FQ_TILE = FQ_TPB * 16;       // one 16-byte load per lane

// what the kernels leave for the host: [0] bytes of text without its trailing blank space, [1] first bad record (~0: none),
// [2] bases of the text, [3] flags (1: more than FQ_MAX_TRAILING blank bytes behind the text), [4] newlines, counted in 64 bits (the
// tiles' line numbers are a 32-bit scan: a text with 2^32 lines or more is refused, not mis-numbered)
struct FqWords { unsigned long long n_eff, bad_rec, n_bases, flags, n_nl; };

// bit 7 of every byte of x that equals '\n' (exact: no borrow runs from one byte into the next)
__device__ __forceinline__ uint32_t newline_flags(uint32_t x) {
    x ^= 0x0A0A0A0Au;
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | x | 0x7F7F7F7Fu);
}

// the lane's 16 bytes of the aligned stream `al` (text = al + bias): newline flags of its four dwords, bytes outside [0, n_eff) cleared
__device__ __forceinline__ void lane_flags(const uint8_t* __restrict__ al, uint32_t bias, uint64_t n_eff, uint64_t tile, uint32_t f[4],
                                           int64_t& i0) {
    const uint64_t p = tile * FQ_TILE + (uint64_t)threadIdx.x * 16;       // position in the aligned stream
    i0 = (int64_t)p - (int64_t)bias;                                        // index of the lane's first byte in the text
    f[0] = f[1] = f[2] = f[3] = 0;
    if (i0 >= (int64_t)n_eff || i0 + 16 <= 0) return;
    const uint4 v = *reinterpret_cast<const uint4*>(al + p);
    f[0] = newline_flags(v.x); f[1] = newline_flags(v.y); f[2] = newline_flags(v.z); f[3] = newline_flags(v.w);
    if (i0 < 0 || i0 + 16 > (int64_t)n_eff) {                               // the text's first / last lane: byte by byte
#pragma unroll
        for (int d = 0; d < 4; d++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int64_t i = i0 + d * 4 + b;
                if (i < 0 || i >= (int64_t)n_eff) f[d] &= ~(0x80u << (8 * b));
            }
    }
}

__global__ __launch_bounds__(FQ_TPB) void fq_lines_kernel(const uint8_t* __restrict__ al, uint32_t bias, const FqWords* __restrict__ w,
                                                          const uint32_t* __restrict__ tile_base, uint64_t n_lines,
                                                          uint64_t* __restrict__ line_start) {
    __shared__ uint32_t s_wave[FQ_TPB / 64];
    uint32_t f[4];
    int64_t i0;
    const uint64_t n_eff = w->n_eff;
    lane_flags(al, bias, n_eff, blockIdx.x, f, i0);
    const uint32_t c = __popc(f[0]) + __popc(f[1]) + __popc(f[2]) + __popc(f[3]);
    uint64_t ord = (uint64_t)tile_base[blockIdx.x] + block_excl_sum<FQ_TPB>(c, s_wave, nullptr);   // newlines in front of this lane's bytes
    if (blockIdx.x == 0 && threadIdx.x == 0) { line_start[0] = 0; line_start[n_lines] = n_eff + 1; }
    if (!c) return;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        uint32_t m = f[d];
        while (m) {
            const int b = (__ffs((int)m) - 1) >> 3;                         // lowest address first
            m &= ~(0x80u << (8 * b));
            ord++;
            if (ord < n_lines) line_start[ord] = (uint64_t)(i0 + d * 4 + b) + 1;
        }
    }
}

}  // namespace
}  // namespace sylph
