// hash_variants.hip — round 5, VERDICT r04 #3: the k-mer loop of reads_kernel (csrc/reads.hip: two window extracts, canonical choice,
// mm_hash64, threshold mask) with the hash / threshold written seven ways and the canonical choice three ways, timed alone on the whole chip (5 waves per SIMD, like the
// kernel) on synthetic stream words held in LDS.  Reports ms per 8e8 k-mers and, with rocprofv3 --pmc SQ_INSTS_VALU, instructions
// per k-mer.  Build on the GPU box: hipcc --offload-arch=gfx950 -O3 -I sylph_amd/csrc tools/hash_variants.hip -o /tmp/hash_variants
//   V0  mm_hash64 as the compiler lowers it (64-bit multiplies)
//   V1  every "x + (x << n)" a v_lshl_add_u64 chain, the NOT folded into a v_bitop3: what reads_kernel ran up to round 11
//   V2  V1 with the LAST step on the high word only — h < T needs hi(h) unless hi(h) == hi(T): the mask is a superset (hi' <= hi(T),
//       carry from the low word ignored), the 1-in-200 candidates are re-hashed exactly anyway (the cooperative pass) and would have
//       to be re-TESTED there (2 false candidates per 2^32 k-mers: a tombstone path that the slots do not have today)
//   V3  every 64-bit step spelled out on 32-bit halves (v_alignbit / v_add_co / v_addc): exact
//   V4  V1 with * 265 as mul_const_u64 (device_common.h): v_mul_lo_u32 on the high word + ONE v_mad_u64_u32 for three 64-bit
//       instructions: mm_hash64_gfx950, what reads_kernel runs
//   V5  V4 with * 21 the same way (two for two; the mad's rate against v_lshl_add_u64's)
//   V6  V5 with the first step (* (2^21 + 1)) and the last (* (2^31 + 1)) the same way (two for two each)
//   V7  V4 with the canonical choice as two v_lshrrev_b64 (each left-aligned window down to its clean right-aligned form) + ONE v_min_f64
//       (min_u62, device_common.h) where V0-V6 spend v_cmp_lt_u64 + two v_cndmask_b32 + one shift: the fallback of round 13
//   V8  V4 with both windows BUILT right-aligned with clean tops (v_alignbit_b32 low word, v_bfe_u32 high word out of a cut that two
//       neighbouring k-mers share) + v_min_f64: what reads_kernel runs since round 13 (profiles/r13_canon_min.md)
//   V9  V8 with the threshold test's second instruction gone: v_cmpx_lt_u64 narrows EXEC to the hits, ONE no-return ds_xor_b32 under it
//       sets the k-mer's bit in the lane's own LDS column (seed_plan.h hit_const / hit_cleared / hit_decode: 16 constant VGPRs, the
//       bit in both halves of the word), s_mov_b64 puts EXEC back; per-lane column [MASKW][256] beside the stream, like the kernel's
// Every arm prints the sum of its masks: the exact arms (all but V2) must agree.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "device_common.h"
#include "seed_plan.h"

using namespace sylph;

__device__ __forceinline__ uint64_t hash_halves(uint64_t key) {
    uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32), c;
    auto add_shl = [&](int n) {      // (hi:lo) += (hi:lo) << n, 0 < n < 32
        const uint32_t slo = lo << n, shi = __builtin_amdgcn_alignbit(hi, lo, 32 - n);
        const uint32_t l2 = lo + slo;
        c = l2 < lo ? 1u : 0u;
        hi = hi + shi + c;
        lo = l2;
    };
    auto xor_shr = [&](int n) {      // (hi:lo) ^= (hi:lo) >> n, 0 < n < 32
        lo ^= __builtin_amdgcn_alignbit(hi, lo, n);
        hi ^= hi >> n;
    };
    add_shl(21); lo = ~lo; hi = ~hi;
    xor_shr(24);
    { const uint32_t l0 = lo, h0 = hi; add_shl(3); const uint32_t slo = l0 << 8, shi = __builtin_amdgcn_alignbit(h0, l0, 24); const uint32_t l2 = lo + slo; hi = hi + shi + (l2 < lo ? 1u : 0u); lo = l2; }
    xor_shr(14);
    { const uint32_t l0 = lo, h0 = hi; add_shl(2); const uint32_t slo = l0 << 4, shi = __builtin_amdgcn_alignbit(h0, l0, 28); const uint32_t l2 = lo + slo; hi = hi + shi + (l2 < lo ? 1u : 0u); lo = l2; }
    xor_shr(28);
    add_shl(31);
    return ((uint64_t)hi << 32) | lo;
}

// mm_hash64 with each multiply step either as its shift-add chain or as mul_const_u64
template <bool M265, bool M21, bool MENDS>
__device__ __forceinline__ uint64_t hash_spelled(uint64_t key) {
    uint64_t t = MENDS ? mul_const_u64<(1u << 21) + 1u>(key) : lshl_add_u64<0>(key << 21, key);
    {
        uint64_t sh;
        asm("v_lshrrev_b64 %0, 24, %1" : "=v"(sh) : "v"(t));
        uint32_t hi;
        asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(hi) : "v"((uint32_t)(t >> 32)), "v"((uint32_t)(sh >> 32)), "s"(0xFFFFFF00u));
        t = ((uint64_t)hi << 32) | ((uint32_t)t ^ (uint32_t)sh);
    }
    t = M265 ? mul_const_u64<265>(t) : lshl_add_u64<0>(t << 8, lshl_add_u64<3>(t, t));
    t = t ^ (t >> 14);
    t = M21 ? mul_const_u64<21>(t) : lshl_add_u64<4>(t, lshl_add_u64<2>(t, t));
    t = t ^ (t >> 28);
    return MENDS ? mul_const_u64<(1u << 31) + 1u>(t) : lshl_add_u64<0>(t << 31, t);
}

template <int V>
__device__ __forceinline__ void hash_and_mask(uint64_t canon, uint64_t thr, uint32_t& mask) {
    if constexpr (V == 2) {
        // steps 1..6 as V1, then hi(h) without the low word's carry; candidate <=> hi' <= hi(T)
        uint64_t t = lshl_add_u64<0>(canon << 21, canon);
        {
            uint64_t sh;
            asm("v_lshrrev_b64 %0, 24, %1" : "=v"(sh) : "v"(t));
            uint32_t hi;
            asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(hi) : "v"((uint32_t)(t >> 32)), "v"((uint32_t)(sh >> 32)), "s"(0xFFFFFF00u));
            t = ((uint64_t)hi << 32) | ((uint32_t)t ^ (uint32_t)sh);
        }
        t = lshl_add_u64<0>(t << 8, lshl_add_u64<3>(t, t));
        t = t ^ (t >> 14);
        t = lshl_add_u64<4>(t, lshl_add_u64<2>(t, t));
        t = t ^ (t >> 28);
        const uint32_t hi = (uint32_t)(t >> 32) + __builtin_amdgcn_alignbit((uint32_t)(t >> 32), (uint32_t)t, 1);
        const uint32_t thi = (uint32_t)(thr >> 32) + 1u;
        asm("v_cmp_lt_u32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(mask) : "v"(hi), "s"(thi) : "vcc");
    } else {
        const uint64_t h = V == 0 ? mm_hash64(canon) : V == 1 ? hash_spelled<false, false, false>(canon) : V == 3 ? hash_halves(canon)
                         : V == 4 ? mm_hash64_gfx950(canon) : V == 5 ? hash_spelled<true, true, false>(canon) : hash_spelled<true, true, true>(canon);
        asm("v_cmp_lt_u64 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(mask) : "v"(h), "s"(thr) : "vcc");
    }
}

// (Bm, the image of the word in front of the group, is read by the left-aligned extracts of V0-V7 only; fword / rword: device_common.h)
template <int K, int T, int V>
__device__ __forceinline__ void kmer_step(uint32_t A0, uint32_t A1, uint32_t A2, uint32_t Bm, uint32_t B0, uint32_t B1, uint32_t B2, uint64_t thr, uint32_t& mask) {
    constexpr int D = 64 - 2 * K;
    static_assert(2 * K <= 62, "min_u62");
    if constexpr (V == 8) {
        constexpr int HB = 2 * K - 32, T0 = T & ~1;
        const uint32_t cf = fword<2 * T0>(A0, A1, A2), cr = rword<2 * T0 + 32>(B0, B1, B2);
        const uint32_t fhi = __builtin_amdgcn_ubfe(cf, 32 - HB - 2 * (T - T0), HB), rhi = __builtin_amdgcn_ubfe(cr, 2 * (T - T0), HB);
        const uint32_t flo = fword<2 * T + HB>(A0, A1, A2), rlo = rword<2 * T>(B0, B1, B2);
        hash_and_mask<4>(min_u62(((uint64_t)fhi << 32) | flo, ((uint64_t)rhi << 32) | rlo), thr, mask);
        return;
    }
    uint32_t fhi, flo, rhi, rlo;
    if constexpr (T == 0) { fhi = A0; flo = A1; }
    else { fhi = __builtin_amdgcn_alignbit(A0, A1, 32 - 2 * T); flo = __builtin_amdgcn_alignbit(A1, A2, 32 - 2 * T); }
    constexpr int OFF = 2 * T - D;
    if constexpr (OFF < 0) { rlo = __builtin_amdgcn_alignbit(B0, Bm, OFF + 32); rhi = __builtin_amdgcn_alignbit(B1, B0, OFF + 32); }
    else if constexpr (OFF == 0) { rlo = B0; rhi = B1; }
    else { rlo = __builtin_amdgcn_alignbit(B1, B0, OFF); rhi = __builtin_amdgcn_alignbit(B2, B1, OFF); }
    const uint64_t f = ((uint64_t)fhi << 32) | flo, rc = ((uint64_t)rhi << 32) | rlo;
    if constexpr (V == 7) {
        uint64_t fs, rs;
        asm("v_lshrrev_b64 %0, %1, %2" : "=v"(fs) : "n"(D), "v"(f));
        asm("v_lshrrev_b64 %0, %1, %2" : "=v"(rs) : "n"(D), "v"(rc));
        hash_and_mask<4>(min_u62(fs, rs), thr, mask);
    } else {
        hash_and_mask<V>((f < rc ? f : rc) >> D, thr, mask);
    }
}
template <int K, int T0, int V>
__device__ __forceinline__ void steps8(uint32_t A0, uint32_t A1, uint32_t A2, uint32_t Bm, uint32_t B0, uint32_t B1, uint32_t B2, uint64_t thr, uint32_t& mask) {
    kmer_step<K, T0 + 0, V>(A0, A1, A2, Bm, B0, B1, B2, thr, mask); kmer_step<K, T0 + 1, V>(A0, A1, A2, Bm, B0, B1, B2, thr, mask);
    kmer_step<K, T0 + 2, V>(A0, A1, A2, Bm, B0, B1, B2, thr, mask); kmer_step<K, T0 + 3, V>(A0, A1, A2, Bm, B0, B1, B2, thr, mask);
    kmer_step<K, T0 + 4, V>(A0, A1, A2, Bm, B0, B1, B2, thr, mask); kmer_step<K, T0 + 5, V>(A0, A1, A2, Bm, B0, B1, B2, thr, mask);
    kmer_step<K, T0 + 6, V>(A0, A1, A2, Bm, B0, B1, B2, thr, mask); kmer_step<K, T0 + 7, V>(A0, A1, A2, Bm, B0, B1, B2, thr, mask);
}

// one lane = one "read" of n_grp groups of 16 k-mers over LDS stream words, as reads_kernel's hot loop
template <int V>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void loop_kernel(uint32_t n_grp, uint64_t thr, uint32_t* __restrict__ out) {
    __shared__ uint32_t sF[256 * 10 + 64];
    for (uint32_t i = threadIdx.x; i < 256 * 10 + 64; i += 256) sF[i] = (i + blockIdx.x * 977u) * 2654435761u ^ (i * 40503u);
    __syncthreads();
    const uint32_t w0 = threadIdx.x * 9, sh = 32u - (threadIdx.x & 15u) * 2u;
    uint32_t raw = sF[w0], nxt = sF[w0 + 1], j = 0;
    auto next_word = [&]() {
        const uint32_t a = (uint32_t)((((uint64_t)raw << 32) | nxt) >> sh);
        raw = nxt;
        nxt = sF[w0 + 2 + (j++ % 8)];
        return a;
    };
    uint32_t A0 = next_word(), A1 = next_word(), A2 = next_word();
    uint32_t Bm = 0, B0 = rcword(A0), B1 = rcword(A1), B2 = rcword(A2);
    uint32_t acc = 0;
    for (uint32_t g = 0; g < n_grp; g++) {
        uint32_t mask = 0;
        steps8<31, 0, V>(A0, A1, A2, Bm, B0, B1, B2, thr, mask);
        steps8<31, 8, V>(A0, A1, A2, Bm, B0, B1, B2, thr, mask);
        A0 = A1; A1 = A2; A2 = next_word();
        Bm = B0; B0 = B1; B1 = B2; B2 = rcword(A2);
        acc += mask;
    }
    out[blockIdx.x * 256 + threadIdx.x] = acc;
}

// V9: the hit bit goes to LDS under the compare's own lane mask.  Nothing else runs under the narrowed EXEC; the block restores the EXEC
// of the loop (exec0) and clobbers vcc only.  The blocks have no side effect the compiler knows of and take no "memory" clobber — the hash
// chains of neighbouring k-mers stay free to interleave, the stream reads free to move — and are kept in program order among themselves
// and against the clearing stores by passing the column's address THROUGH every one of them (hit_chain_begin / hit_chain_end close the
// chain against ordinary loads and stores on both sides of the loop).
__device__ __forceinline__ void hit_bit_to_lds(uint64_t h, uint64_t thr, uint32_t& addr, uint32_t bit, uint64_t exec0) {
    asm("v_cmpx_lt_u64 vcc, %1, %2\n\tds_xor_b32 %0, %3\n\ts_mov_b64 exec, %4" : "+v"(addr) : "v"(h), "s"(thr), "v"(bit), "s"(exec0) : "vcc");
}
__device__ __forceinline__ void hit_clear_lower(uint32_t& addr, uint32_t zero) { asm("ds_write_b16 %0, %1" : "+v"(addr) : "v"(zero)); }
__device__ __forceinline__ void hit_chain_begin(uint32_t& addr) { asm volatile("" : "+v"(addr) : : "memory"); }
__device__ __forceinline__ void hit_chain_end(uint32_t& addr) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(addr) : : "memory"); }
template <int K, int T>
__device__ __forceinline__ void kmer_step_lds(uint32_t A0, uint32_t A1, uint32_t A2, uint32_t B0, uint32_t B1, uint32_t B2, uint64_t thr, uint32_t& addr,
                                              const uint32_t (&bit)[16], uint64_t exec0) {
    constexpr int HB = 2 * K - 32, T0 = T & ~1;
    const uint32_t cf = fword<2 * T0>(A0, A1, A2), cr = rword<2 * T0 + 32>(B0, B1, B2);
    const uint32_t fhi = __builtin_amdgcn_ubfe(cf, 32 - HB - 2 * (T - T0), HB), rhi = __builtin_amdgcn_ubfe(cr, 2 * (T - T0), HB);
    const uint32_t flo = fword<2 * T + HB>(A0, A1, A2), rlo = rword<2 * T>(B0, B1, B2);
    hit_bit_to_lds(mm_hash64_gfx950(min_u62(((uint64_t)fhi << 32) | flo, ((uint64_t)rhi << 32) | rlo)), thr, addr, bit[T], exec0);
}
template <int K, int T0>
__device__ __forceinline__ void steps8_lds(uint32_t A0, uint32_t A1, uint32_t A2, uint32_t B0, uint32_t B1, uint32_t B2, uint64_t thr, uint32_t& addr,
                                           const uint32_t (&bit)[16], uint64_t exec0) {
    kmer_step_lds<K, T0 + 0>(A0, A1, A2, B0, B1, B2, thr, addr, bit, exec0); kmer_step_lds<K, T0 + 1>(A0, A1, A2, B0, B1, B2, thr, addr, bit, exec0);
    kmer_step_lds<K, T0 + 2>(A0, A1, A2, B0, B1, B2, thr, addr, bit, exec0); kmer_step_lds<K, T0 + 3>(A0, A1, A2, B0, B1, B2, thr, addr, bit, exec0);
    kmer_step_lds<K, T0 + 4>(A0, A1, A2, B0, B1, B2, thr, addr, bit, exec0); kmer_step_lds<K, T0 + 5>(A0, A1, A2, B0, B1, B2, thr, addr, bit, exec0);
    kmer_step_lds<K, T0 + 6>(A0, A1, A2, B0, B1, B2, thr, addr, bit, exec0); kmer_step_lds<K, T0 + 7>(A0, A1, A2, B0, B1, B2, thr, addr, bit, exec0);
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void loop_kernel_lds(uint32_t n_grp, uint64_t thr, uint32_t* __restrict__ out) {
    __shared__ uint32_t sF[256 * 10 + 64];
    __shared__ uint32_t s_mask[seed_plan::MASKW][256];
    for (uint32_t i = threadIdx.x; i < 256 * 10 + 64; i += 256) sF[i] = (i + blockIdx.x * 977u) * 2654435761u ^ (i * 40503u);
    const uint32_t rows = seed_plan::rows_used(n_grp * 2);             // n_grp <= 2 * MASKW
    for (uint32_t w = 0; w < rows; w++) s_mask[w][threadIdx.x] = 0;
    __syncthreads();
    const uint32_t w0 = threadIdx.x * 9, sh = 32u - (threadIdx.x & 15u) * 2u;
    uint32_t raw = sF[w0], nxt = sF[w0 + 1], j = 0;
    auto next_word = [&]() {
        const uint32_t a = (uint32_t)((((uint64_t)raw << 32) | nxt) >> sh);
        raw = nxt;
        nxt = sF[w0 + 2 + (j++ % 8)];
        return a;
    };
    uint32_t A0 = next_word(), A1 = next_word(), A2 = next_word();
    uint32_t B0 = rcword(A0), B1 = rcword(A1), B2 = rcword(A2);
    uint32_t bit[16], zero;
#pragma unroll
    for (int t = 0; t < 16; t++) asm("v_mov_b32 %0, %1" : "=v"(bit[t]) : "s"(seed_plan::hit_const(t)));   // opaque: held in registers, not rebuilt per k-mer
    asm("v_mov_b32 %0, 0" : "=v"(zero));
    const uint64_t exec0 = __builtin_amdgcn_read_exec();
    uint32_t addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)&s_mask[0][threadIdx.x];
    hit_chain_begin(addr);
    for (uint32_t g = 0; g < n_grp; g++) {
        steps8_lds<31, 0>(A0, A1, A2, B0, B1, B2, thr, addr, bit, exec0);
        steps8_lds<31, 8>(A0, A1, A2, B0, B1, B2, thr, addr, bit, exec0);
        A0 = A1; A1 = A2; A2 = next_word();
        B0 = B1; B1 = B2; B2 = rcword(A2);
        if (seed_plan::hit_clear_after(g)) hit_clear_lower(addr, zero);
        else addr += seed_plan::hit_word_offset(2, 256);
    }
    hit_chain_end(addr);
    uint32_t acc = 0;
    for (uint32_t w = 0; w < rows; w++) {
        const uint32_t m = seed_plan::hit_decode(s_mask[w][threadIdx.x]);
        acc += (m >> 16) + (m & 0xFFFFu);
    }
    out[blockIdx.x * 256 + threadIdx.x] = acc;
}

template <int V>
void run(const char* what, uint32_t* out) {
    const uint32_t n_grp = 120 / 16 + 1;                 // a 150 bp read: 120 k-mers -> 7.5 groups (8 here)
    const uint32_t blocks = 26042;                       // as many workgroups as a 1 Gbp batch has blocks of 256 reads
    const uint64_t thr = UINT64_MAX / 200;
    hipEvent_t a, b;
    (void)hipEventCreate(&a); (void)hipEventCreate(&b);
    float best = 1e9f;
    for (int rep = 0; rep < 5; rep++) {
        (void)hipEventRecord(a, 0);
        if constexpr (V == 9) hipLaunchKernelGGL(loop_kernel_lds, dim3(blocks), dim3(256), 0, 0, n_grp, thr, out);
        else hipLaunchKernelGGL(loop_kernel<V>, dim3(blocks), dim3(256), 0, 0, n_grp, thr, out);
        (void)hipEventRecord(b, 0);
        (void)hipEventSynchronize(b);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, a, b);
        if (rep) best = ms < best ? ms : best;
    }
    const double kmers = (double)blocks * 256 * n_grp * 16;
    static uint32_t* host = (uint32_t*)malloc((size_t)blocks * 256 * 4);
    (void)hipMemcpy(host, out, (size_t)blocks * 256 * 4, hipMemcpyDeviceToHost);
    uint64_t sum = 0;
    for (size_t i = 0; i < (size_t)blocks * 256; i++) sum += host[i];
    printf("%-58s %7.4f ms per launch of %.3e k-mers = %7.4f ms per 8.0e8 k-mers (one 1 Gbp sample of 2 x 150 bp)  masks %016llx\n", what, best, kmers,
           best * 8.0e8 / kmers, (unsigned long long)sum);
}

int main() {
    uint32_t* out;
    (void)hipMalloc(&out, (size_t)26042 * 256 * 4);
    run<0>("V0 mm_hash64 (compiler's multiplies)", out);
    run<1>("V1 v_lshl_add_u64 chains (reads_kernel up to round 11)", out);
    run<2>("V2 V1, last step + threshold on the high word (superset)", out);
    run<3>("V3 32-bit halves throughout (exact)", out);
    run<4>("V4 V1, * 265 as mul + mad: mm_hash64_gfx950 (the kernel of round 12)", out);
    run<5>("V5 V4, * 21 as mul + mad too", out);
    run<6>("V6 V5, first and last step too", out);
    run<7>("V7 V4, canonical choice: 2 x v_lshrrev_b64 + v_min_f64", out);
    run<8>("V8 V4, clean right-aligned windows + v_min_f64 (the kernel)", out);
    run<9>("V9 V8, hit bit by ds_xor_b32 under v_cmpx's lane mask", out);
    run<4>("V4 again (clocks settled)", out);
    run<7>("V7 again", out);
    run<8>("V8 again", out);
    run<9>("V9 again", out);
    run<8>("V8 a third time", out);
    run<9>("V9 a third time", out);
    return 0;
}
