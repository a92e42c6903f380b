// reads_block.h — the steps of the short-read seeding kernel (reads.hip reads_kernel: one lane per record), in the order the kernel
// runs them for every pass of a block: load_stream, stage_offsets | record_geometry, deal_by_length, hash_record, count_hits,
// publish_markers, list_survivors, finish_survivors | close_slots (common.h: shared with the position kernel).  The LDS they share is ReadsLds; which stream words, mask bits and
// records belong to a block is seed_plan.h's arithmetic (free of HIP, tested on the CPU).  Every value of the hash loop lives in named
// locals of hash_record: the steps pass scalars, never per-lane state in a struct (HitRegs, the 17 constant registers of the LDS hit
// bits, is the one bundle: built once per kernel, read only).
// What the compiler makes of the steps was held against the one-body kernel they came from (profiles/seed_steps_census.txt); three things
// in their signatures come from that: ReadsLds travels by value and its pointers are LDS-typed, the steps' global pointers carry no
// __restrict__ (the kernel's arguments do: a second set of alias scopes changed the schedule and spilled in two instances), and
// stage_offsets gets its first index by value.
#pragma once
#include "common.h"
#include "device_common.h"
#include "seed_plan.h"
#include "sketch_session.h"

namespace sylph {
namespace {

using namespace seed_plan;

template <int K>
struct KC {
    static constexpr uint64_t MASK = (1ull << (2 * K)) - 1;
};

// The workgroup's LDS.  Two arrays take over the place of two others, and nowhere else:
//   * m0 / m1, the records' markers, lie over the staged offsets `off`: the lanes have taken their stream bases from them by then
//     (record_geometry; a block with several passes keeps its offsets in global memory instead);
//   * hist, the dealing's histogram, lies over `first`, which is not in use before count_hits.
// (The pointers carry the LDS address space in their type: every access through them is an LDS instruction whatever the optimiser makes
//  of the code around it — with plain pointers the two arms of record_geometry, staged and global offsets, were merged into flat loads.)
#define SY_LDS __attribute__((address_space(3)))
template <int TPB>
struct ReadsLds {
    SY_LDS uint32_t* sF;                   // the block's stream: lds_words(rt) words (dynamic)
    SY_LDS uint64_t* off;                  // staged record offsets: offs_staged(TPB) + 4
    SY_LDS uint64_t *m0, *m1;              // per lane: the record's markers                                          (over off)
    SY_LDS uint32_t (*mask)[TPB];          // [MASKW][TPB] hit masks, one column per record; the free rows hold the survivors' list
    SY_LDS uint32_t* wave;                 // the scan's wave totals
    SY_LDS uint32_t* first;                // per lane: its first hit of the pass (bit 31: has markers); [TPB] = the pass's total
    SY_LDS uint32_t* hist;                 // 64 bins of the dealing                                                  (over first)
    SY_LDS uint32_t* rel;                  // per lane: its record's stream base
    SY_LDS uint16_t *perm, *nh;            // the dealing: lane -> record slot it hashes; per lane: its record's hashed k-mers
    SY_LDS uint32_t *redo, *redo_deal;     // HV == 2: a candidate failed the exact test; the pass is ragged
};
template <int TPB>
__device__ __forceinline__ ReadsLds<TPB> reads_lds() {
    constexpr int OFFS = offs_staged(TPB);
    extern __shared__ uint32_t sF[];
    __shared__ uint64_t s_off[OFFS + 4];
    __shared__ uint32_t s_mask[MASKW][TPB];
    __shared__ uint32_t s_wave[TPB / 64];
    __shared__ uint32_t s_first[TPB + 1], s_rel[TPB];
    __shared__ uint16_t s_perm[TPB], s_nh[TPB];
    __shared__ uint32_t s_redo, s_redo_deal;
    static_assert((OFFS + 4) >= 2 * TPB, "the marker arrays alias the staged offsets");
    static_assert(TPB + 1 >= 64, "the histogram aliases s_first");
    using W = SY_LDS uint32_t*; using D = SY_LDS uint64_t*; using H = SY_LDS uint16_t*;
    return ReadsLds<TPB>{(W)sF, (D)s_off, (D)s_off, (D)s_off + TPB, (SY_LDS uint32_t(*)[TPB])s_mask, (W)s_wave, (W)s_first, (W)s_first, (W)s_rel,
                         (H)s_perm, (H)s_nh, (W)&s_redo, (W)&s_redo_deal};
}

// 64-bit window of 32 bases starting at stream base `b`: base b in bits 63:62
__device__ __forceinline__ uint64_t win64(const SY_LDS uint32_t* sF, uint32_t b) {
    const uint32_t j = b >> 4, ph = (b & 15u) * 2u;
    const uint64_t x = ((uint64_t)sF[j] << 32) | sF[j + 1];
    return (x << ph) | ((uint64_t)sF[j + 2] >> (32u - ph));   // ph = 0: second term shifts a 32-bit value by 32 -> 0
}

// reverse complement of the k-mer in the top 2K bits of x (anything below is ignored): field order reversed by a 64-bit
// bit reversal, the two bits of every field swapped back, complement = bitwise NOT of a 2-bit code
template <int K>
__device__ __forceinline__ uint64_t revcomp_top(uint64_t x) {
    const uint64_t rev = __brevll(x);
    const uint64_t y = ((rev & 0x5555555555555555ull) << 1) | ((rev >> 1) & 0x5555555555555555ull);
    return (~y) & KC<K>::MASK;
}

// every other base of a 32-base window, first base most significant (the order pair_kmer builds its 16-mers in): ev = bases
// 0, 2, .., 30, od = bases 1, 3, .., 31.  Done on the two 32-bit halves: two shift-or steps bring the wanted fields of every
// byte pair side by side (bytes 3 and 1 then hold four bases each), and ONE v_perm_b32 picks those bytes out of both halves —
// 9-11 instructions per 16-mer where five 64-bit shift/or/and stages took about 25.
__device__ __forceinline__ uint32_t even_fields_to_bytes31(uint32_t w) {
    uint32_t t = w & 0xCCCCCCCCu;
    t = (t | (t << 2)) & 0xF0F0F0F0u;
    return t | (t << 4);                       // byte 3 = bases 0,2,4,6 of the half, byte 1 = bases 8,10,12,14
}
__device__ __forceinline__ void evenodd16(uint64_t x, uint32_t& ev, uint32_t& od) {
    const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
    // __builtin_amdgcn_perm(a, b, sel): selector 0-3 = bytes of b, 4-7 = bytes of a
    ev = __builtin_amdgcn_perm(even_fields_to_bytes31(hi), even_fields_to_bytes31(lo), 0x07050301u);
    od = __builtin_amdgcn_perm(even_fields_to_bytes31(hi << 2), even_fields_to_bytes31(lo << 2), 0x07050301u);
}

// One k-mer of a group of 16: T = index inside the group.  A0..A2: the lane-aligned forward words of the group and the two
// behind it; B0..B2: their reverse-complement images.  Forward k-mer = stream bits [2T, 2T + 2K) of A0:A1:A2 counted from A0's
// bit 31; its reverse complement = bits [2T, 2T + 2K) of the little-endian multiword B2:B1:B0 counted from B0's bit 0.  Both are
// built RIGHT-ALIGNED with the top 64 - 2K bits zero: the low word is one funnel shift, the high word's 2K - 32 bits are a
// v_bfe_u32 out of A0 / B1 where the field lies inside that word, else out of a 32-bit cut that the k-mers T0 = T & ~1 and T0 + 1 share
// (2.5 instructions per window at most).  Two values below
// 2^62 take their minimum in ONE v_min_f64 (min_u62, device_common.h) where compare + two selects + the shift of the winner
// took four.
// The threshold test, LB false: v_cmp + v_addc_co_u32 shift the compare's lane mask into the lane's `mask` register, one bit per k-mer (the
// second instruction only transposes that bit).  LB true (round 14, seed_plan.h "hit bits set by LDS atomics"): v_cmpx narrows EXEC to
// the hits, ONE no-return ds_xor_b32 under it sets the bit in the record's mask column — `mask` is the LDS byte address of the group's
// word there, hit.bit[T] the k-mer's constant — and s_mov_b64 puts back the EXEC of the loop (hit.exec0).  Nothing else runs under the
// narrowed EXEC; the block clobbers vcc only and takes no "memory" clobber: the blocks are kept in program order among themselves and
// against hit_clear_lower by passing the address THROUGH every one of them, and against ordinary loads and stores by hit_chain_begin /
// hit_chain_end on both sides of the loop.
struct HitRegs {
    uint32_t bit[16];     // hit_const(T), held in registers for the whole loop (opaque to the compiler: never rebuilt per k-mer)
    uint32_t zero;
    uint64_t exec0;       // EXEC of the loop (hash_record reads it in front of its loop: the loop's control flow is scalar)
};
// (built once per kernel: 17 moves per pass are a seventh of what the spelling saves a 150 bp read)
__device__ __forceinline__ HitRegs hit_regs() {
    HitRegs r;
#pragma unroll
    for (int t = 0; t < 16; t++) asm("v_mov_b32 %0, %1" : "=v"(r.bit[t]) : "s"(hit_const(t)));
    asm("v_mov_b32 %0, 0" : "=v"(r.zero));
    r.exec0 = 0;
    return r;
}
__device__ __forceinline__ void hit_clear_lower(uint32_t& addr, uint32_t zero) { asm("ds_write_b16 %0, %1" : "+v"(addr) : "v"(zero)); }
__device__ __forceinline__ void hit_chain_begin(uint32_t& addr) { asm volatile("" : "+v"(addr) : : "memory"); }
// (the compiler counts no LDS operation of the blocks: wait for them here, in front of the column's readers and the barrier)
__device__ __forceinline__ void hit_chain_end(uint32_t& addr) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(addr) : : "memory"); }

template <int K, int T, int HV, bool LB>
__device__ __forceinline__ void kmer_step(uint32_t A0, uint32_t A1, uint32_t A2, uint32_t B0, uint32_t B1, uint32_t B2,
                                          uint64_t thr, uint32_t& mask, const HitRegs& hit) {
    static_assert(2 * K <= 62 && 2 * K > 32, "min_u62 wants both windows below 2^62; the high word holds 2K - 32 bits");
    constexpr int HB = 2 * K - 32, T0 = T & ~1;
    uint32_t fhi, rhi;
    if constexpr (2 * T + HB <= 32) {                                                                // the field lies inside A0 / B1: no cut
        fhi = __builtin_amdgcn_ubfe(A0, 32 - HB - 2 * T, HB); rhi = __builtin_amdgcn_ubfe(B1, 2 * T, HB);
    } else {
        const uint32_t cf = fword<2 * T0>(A0, A1, A2), cr = rword<2 * T0 + 32>(B0, B1, B2);          // shared by k-mers T0 and T0 + 1
        fhi = __builtin_amdgcn_ubfe(cf, 32 - HB - 2 * (T - T0), HB); rhi = __builtin_amdgcn_ubfe(cr, 2 * (T - T0), HB);
    }
    const uint32_t flo = fword<2 * T + HB>(A0, A1, A2), rlo = rword<2 * T>(B0, B1, B2);
    const uint64_t canon = min_u62(((uint64_t)fhi << 32) | flo, ((uint64_t)rhi << 32) | rlo);       // seeding.rs:134-139
    if constexpr (HV == 2) {
        // candidate test on the HIGH word: u = hi(h) + 1 - (the low word's carry), `thr` holds hi(T) + 1 here (reads_kernel)
        const uint32_t u = mm_hash64_gfx950_hi1(canon);
        if constexpr (LB)
            asm("v_cmpx_ge_u32 vcc, %2, %1\n\tds_xor_b32 %0, %3\n\ts_mov_b64 exec, %4"
                : "+v"(mask) : "v"(u), "s"((uint32_t)thr), "v"(hit.bit[T]), "s"(hit.exec0) : "vcc");
        else
            asm("v_cmp_ge_u32 vcc, %2, %1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(mask) : "v"(u), "s"((uint32_t)thr) : "vcc");
    } else {
        const uint64_t h = HV ? mm_hash64_gfx950(canon) : mm_hash64(canon);
        if constexpr (LB)
            asm("v_cmpx_lt_u64 vcc, %1, %2\n\tds_xor_b32 %0, %3\n\ts_mov_b64 exec, %4"
                : "+v"(mask) : "v"(h), "s"(thr), "v"(hit.bit[T]), "s"(hit.exec0) : "vcc");
        else
            asm("v_cmp_lt_u64 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(mask) : "v"(h), "s"(thr) : "vcc");
    }
}
template <int K, int T0, int HV, bool LB>
__device__ __forceinline__ void kmer_steps8(uint32_t A0, uint32_t A1, uint32_t A2, uint32_t B0, uint32_t B1, uint32_t B2,
                                            uint64_t thr, uint32_t& mask, const HitRegs& hit) {
    kmer_step<K, T0 + 0, HV, LB>(A0, A1, A2, B0, B1, B2, thr, mask, hit);
    kmer_step<K, T0 + 1, HV, LB>(A0, A1, A2, B0, B1, B2, thr, mask, hit);
    kmer_step<K, T0 + 2, HV, LB>(A0, A1, A2, B0, B1, B2, thr, mask, hit);
    kmer_step<K, T0 + 3, HV, LB>(A0, A1, A2, B0, B1, B2, thr, mask, hit);
    kmer_step<K, T0 + 4, HV, LB>(A0, A1, A2, B0, B1, B2, thr, mask, hit);
    kmer_step<K, T0 + 5, HV, LB>(A0, A1, A2, B0, B1, B2, thr, mask, hit);
    kmer_step<K, T0 + 6, HV, LB>(A0, A1, A2, B0, B1, B2, thr, mask, hit);
    kmer_step<K, T0 + 7, HV, LB>(A0, A1, A2, B0, B1, B2, thr, mask, hit);
}

// 1. The block's stream words [0, n_words) from the aligned coordinate a0 on, as a 2-bit big-endian stream.  Only the first and the
// last block of a batch reach outside [0, n_al): every other block loads unconditionally.
template <int ENC, int TPB>
__device__ __forceinline__ void load_stream(SY_LDS uint32_t* sF, const uint8_t* bases_al, uint64_t n_al, uint32_t blk, int64_t a0, uint32_t n_words) {
    const uint32_t tid = threadIdx.x;
    const bool interior = block_starts_inside(blk) && (uint64_t)(a0 + (int64_t)n_words * 16) <= n_al;
    // (the block's first word is a scalar address — a0 may be negative: it is only dereferenced at words inside [0, n_al) — and a lane
    //  adds a 32-bit byte offset: no 64-bit coordinate per lane, in either arm)
    const uintptr_t src0 = (uintptr_t)bases_al + (uintptr_t)(ENC == 0 ? a0 : (a0 >> 2));
    constexpr uint32_t WB = ENC == 0 ? 16u : 4u;                   // bytes of input per stream word
    if (interior) {
        if constexpr (ENC == 0) {
            for (uint32_t ci = tid; ci < n_words; ci += TPB) sF[ci] = pack16_fwd(*reinterpret_cast<const uint4*>(src0 + ci * WB));
        } else {
            for (uint32_t ci = tid; ci < n_words; ci += TPB)
                sF[ci] = __builtin_amdgcn_perm(0u, *reinterpret_cast<const uint32_t*>(src0 + ci * WB), 0x00010203u);
        }
    } else {
        // word ci starts at coordinate a0 + 16 ci: inside [0, n_al) for ci in [ci_lo, ci_hi) (stream_word_range, scalars)
        uint32_t ci_lo, ci_hi;
        stream_word_range(a0, n_al, n_words, ci_lo, ci_hi);
        for (uint32_t ci = tid; ci < n_words; ci += TPB) {
            const bool inside = ci >= ci_lo && ci < ci_hi;
            if constexpr (ENC == 0) {                              // ASCII: 16 bytes -> one word
                uint4 v = make_uint4(0, 0, 0, 0);
                if (inside) v = *reinterpret_cast<const uint4*>(src0 + ci * WB);
                sF[ci] = pack16_fwd(v);
            } else {                                               // packed input: 4 bytes, first base in bits 7:6 of byte 0
                uint32_t w = 0;
                if (inside) w = *reinterpret_cast<const uint32_t*>(src0 + ci * WB);
                sF[ci] = __builtin_amdgcn_perm(0u, w, 0x00010203u);
            }
        }
    }
}

// 2. The offsets of the block's records [R0, R1) (+ the mate-1 offset in front of a block that starts with a mate 2, + two behind) into
// LDS, from index w_lo on.  False — nothing staged — where they do not fit or the block takes several passes.
// (Record indices are 32-bit — blk_rec holds them so — and what a lane adds to the scalar w_lo is a 32-bit count.)
template <int TPB>
__device__ __forceinline__ bool stage_offsets(const ReadsLds<TPB> s, const uint64_t* off, uint64_t n_rec, uint32_t R0, uint32_t R1,
                                              uint32_t w_lo) {
    const uint32_t w_hi = R1 + min((uint32_t)n_rec - R1, 2u);   // last offset index needed: min(R1 + 2, n_rec), R1 <= n_rec < 2^32
    const uint32_t n_stage = w_hi - w_lo + 1;
    const bool in_lds = n_stage <= (uint32_t)(offs_staged(TPB) + 4) && (R1 - R0) <= (uint32_t)TPB;
    if (in_lds) {
        const uint64_t* const src = off + w_lo;
        for (uint32_t t = threadIdx.x; t < n_stage; t += TPB) s.off[t] = src[t];
    }
    return in_lds;
}

// 3. The lane's record r (if `active`: the pass has a record for this lane): the k-mers the reference hashes of it, its stream base, and
// the stream bases of its marker windows (seed_plan.h MarkerBases; none asked for: 0, 0).  The 64-bit offsets end HERE: a single read loads its two, a mate the three of its
// pair (its own two are among them), the lengths are tested against the halo in 64 bits and everything that leaves is a length of at
// most RH or a base relative to the block — one 32-bit add on an offset's low word (rb = rel_bias of the block).  The steps behind the
// hash loop want nothing else, and four offsets carried through the loop were eight registers.
// True: the record (or a mate of its pair) is longer than the halo — the host reruns the batch through the position kernel.
template <int K, int TPB>
__device__ __forceinline__ bool record_geometry(const ReadsLds<TPB> s, const uint64_t* off, bool in_lds, uint32_t w_lo, uint32_t r,
                                                bool active, int paired, uint32_t rb, int avx2_compat, int want_markers, uint32_t& nh,
                                                uint32_t& rel, uint32_t& ba, uint32_t& bb) {
    uint64_t o0 = 0, o1 = 0, o2 = 0;                              // single: the record's start and end; paired: s1, s2, e2 of its pair
    if (active) {
        const uint32_t r0 = paired ? (r & ~1u) : r;               // (w_lo is even where the input is paired: r0 >= w_lo)
        if (in_lds) {
            const SY_LDS uint64_t* const o = s.off + (r0 - w_lo);
            o0 = o[0]; o1 = o[1];
            if (paired) o2 = o[2];
        } else {
            const uint64_t* const o = off + r0;
            o0 = o[0]; o1 = o[1];
            if (paired) o2 = o[2];
        }
    }
    const uint64_t d1 = o1 - o0, d2 = o2 - o1;                   // (paired: both mates' lengths; an idle lane: 0, 0)
    const bool too_long = d1 > (uint64_t)RH || (paired && d2 > (uint64_t)RH);
    const bool mate2 = paired && (r & 1u);
    const uint32_t L = too_long ? 0u : (uint32_t)(mate2 ? d2 : d1);
    const uint32_t rel1 = record_rel32(o0, rb), rel2 = record_rel32(o1, rb);
    nh = (uint32_t)n_hashed_kmers(L, K, avx2_compat, 0);
    rel = active ? (mate2 ? rel2 : rel1) : 0u;
    MarkerBases mk{0u, 0u};
    if (want_markers && active && !too_long) mk = paired ? pair_marker_bases(rel1, rel2, (uint32_t)d1, (uint32_t)d2) : single_marker_bases(rel, L);
    ba = mk.ba; bb = mk.bb;
    return too_long;
}

// 4. A wavefront walks as many k-mer groups as its LONGEST record has: deal the pass's records to the lanes in order of
// length (counting sort by the number of half-groups, longest first; ties in any order), so that trimmed reads of
// 35..151 bp cost a wavefront what its own quartile needs instead of what the longest read of 64 needs.  Only the
// hash loop runs in this order — hit masks are stored under the record's own slot and everything after the loop is
// indexed by record again, so the output does not depend on the dealing.  A pass of equally long records (every
// lane in one bin) is hashed as it lies.
// Gives the record slot this lane hashes with that record's stream base and k-mers, and the mask rows the pass's longest record
// reaches; returns whether the pass was dealt (uniform over the workgroup).  LB (hit bits by LDS atomics): the lane's own column is
// zeroed over those rows — in a dealt pass another lane hashes into it, behind the dealing's last barrier.
template <int TPB, bool LB>
__device__ __forceinline__ bool deal_by_length(const ReadsLds<TPB> s, uint32_t nh, uint32_t rel, uint32_t& slot, uint32_t& rel_h, uint32_t& nh_h,
                                               uint32_t& rows) {
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    if (tid < 64) s.hist[tid] = 0;
    s.rel[tid] = rel;
    s.nh[tid] = (uint16_t)nh;
    // Round 6 (VERDICT r05 #4a): whether the pass needs dealing at all is asked FIRST — one compare with the first record's count and
    // one LDS word — and a pass of equally long records (every pass of an untrimmed 2 x 150 bp sample) skips the histogram: its 256
    // atomic adds all went to ONE counter (the LDS serialises them), then a scan and a barrier, to find that nothing moves.
    if (tid == 0) *s.redo_deal = 0;
    __syncthreads();
    if (__ballot(nh != (uint32_t)s.nh[0]) && lane == 0) *s.redo_deal = 1;
    __syncthreads();
    const bool dealt = *s.redo_deal != 0;                      // uniform over the workgroup
    const uint32_t bin = deal_bin(nh);                         // nh <= RH - 20: at most 48 half-groups
    uint32_t hg_max = half_groups(nh), arrival = 0, hc = 0;
    if (dealt) {
        arrival = atomicAdd((uint32_t*)&s.hist[bin], 1u);
        __syncthreads();
        hc = s.hist[lane];
        // the longest record of the pass (uniform over the workgroup: every wavefront reads the same histogram): its lowest
        // non-empty bin; the mask rows above its words are free in this pass (see list_survivors)
        const uint64_t bins_used = __ballot(hc != 0u);
        hg_max = bins_used ? 63u - (uint32_t)(__ffsll((unsigned long long)bins_used) - 1) : 0u;   // half-groups of 8 k-mers
    }
    rows = rows_used(hg_max);
    if constexpr (LB) {
        // (two rows per turn, counted in a scalar: row `rows` itself, where rows is odd, belongs to the survivors' list — not in use yet)
        const uint32_t rows_u = (uint32_t)__builtin_amdgcn_readfirstlane((int)rows);
        for (uint32_t w = 0; w < rows_u; w += 2) { s.mask[w][tid] = 0; s.mask[w + 1][tid] = 0; }
    }
    if (dealt) {
        const uint32_t incl = wave_inclusive_sum(hc);
        s.perm[(uint32_t)__shfl((int)(incl - hc), (int)bin) + arrival] = (uint16_t)tid;
        __syncthreads();
    }
    slot = dealt ? s.perm[tid] : tid;
    rel_h = dealt ? s.rel[slot] : rel;
    nh_h = dealt ? s.nh[slot] : nh;
    return dealt;
}

// 5. The hit masks of record slot `slot` (stream base rel_h, nh_h k-mers): every lane of the wavefront walks the groups of the
// wavefront's longest record (seed_plan.h hash_hi_word: how far that reads).
template <int K, int HV, int TPB, bool LB>
__device__ __forceinline__ void hash_record(const ReadsLds<TPB> s, uint32_t slot, uint32_t rel_h, uint32_t nh_h, uint64_t thr_loop,
                                            const HitRegs& hit_consts) {
    const SY_LDS uint32_t* const sF = s.sF;
    const uint32_t nh_max = wave_max_u32(nh_h);     // a scalar (LB: the blocks restore ONE EXEC, no lane may leave the loop alone)
    if (nh_max) {
        // lane-aligned stream words A(j) = bases [rel + 16 j, rel + 16 j + 16): one LDS read and one 64-bit shift each
        const uint32_t w0 = rel_h >> 4, sh = 32u - (rel_h & 15u) * 2u;      // sh in [2, 32]
        uint32_t raw = sF[w0], nxt = sF[w0 + 1];
        auto next_word = [&](uint32_t j) {                                   // A(j), advancing the raw pair to j + 1
            const uint32_t a = (uint32_t)((((uint64_t)raw << 32) | nxt) >> sh);
            raw = nxt;
            nxt = sF[w0 + j + 2];
            return a;
        };
        uint32_t A0 = next_word(0), A1 = next_word(1), A2 = next_word(2);
        uint32_t B0 = rcword(A0), B1 = rcword(A1), B2 = rcword(A2);
        const uint32_t n_half = half_groups(nh_max);                         // half-groups of 8 k-mers (uniform per wave)
        // k-mer i <-> bit 31 - (i & 31) of word i >> 5: a group of 16 is one 16-bit half of its word, even groups the
        // upper half (seed_plan.h group_half).  Stored as halves (ds_write_b16): no "is the word complete" bookkeeping in the loop;
        // whatever a half that was never written holds lies beyond nh and is cleared with the tail in count_hits.
        SY_LDS uint16_t* const mask_half = (SY_LDS uint16_t*)&s.mask[0][slot];
        const uint32_t n_grp = n_half >> 1;
        if constexpr (LB) {
            // the same walk with the hit bits set in LDS: the column's words are zero (deal_by_length), every k-mer's block xors its
            // constant into the group's word, the lower half is cleared behind an even group, count_hits decodes (seed_plan.h)
            HitRegs hit = hit_consts;
            hit.exec0 = __builtin_amdgcn_read_exec();
            uint32_t addr = (uint32_t)(uintptr_t)&s.mask[0][slot];
            hit_chain_begin(addr);
            for (uint32_t g = 0; g < n_grp; g++) {
                kmer_steps8<K, 0, HV, true>(A0, A1, A2, B0, B1, B2, thr_loop, addr, hit);
                kmer_steps8<K, 8, HV, true>(A0, A1, A2, B0, B1, B2, thr_loop, addr, hit);
                A0 = A1; A1 = A2; A2 = next_word(g + 3);
                B0 = B1; B1 = B2; B2 = rcword(A2);
                if (hit_clear_after(g)) hit_clear_lower(addr, hit.zero);
                else addr += hit_word_offset(2, TPB);
            }
            if (n_half & 1u) {
                kmer_steps8<K, 0, HV, true>(A0, A1, A2, B0, B1, B2, thr_loop, addr, hit);
                if (hit_clear_after(n_grp)) hit_clear_lower(addr, hit.zero);
            }
            hit_chain_end(addr);
            return;
        }
        const HitRegs hit{};
        // whole groups of 16: one straight-line block (the odd half-group of a record's tail is done after the loop —
        // with the test inside the loop the second half of every group lived in its own basic block and took two
        // extra register moves per k-mer)
        for (uint32_t g = 0; g < n_grp; g++) {
            uint32_t mask = 0;
            kmer_steps8<K, 0, HV, false>(A0, A1, A2, B0, B1, B2, thr_loop, mask, hit);
            kmer_steps8<K, 8, HV, false>(A0, A1, A2, B0, B1, B2, thr_loop, mask, hit);
            A0 = A1; A1 = A2; A2 = next_word(g + 3);
            B0 = B1; B1 = B2; B2 = rcword(A2);
            mask_half[group_half(g, TPB)] = (uint16_t)mask;
        }
        if (n_half & 1u) {                                                   // a last half-group: its 8 k-mers are the top byte
            uint32_t mask = 0;
            kmer_steps8<K, 0, HV, false>(A0, A1, A2, B0, B1, B2, thr_loop, mask, hit);
            mask_half[group_half(n_grp, TPB)] = (uint16_t)(mask << 8);
        }
    }
}

// 6. The real hits of the lane's own record (k-mer i < nh; the bits beyond are cleared from its last word), scanned over the
// workgroup: lanes are in record order, so `first` — the hits in front of this lane's — is file order.  Returns the lane's count.
// `decode`: the words are as the LDS atomics left them (hit_decode, its own inverse: true in the pass's FIRST round only — the second
// round of HV == 2 finds decoded words with the struck candidates gone).
template <int TPB>
__device__ __forceinline__ uint32_t count_hits(const ReadsLds<TPB> s, uint32_t nh, bool decode, uint32_t& first, uint32_t& total) {
    const uint32_t tid = threadIdx.x;
    uint32_t cnt = 0;
    const uint32_t nw = mask_words(nh);
    for (uint32_t w = 0; w + 1 < nw; w++) {
        uint32_t m = s.mask[w][tid];
        if (decode) { m = hit_decode(m); s.mask[w][tid] = m; }
        cnt += __popc(m);
    }
    if (nw) {                                                   // the record's last word: bits beyond k-mer nh - 1 are not its own
        const uint32_t m0 = s.mask[nw - 1][tid];
        const uint32_t m = (decode ? hit_decode(m0) : m0) & tail_mask(nh);
        s.mask[nw - 1][tid] = m;
        cnt += __popc(m);
    }
    first = block_excl_sum<TPB>(cnt, (uint32_t*)s.wave, &total);
    return cnt;
}

// 7. Survivors (1 in c k-mers) are finished COOPERATIVELY: lanes publish where their hits start in the pass and their
// record's markers; then the pass's hits are dealt one per lane (finish_survivors).  (Each lane looping over its own hits made every
// wavefront run the ~95-instruction body as often as its busiest lane had hits: 3-4 times for ~0.6 hits per lane.)
template <int TPB>
__device__ __forceinline__ void publish_markers(const ReadsLds<TPB> s, uint32_t cnt, uint32_t first, uint32_t total, uint32_t ba, uint32_t bb) {
    const uint32_t tid = threadIdx.x;
    uint64_t m0 = 0, m1 = 0;
    const uint32_t has = (cnt && bb) ? 1u : 0u;                  // (record_geometry: which records carry markers, and where their windows start)
    if (has) {
        const uint64_t wa64 = win64(s.sF, ba), wb64 = win64(s.sF, bb);
        uint32_t ea, oa, eb, ob;
        evenodd16(wa64, ea, oa);
        evenodd16(wb64, eb, ob);
        m0 = (uint64_t)ea | ((uint64_t)eb << 32);
        m1 = (uint64_t)oa | ((uint64_t)ob << 32);
    }
    s.m0[tid] = m0;
    s.m1[tid] = m1;
    s.first[tid] = first | (has << 31);
    if (tid == 0) s.first[TPB] = total;
}

// 8. The pass's survivors as a list, hit number -> (lane, k-mer index), written by the lanes that own them (a lane has
// 0.6 hits on average: a short loop over its own mask words) into the mask rows no record of this pass reaches.
// Without room for the whole list (records near READ_HALO, or c so small that a pass has thousands of hits) finish_survivors finds
// owner and k-mer by a search over the lanes' start offsets and a walk over the owner's masks instead — what it always did before
// round 3: ~150 instructions per wavefront and pass more.  Returns whether the list was written (uniform over the workgroup).
template <int TPB>
__device__ __forceinline__ bool list_survivors(const ReadsLds<TPB> s, uint32_t nh, uint32_t cnt, uint32_t first, uint32_t total, uint32_t rows) {
    const uint32_t tid = threadIdx.x;
    SY_LDS uint32_t* const s_owner = &s.mask[0][0] + rows * TPB;
    const bool is_listed = listed(total, rows, TPB);
    if (is_listed && cnt) {
        uint32_t p = first;
        for (uint32_t w = 0; w < mask_words(nh); w++) {
            uint32_t m = s.mask[w][tid];
            while (m) {
                const uint32_t bpos = (uint32_t)__clz((int)m);
                s_owner[p++] = tid | ((w * 32 + bpos) << OWNER_LANE_BITS);
                m &= ~(0x80000000u >> bpos);
            }
        }
    }
    return is_listed;
}

// 9. The pass's hits, one per lane — owner and k-mer index from the list, or by a search over the TPB start offsets and the owner's
// hit masks — re-hashed from the LDS stream and written as finished 32 B records, consecutive lanes to consecutive slots.
// HV == 2: the loop's test yields a superset; a candidate that fails the exact test is struck from its record's mask and *s.redo set —
// the caller redoes the pass's bookkeeping from count_hits on.
template <int K, int HV, int TPB>
__device__ __forceinline__ void finish_survivors(const ReadsLds<TPB> s, bool is_listed, uint32_t rows, uint32_t total, uint32_t base_prev,
                                                 uint32_t slot_cap, uint64_t thr, uint64_t rec_base, uint64_t pass, int paired, int avx2_compat,
                                                 uint64_t out0, OccRec* slot_rec, uint32_t* slot_key, int key_sh) {
    const SY_LDS uint32_t* const s_owner = &s.mask[0][0] + rows * TPB;
    for (uint32_t hix = threadIdx.x; hix < total; hix += TPB) {
        uint32_t lo, i = 0, f;
        if (is_listed) {
            const uint32_t ow = s_owner[hix];
            lo = ow & ((1u << OWNER_LANE_BITS) - 1u);
            i = ow >> OWNER_LANE_BITS;
            f = s.first[lo];
        } else {
            lo = 0;
            uint32_t hi = TPB;                                          // owner: the last lane whose first hit is <= hix
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if ((s.first[mid] & 0x7FFFFFFFu) <= hix) lo = mid; else hi = mid;
            }
            // (lanes without hits share the start offset of the next lane with hits: the LAST lane with that offset that
            //  actually owns hix is the one whose successor starts beyond it — the search above returns exactly that lane)
            f = s.first[lo];
            uint32_t j = hix - (f & 0x7FFFFFFFu);                       // the j-th hit of lane `lo`
            for (uint32_t w = 0; w < MASKW; w++) {
                uint32_t m = s.mask[w][lo];
                const uint32_t c = (uint32_t)__popc(m);
                if (j >= c) { j -= c; continue; }
                for (; j; j--) m &= ~(0x80000000u >> __clz((int)m));   // drop the j highest set bits
                i = w * 32 + (uint32_t)__clz((int)m);
                break;
            }
        }
        const uint32_t o = base_prev + hix;
        if (o < slot_cap) {
            const uint64_t ft = win64(s.sF, s.rel[lo] + i);
            const uint64_t fk = ft >> (64 - 2 * K), rk = revcomp_top<K>(ft);
            const uint64_t h = mm_hash64_gfx950(fk < rk ? fk : rk);      // (round 6, VERDICT r05 #4d: the spelling the loop uses — v_lshl_add_u64, v_bitop3)
            if constexpr (HV == 2) {
                if (h >= thr) {                                          // not a hit after all: out of its record's mask
                    atomicAnd((uint32_t*)&s.mask[kmer_word(i)][lo], ~(1u << kmer_bit(i)));
                    *s.redo = 1u;
                    continue;
                }
            }
            uint64_t rid = rec_base + pass + lo;
            if (f >> 31) {
                rid |= RID_MARKER_BIT;
                if (paired) rid |= min(emission_rank(i, s.nh[lo], avx2_compat), RID_RANK_MAX) << RID_RANK_SHIFT;   // (sketch_session.h)
            }
            slot_rec[out0 + o] = OccRec{h, rid, s.m0[lo], s.m1[lo]};
            if (slot_key) slot_key[out0 + o] = (uint32_t)(h >> key_sh);   // what finish() partitions by (replay_lds.hip)
        }
    }
}

#undef SY_LDS

}  // namespace
}  // namespace sylph
