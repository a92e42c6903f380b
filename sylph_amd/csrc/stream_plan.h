// stream_plan.h — what the two device decompressors' plan headers (inflate_plan.h, bunzip2_plan.h) share, host-compilable: CRC-32 as
// polynomial arithmetic in either bit order, and the files of one call as one run of bytes.  tests/test_stream_plan.py checks it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define SYLPH_HD __host__ __device__
#else
#define SYLPH_HD
#endif

namespace sylph {
namespace stream_plan {

// ---- CRC-32 as polynomial arithmetic over GF(2) ---------------------------------------------------------------------------------
// Reflected (gzip; zlib's convention in crc32.c: multmodp / x2nmodp): polynomial 0xEDB88320, bit 31 of a word is the coefficient of x^0.
// Not reflected (bzip2, MSB first): polynomial 0x04C11DB7, bit 31 is the coefficient of x^31; the implicit x^32 is left out.
// A CRC is linear over GF(2): the CRC of a text is put together from the registers of pieces computed anywhere, each started at 0
// and shifted (shift) by the bytes behind the piece.
template <bool Reflected>
struct Crc32 {
    static constexpr uint32_t POLY = Reflected ? 0xEDB88320u : 0x04C11DB7u;
    static constexpr uint32_t X0 = Reflected ? 1u << 31 : 1u, X1 = Reflected ? 1u << 30 : 2u;

    // a * b mod P
    SYLPH_HD static inline uint32_t multmodp(uint32_t a, uint32_t b) {
        if constexpr (Reflected) {
            uint32_t m = 1u << 31, p = 0;
            for (;;) {
                if (a & m) {
                    p ^= b;
                    if ((a & (m - 1)) == 0) break;
                }
                m >>= 1;
                b = (b & 1) ? (b >> 1) ^ POLY : b >> 1;
            }
            return p;
        } else {
            uint32_t p = 0;
            for (int i = 31; i >= 0; i--) {
                p = (p & 0x80000000u) ? (p << 1) ^ POLY : p << 1;
                if ((a >> i) & 1) p ^= b;
            }
            return p;
        }
    }
    // x2n[k] = x^(2^k) mod P, k = 0 .. 63
    static inline void x2n_table(uint32_t t[64]) {
        uint32_t p = X1;
        t[0] = p;
        for (int k = 1; k < 64; k++) t[k] = p = multmodp(p, p);
    }
    // x^(8 n) mod P
    SYLPH_HD static inline uint32_t x8n(const uint32_t* x2n, unsigned long long n_bytes) {
        uint32_t p = X0;
        unsigned k = 3;
        while (n_bytes) {
            if (n_bytes & 1) p = multmodp(x2n[k & 63], p);
            n_bytes >>= 1;
            k++;
        }
        return p;
    }
    // the register of the CRC loop (no initial or final inversion) after n more zero bytes
    SYLPH_HD static inline uint32_t shift(const uint32_t* x2n, uint32_t reg, unsigned long long n_bytes) {
        return n_bytes ? multmodp(x8n(x2n, n_bytes), reg) : reg;
    }
    // the CRC of n bytes from `raw` = XOR over their pieces of shift(register of the piece started at 0, bytes behind the piece):
    // the initial 0xFFFFFFFF travels through all n bytes, the final inversion is on top
    static inline uint32_t finish(const uint32_t* x2n, uint32_t raw, unsigned long long n_bytes) {
        return ~(raw ^ shift(x2n, 0xFFFFFFFFu, n_bytes));
    }
    // byte-at-a-time table and the raw register update
    static inline void byte_table(uint32_t t[256]) {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = Reflected ? i : i << 24;
            for (int k = 0; k < 8; k++) {
                if constexpr (Reflected) c = (c & 1) ? (c >> 1) ^ POLY : c >> 1;
                else c = (c & 0x80000000u) ? (c << 1) ^ POLY : c << 1;
            }
            t[i] = c;
        }
    }
    SYLPH_HD static inline uint32_t raw(const uint32_t* t, uint32_t reg, const uint8_t* p, size_t n) {
        for (size_t i = 0; i < n; i++) {
            if constexpr (Reflected) reg = t[(reg ^ p[i]) & 0xFF] ^ (reg >> 8);
            else reg = (reg << 8) ^ t[(reg >> 24) ^ p[i]];
        }
        return reg;
    }
};

// ---- the files of one call ------------------------------------------------------------------------------------------------------
// Each file has its own bytes on the host; on the device they lie back to back, and every offset below counts in that run.
struct Segments {
    std::vector<const uint8_t*> ptr;
    std::vector<uint64_t> base;                   // base[i] = offset of file i; base.back() = the total length
    uint64_t total() const { return base.back(); }
    // the file that holds byte `pos` (the last one for pos >= total(); an empty file holds nothing)
    size_t find(uint64_t pos) const { return (size_t)(std::upper_bound(base.begin(), base.end() - 1, pos) - base.begin()) - 1; }
};
inline Segments one_segment(const uint8_t* d, uint64_t n) { return Segments{{d}, {0, n}}; }

}  // namespace stream_plan
}  // namespace sylph
