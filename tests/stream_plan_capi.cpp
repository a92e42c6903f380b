// C wrapper around sylph_amd/csrc/stream_plan.h for tests/test_stream_plan.py (g++, no HIP): the very header inflate_plan.h and
// bunzip2_plan.h take their CRC-32 arithmetic and their Segments from.  Test infrastructure: the product never runs this.
#include "../sylph_amd/csrc/stream_plan.h"

using namespace sylph::stream_plan;

namespace {

// the CRC of p[0, n) put together from pieces of `piece` bytes, each started at 0 and shifted to its place, as the crc kernels do
template <bool R>
uint32_t crc_pieces(const uint8_t* p, uint64_t n, uint64_t piece) {
    uint32_t t[256], x2n[64];
    Crc32<R>::byte_table(t);
    Crc32<R>::x2n_table(x2n);
    uint32_t raw = 0;
    for (uint64_t a = 0; a < n; a += piece) {
        const uint64_t e = std::min(n, a + piece);
        raw ^= Crc32<R>::shift(x2n, Crc32<R>::raw(t, 0, p + a, (size_t)(e - a)), n - e);
    }
    return Crc32<R>::finish(x2n, raw, n);
}
template <bool R>
uint32_t crc_shift(uint32_t reg, uint64_t n_bytes) {
    uint32_t x2n[64];
    Crc32<R>::x2n_table(x2n);
    return Crc32<R>::shift(x2n, reg, n_bytes);
}

}  // namespace

extern "C" {

uint32_t sp_crc_pieces(int reflected, const uint8_t* p, uint64_t n, uint64_t piece) { return reflected ? crc_pieces<true>(p, n, piece) : crc_pieces<false>(p, n, piece); }
uint32_t sp_crc_shift(int reflected, uint32_t reg, uint64_t n_bytes) { return reflected ? crc_shift<true>(reg, n_bytes) : crc_shift<false>(reg, n_bytes); }

// files of sizes[0 .. n_files) back to back: the file that holds byte pos; *total = their length
uint64_t sp_segments_find(const uint64_t* sizes, uint32_t n_files, uint64_t pos, uint64_t* total) {
    Segments S;
    S.base.push_back(0);
    for (uint32_t i = 0; i < n_files; i++) { S.ptr.push_back(nullptr); S.base.push_back(S.base.back() + sizes[i]); }
    *total = S.total();
    return S.find(pos);
}
uint64_t sp_one_segment_total(const uint8_t* d, uint64_t n) {
    const Segments S = one_segment(d, n);
    return S.ptr.size() == 1 && S.ptr[0] == d && S.find(n ? n - 1 : 0) == 0 ? S.total() : ~0ull;
}

}  // extern "C"
