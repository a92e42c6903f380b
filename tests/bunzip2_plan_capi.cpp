// C wrapper around sylph_amd/csrc/bunzip2_plan.h for tests/test_bunzip2_host.py (g++, no HIP): the very header bunzip2.hip includes
// — CRC-32/BZIP2 put together from shifted pieces, the run-length scan, the chain walk — driven by a plain CPU MODEL of what the
// device kernels report (every bit position tested for the block magic as scan_kernel does; each candidate's header and symbols
// decoded up to its end-of-block symbol with libbz2's table arithmetic, as decode_kernel does).  Test infrastructure: the product never
// runs this.
#include <algorithm>
#include <cstring>

#include "../sylph_amd/csrc/bunzip2_plan.h"

using namespace sylph::bunzip2_plan;

namespace {

struct BitReader {
    const uint8_t* d;
    uint64_t n_bits, pos;
    bool over = false;
    uint32_t get(unsigned k) {
        uint32_t v = 0;
        for (unsigned i = 0; i < k; i++) {
            if (pos >= n_bits) { over = true; return 0; }
            v = (v << 1) | ((d[pos >> 3] >> (7 - (pos & 7))) & 1u);
            pos++;
        }
        return v;
    }
};

// the model of decode_kernel's report (without the bytes: the chain needs where a block ends, its size and its stored CRC)
BlockReport model_block(const uint8_t* d, uint64_t n_bytes, uint64_t bit) {
    BlockReport r{};
    BitReader b{d, n_bytes * 8, bit};
    auto fail = [&](uint32_t st) { r.status = st; r.end_bit = b.pos; return r; };
    const uint64_t m = ((uint64_t)b.get(24) << 24) | b.get(24);
    if (m != BLOCK_MAGIC) return fail(ST_ERR_MAGIC);
    r.crc = b.get(32);
    r.randomised = b.get(1);
    r.orig_ptr = b.get(24);
    const uint32_t used16 = b.get(16);
    uint32_t n_in_use = 0;
    for (int i = 0; i < 16; i++)
        if ((used16 >> (15 - i)) & 1) n_in_use += __builtin_popcount(b.get(16));
    if (!n_in_use) return fail(ST_ERR_HEADER);
    const uint32_t alpha = n_in_use + 2;
    const uint32_t n_groups = b.get(3), n_sel = b.get(15);
    if (n_groups < 2 || n_groups > 6 || n_sel < 1) return fail(ST_ERR_HEADER);
    if (n_sel > MAX_SELECTORS) return fail(ST_ERR_SELECTORS);
    std::vector<uint8_t> sel(n_sel);
    uint8_t pos[6] = {0, 1, 2, 3, 4, 5};
    for (uint32_t i = 0; i < n_sel; i++) {
        uint32_t j = 0;
        while (b.get(1)) { if (++j >= n_groups) return fail(ST_ERR_HEADER); }
        const uint8_t v = pos[j];
        for (; j > 0; j--) pos[j] = pos[j - 1];
        pos[0] = v;
        sel[i] = v;
        if (b.over) return fail(ST_ERR_OVERRUN);
    }
    int32_t limit[6][24], base[6][24], perm[6][258], minlen[6];
    for (uint32_t t = 0; t < n_groups; t++) {
        uint8_t len[258];
        int32_t curr = (int32_t)b.get(5);
        for (uint32_t i = 0; i < alpha; i++) {
            for (;;) {
                if (curr < 1 || curr > 20) return fail(ST_ERR_HEADER);
                if (!b.get(1)) break;
                curr += b.get(1) ? -1 : 1;
            }
            len[i] = (uint8_t)curr;
        }
        int32_t mn = 32, mx = 0;
        for (uint32_t i = 0; i < alpha; i++) { mn = std::min<int32_t>(mn, len[i]); mx = std::max<int32_t>(mx, len[i]); }
        int32_t pp = 0;
        memset(perm[t], 0, sizeof(perm[t]));
        for (int32_t l = mn; l <= mx; l++)
            for (uint32_t j = 0; j < alpha; j++)
                if (len[j] == l) perm[t][pp++] = (int32_t)j;
        for (int i = 0; i < 24; i++) base[t][i] = limit[t][i] = 0;
        for (uint32_t i = 0; i < alpha; i++) base[t][len[i] + 1]++;
        for (int i = 1; i < 23; i++) base[t][i] += base[t][i - 1];
        int32_t vec = 0;
        for (int32_t l = mn; l <= mx; l++) { vec += base[t][l + 1] - base[t][l]; limit[t][l] = vec - 1; vec <<= 1; }
        for (int32_t l = mn + 1; l <= mx; l++) base[t][l] = ((limit[t][l - 1] + 1) << 1) - base[t][l];
        minlen[t] = mn;
    }
    const uint32_t eob = n_in_use + 1;
    uint32_t group_no = 0, group_pos = 0, g = 0, nb = 0, es = 0, nrun = 1;
    bool first = true;
    for (;;) {
        if (group_pos == 0) {
            if (!first) group_no++;
            first = false;
            if (group_no >= n_sel) return fail(ST_ERR_CODE);
            group_pos = 50;
            g = sel[group_no];
        }
        group_pos--;
        int32_t zn = minlen[g];
        int32_t zvec = (int32_t)b.get((unsigned)zn);
        for (;;) {
            if (zn > 20) return fail(ST_ERR_CODE);
            if (zvec <= limit[g][zn]) break;
            zn++;
            zvec = (zvec << 1) | (int32_t)b.get(1);
        }
        if (b.over) return fail(ST_ERR_OVERRUN);
        const int32_t idx = zvec - base[g][zn];
        if (idx < 0 || idx >= 258) return fail(ST_ERR_CODE);
        const uint32_t sym = (uint32_t)perm[g][idx];
        r.symbols++;
        if (sym <= 1) {
            if (nrun >= 2u * 1024 * 1024) return fail(ST_ERR_SIZE);
            es += (sym + 1) * nrun;
            nrun <<= 1;
            continue;
        }
        if (es) {
            if (nb + es > MAX_BLOCK) return fail(ST_ERR_SIZE);
            nb += es;
            es = 0;
            nrun = 1;
        }
        if (sym == eob) break;
        if (nb >= MAX_BLOCK) return fail(ST_ERR_SIZE);
        nb++;
    }
    r.n = nb;
    r.end_bit = b.pos;
    if (r.orig_ptr >= nb) r.status = ST_ERR_ORIG;
    return r;
}

}  // namespace

extern "C" {

uint32_t bp_crc_raw(const uint8_t* p, uint64_t n, uint32_t reg) {
    uint32_t t[256];
    crc_byte_table(t);
    return crc_raw(t, reg, p, n);
}

// CRC-32/BZIP2 of p[0, n) from pieces of `piece` bytes, each started at 0 and shifted to its place, as crc_kernel does
uint32_t bp_crc_pieces(const uint8_t* p, uint64_t n, uint64_t piece) {
    uint32_t t[256], x2n[64];
    crc_byte_table(t);
    crc_x2n_table(x2n);
    uint32_t raw = 0;
    for (uint64_t a = 0; a < n; a += piece) {
        const uint64_t e = std::min(n, a + piece);
        raw ^= crc_shift(x2n, crc_raw(t, 0, p + a, e - a), n - e);
    }
    return crc_finish(x2n, raw, n);
}

uint32_t bp_combine(const uint32_t* crcs, uint32_t n) {
    uint32_t c = 0;
    for (uint32_t i = 0; i < n; i++) c = combine_stream(c, crcs[i]);
    return c;
}

// RLE1 text p[0, n) decoded straight through, and through chunk functions composed as rlescan_kernel does, then expanded chunk by chunk;
// returns the decoded length, or -1 when the two differ, -2 when a repeat count is due at the end (declined)
long long bp_rle_check(const uint8_t* p, uint32_t n, uint32_t chunk, uint8_t* out, uint64_t cap) {
    std::vector<uint8_t> a(cap), b(cap);
    // straight through from state 0 (cap must hold the text)
    uint32_t k = 0, len_a = 0;
    {
        std::vector<uint8_t> tmp(cap);
        len_a = n ? rle_expand(p, n, 0, 0, tmp.data()) : 0;
        memcpy(a.data(), tmp.data(), len_a);
    }
    const uint32_t nc = (n + chunk - 1) / chunk;
    uint64_t off = 0;
    for (uint32_t c = 0; c < nc; c++) {
        const uint32_t s = c * chunk, m = std::min(chunk, n - s);
        const RleFn f = rle_fn(p + s, m);
        const uint32_t w = rle_expand(p + s, m, k, s ? p[s - 1] : 0, b.data() + off);
        if (w != f.len[k]) return -1;
        off += w;
        const uint32_t ko = f.kout(k);
        k = c + 1 < nc ? rle_eff(ko, p[s + m - 1], p[s + m]) : ko;
    }
    if (k == 4) return -2;
    if (off != len_a || memcmp(a.data(), b.data(), len_a) != 0) return -1;
    memcpy(out, a.data(), len_a);
    return (long long)len_a;
}

// The chain over one or more files (back to back, as bunzip2.hip lays them out): candidates from a CPU scan for the block magic plus
// `n_extra` injected false ones (reported as decoded blocks that end at a random bit), reports from model_block, walked in batches
// of `batch` candidates.  info: streams, blocks, candidates decoded.  crcs/ns: the chain blocks' stored CRCs and sizes (cap entries).
int bp_model_chain(const uint8_t* const* files, const uint64_t* sizes, uint32_t n_files, const uint64_t* extra, uint32_t n_extra,
                   uint32_t batch, uint64_t* info, uint32_t* crcs, uint32_t* ns, uint32_t* files_of, uint32_t cap, char* err, size_t err_cap) {
    Segments S;
    S.base.push_back(0);
    for (uint32_t i = 0; i < n_files; i++) { S.ptr.push_back(files[i]); S.base.push_back(S.base.back() + sizes[i]); }
    std::vector<uint64_t> cand;
    for (uint32_t f = 0; f < n_files; f++)
        for (uint64_t bit = 0; bit + 48 <= sizes[f] * 8; bit++)
            if (bits_at(files[f], sizes[f], bit, 48) == BLOCK_MAGIC) cand.push_back(S.base[f] * 8 + bit);
    std::vector<bool> fake;
    for (uint32_t i = 0; i < n_extra; i++) cand.push_back(extra[i]);
    std::sort(cand.begin(), cand.end());
    cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
    std::vector<BlockReport> rep(cand.size());
    ChainWalk walk;
    walk.start(&S, &cand);
    size_t have = 0;
    uint64_t rnd = 0x9E3779B97F4A7C15ull;
    for (;;) {
        const bool fin = walk.step(rep.data(), have);
        if (!walk.why.empty()) { snprintf(err, err_cap, "%s", walk.why.c_str()); return -1; }
        if (fin) break;
        const size_t cnt = std::min<size_t>(batch, cand.size() - have);
        if (!cnt) { snprintf(err, err_cap, "the chain needs a candidate that is not there"); return -1; }
        for (size_t i = have; i < have + cnt; i++) {
            const bool injected = std::find(extra, extra + n_extra, cand[i]) != extra + n_extra;
            uint32_t f = 0;
            while (f + 1 < n_files && S.base[f + 1] * 8 <= cand[i]) f++;
            if (injected) {
                rnd = rnd * 6364136223846793005ull + 1442695040888963407ull;
                rep[i] = BlockReport{};
                rep[i].n = 1000;
                rep[i].end_bit = cand[i] + 100 + (rnd >> 40) % 5000;
            } else {
                rep[i] = model_block(S.ptr[f], sizes[f], cand[i] - S.base[f] * 8);
                rep[i].end_bit += S.base[f] * 8;
            }
        }
        have += cnt;
    }
    info[0] = walk.n_streams;
    info[1] = walk.blocks.size();
    info[2] = have;
    for (size_t i = 0; i < walk.blocks.size() && i < cap; i++) {
        crcs[i] = rep[walk.blocks[i].cand].crc;
        ns[i] = walk.blocks[i].n;
        files_of[i] = walk.blocks[i].file;
    }
    return 0;
}

}  // extern "C"
