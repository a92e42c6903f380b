// C wrapper around sylph_amd/csrc/bunzip2_stream_plan.h for tests/test_bunzip2_stream_plan.py (g++, no HIP): the very header
// bunzip2.hip includes — the carry, the cut, the sliced chain walk — driven by the CPU MODEL of the kernels' reports that
// bunzip2_plan_capi.cpp holds (included here, not copied): every bit position of a slice's uploaded bytes tested for the block magic,
// as scan_kernel does within a slice's limits; each candidate decoded up to its end-of-block symbol or to the end of the slice's bytes
// (ST_ERR_OVERRUN there), as decode_kernel does.  A "stream" here is the host half of sylph_bunzip2_stream_*: carries, one slice per
// advancing file per call, reports in batches.  It returns the chain blocks' bit ranges and stored CRCs; the test decodes each with
// Python's bz2.  Test infrastructure: the product never runs this.
#include "bunzip2_plan_capi.cpp"

#include "../sylph_amd/csrc/bunzip2_stream_plan.h"

using namespace sylph::bunzip2_stream_plan;

namespace {

struct ModelStream {
    std::vector<const uint8_t*> d;
    std::vector<uint64_t> n;
    std::vector<Carry> carry;
    uint64_t slice_bytes = 0, overlap = OVERLAP;
    uint32_t batch = 1000;
    uint64_t n_slices = 0, peak_upload = 0, rnd = 0x9E3779B97F4A7C15ull;
};

// candidate bits (of the file) whose 48 bits lie in the bytes [pos, end)
std::vector<uint64_t> scan_slice(const uint8_t* d, uint64_t pos, uint64_t end) {
    std::vector<uint64_t> out;
    uint64_t win = 0;
    for (uint64_t bit = pos * 8; bit < end * 8; bit++) {
        win = ((win << 1) | ((d[bit >> 3] >> (7 - (bit & 7))) & 1u)) & 0xFFFFFFFFFFFFull;
        if (bit + 1 >= pos * 8 + 48 && win == BLOCK_MAGIC) out.push_back(bit + 1 - 48);
    }
    return out;
}

}  // namespace

extern "C" {

void bsp_cut(uint64_t carry_bit, uint64_t file_bytes, uint64_t slice_bytes, uint64_t* out3) {
    Carry c;
    c.pos.bit = carry_bit;
    const SliceCut s = slice_cut(c, file_bytes, slice_bytes);
    out3[0] = s.pos; out3[1] = s.cut; out3[2] = s.end;
}

uint64_t bsp_overlap() { return OVERLAP; }
uint64_t bsp_min_slice() { return MIN_SLICE; }

// overlap 0: the plan's own
void* bsp_open(const uint8_t* const* files, const uint64_t* sizes, uint32_t n_files, uint64_t slice_bytes, uint64_t overlap, uint32_t batch) {
    ModelStream* m = new ModelStream();
    for (uint32_t i = 0; i < n_files; i++) { m->d.push_back(files[i]); m->n.push_back(sizes[i]); }
    m->carry.assign(n_files, Carry{});
    m->slice_bytes = slice_bytes;
    if (overlap) m->overlap = overlap;
    m->batch = batch ? batch : 1;
    return m;
}
void bsp_close(void* h) { delete (ModelStream*)h; }

// One step: every file with advance[i] != 0 (NULL: all) goes one slice further.  extra: injected false candidates, (file, bit of the
// file) pairs, reported as decoded blocks that end at a random bit.  Per chain block of this step, in file order: blk[4 k + 0..3] =
// file, start bit, end bit, stored CRC (cap blocks).  state[6 f + 0..5] = carry bit, in_stream, level, combined, streams, blocks of file
// f behind the step; finished[f].  info: slices walked so far, largest upload (bytes), candidates decoded in this step.
int bsp_next(void* h, const uint8_t* advance, const uint64_t* extra, uint32_t n_extra, uint64_t* blk, uint32_t cap, uint32_t* n_blk, uint64_t* state,
             uint8_t* finished, uint64_t* info, char* err, size_t err_cap) {
    ModelStream& m = *(ModelStream*)h;
    const uint32_t F = (uint32_t)m.d.size();
    *n_blk = 0;
    uint64_t upload = 0, decoded = 0;
    std::vector<Carry> next = m.carry;
    for (uint32_t f = 0; f < F; f++) {
        if ((advance && !advance[f]) || m.carry[f].finished) continue;
        SliceCut sc = slice_cut(m.carry[f], m.n[f], m.slice_bytes);
        sc.end = sc.cut + std::min<uint64_t>(m.overlap, m.n[f] - sc.cut);
        upload += sc.end - sc.pos;
        std::vector<uint64_t> cand = scan_slice(m.d[f], sc.pos, sc.end);
        std::vector<uint64_t> fake;
        for (uint32_t i = 0; i < n_extra; i++)
            if (extra[2 * i] == f && extra[2 * i + 1] >= sc.pos * 8 && extra[2 * i + 1] + 48 <= sc.end * 8 &&
                !std::binary_search(cand.begin(), cand.end(), extra[2 * i + 1]))
                fake.push_back(extra[2 * i + 1]);
        cand.insert(cand.end(), fake.begin(), fake.end());
        std::sort(cand.begin(), cand.end());
        cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
        std::vector<BlockReport> rep(cand.size());
        SliceWalk w;
        w.start(m.d[f], m.n[f], f, m.carry[f], sc, &cand, (int64_t)(sc.pos * 8));
        size_t have = 0;
        for (;;) {
            const bool fin = w.step(rep.data(), have);
            if (!w.why.empty()) { snprintf(err, err_cap, "%s", w.why.c_str()); return -1; }
            if (fin) break;
            const size_t cnt = std::min<size_t>(m.batch, cand.size() - have);
            if (!cnt) { snprintf(err, err_cap, "the chain needs a candidate that is not there"); return -1; }
            for (size_t i = have; i < have + cnt; i++) {
                if (std::find(fake.begin(), fake.end(), cand[i]) != fake.end()) {
                    m.rnd = m.rnd * 6364136223846793005ull + 1442695040888963407ull;
                    rep[i] = BlockReport{};
                    rep[i].n = 1000;
                    rep[i].end_bit = cand[i] - sc.pos * 8 + 100 + (m.rnd >> 40) % 5000;
                } else {
                    rep[i] = model_block(m.d[f] + sc.pos, sc.end - sc.pos, cand[i] - sc.pos * 8);      // (the slice's bytes are all it sees)
                }
            }
            have += cnt;
        }
        decoded += have;
        for (const ChainBlock& cb : w.blocks) {
            if (*n_blk < cap) {
                uint64_t* o = blk + 4 * (size_t)*n_blk;
                o[0] = f;
                o[1] = cand[cb.cand];
                o[2] = rep[cb.cand].end_bit + sc.pos * 8;
                o[3] = rep[cb.cand].crc;
            }
            (*n_blk)++;
        }
        next[f] = w.next;
        m.n_slices++;
    }
    m.carry = next;
    m.peak_upload = std::max(m.peak_upload, upload);
    for (uint32_t f = 0; f < F; f++) {
        const ChainPos& p = m.carry[f].pos;
        uint64_t* s = state + 6 * (size_t)f;
        s[0] = p.bit; s[1] = p.in_stream; s[2] = (uint64_t)p.level; s[3] = p.combined; s[4] = p.n_streams; s[5] = p.n_blocks;
        finished[f] = m.carry[f].finished;
    }
    info[0] = m.n_slices; info[1] = m.peak_upload; info[2] = decoded;
    return 0;
}

}  // extern "C"
