// bunzip2_stream_plan.h — the bookkeeping of ONE SLICE of the streamed device bzip2 decoder (csrc/bunzip2.hip, sylph_bunzip2_stream_*),
// host-compilable like bunzip2_plan.h, which it includes: tests/bunzip2_stream_plan_capi.cpp builds it with g++ and the CPU suite checks
// it against Python's bz2 (tests/test_bunzip2_stream_plan.py).
//
// sylph_bunzip2_files handles a file in one piece: all compressed bytes on the device, the whole text of all files in one buffer.  The
// stream runs the same phases over one slice of the compressed bytes per call.  A bzip2 block never refers to the one before it, so what
// lies between two calls is small:
//   * the CARRY of a file: where its chain stands (bunzip2_plan.h ChainPos: the bit where it continues, whether that is inside a
//     stream, that stream's level and combined CRC so far, the streams and blocks counted so far) and whether the file is finished;
//   * THE CUT (slice_cut, SliceWalk): a slice uploads the bytes [pos, min(file end, pos + slice_bytes + OVERLAP)), pos = the byte of
//     the carry's bit.  The chain is walked from the carry's bit with chain_step, the very link ChainWalk follows: headers,
//     end-of-stream trailers and combined CRCs are read in the host's copy of the file, which is whole, so a cut between a stream
//     header and its first block, or in front of an end-of-stream magic, resumes at that byte or bit, and an empty stream or a stream
//     boundary on a slice end needs nothing special.  The slice ends in front of the first chain block that starts at or behind
//     pos + slice_bytes — the decoder's ST_ERR_OVERRUN of such a block, or an end behind the uploaded bytes, says that the SLICE ended
//     there and is nobody's damage: the next slice begins with that block.
//   * OVERLAP is 1 MiB: libbz2's encoder writes at most 1.01 n + 600 bytes for the n <= 900 000 bytes of a block, 909 600, so every
//     block it can write that starts in front of the nominal cut has its end on the device.  A chain block that starts in front of the
//     cut and still runs out of the uploaded bytes is declined (SYLPH_ERR_FORMAT): NO ENCODER IN USE WRITES SUCH A BLOCK (it would
//     have to code 900 000 bytes in more than a MiB), and the host's libbz2 takes the file.  Where the FILE ends in the slice, the
//     same report is the damage it is for the whole file.
// Trailing bytes that are no further stream are damage in the slice that reaches them.
#pragma once
#include <algorithm>

#include "bunzip2_plan.h"

namespace sylph {
namespace bunzip2_stream_plan {

using namespace bunzip2_plan;

constexpr uint64_t MIN_SLICE = 64ull << 10;          // "bunzip2_slice_bytes" is at least this
constexpr uint64_t DEFAULT_SLICE = 256ull << 20;     // profiles/bunzip2_stream.txt
constexpr uint64_t OVERLAP = 1ull << 20;             // bytes uploaded behind the nominal cut (see above)

struct Carry {
    ChainPos pos;                // bit, in_stream, level, combined, n_streams, n_blocks: bits and counts of the FILE
    bool finished = false;       // the file has no more bytes to give
};

// file bytes of a slice: [pos, end) travel, the chain stops in front of the first block at or behind `cut`
struct SliceCut { uint64_t pos, cut, end; };
inline SliceCut slice_cut(const Carry& c, uint64_t file_bytes, uint64_t slice_bytes) {
    SliceCut s;
    slice_bytes = std::max(slice_bytes, MIN_SLICE);
    s.pos = std::min<uint64_t>(c.pos.bit / 8, file_bytes);
    s.cut = s.pos + std::min<uint64_t>(slice_bytes, file_bytes - s.pos);
    s.end = s.cut + std::min<uint64_t>(OVERLAP, file_bytes - s.cut);
    return s;
}

// One file's chain over one slice, from its carry: step() as ChainWalk::step, as the reports of the SLICE's candidates come in.
// cand: sorted, unique candidate bits OF THE FILE that the slice's scan found (only those whose 48 bits lie in [pos, end));
// rep[i].end_bit + bit_shift = the bit in the file.  ChainBlock::cand indexes `cand`; ::stream counts the file's streams.
struct SliceWalk {
    const uint8_t* d = nullptr;                    // the file whole, in host memory
    uint64_t fn = 0;
    uint32_t file = 0;
    SliceCut sc{};
    const std::vector<uint64_t>* cand = nullptr;
    int64_t bit_shift = 0;
    std::vector<ChainBlock> blocks;                // this slice's chain blocks, in order
    std::string why;                               // non-empty: damage (or a block no encoder writes): the stream is given up
    bool ended = false;                            // the slice's chain is walked: `next` is the next slice's entry state
    Carry next;
    size_t next_cand = 0;

    void start(const uint8_t* d_, uint64_t fn_, uint32_t file_, const Carry& in, const SliceCut& sc_, const std::vector<uint64_t>* cand_, int64_t shift) {
        d = d_; fn = fn_; file = file_; sc = sc_; cand = cand_; bit_shift = shift;
        next = in;
        ended = in.finished;
    }
    bool slice_short() const { return sc.end < fn; }                           // the slice ended before the file did
    // reports of candidates [0, have) of `cand` are known.  false: it stopped for a report it has not got.
    bool step(const BlockReport* rep, size_t have) {
        ChainPos& p = next.pos;
        while (!ended && why.empty()) {
            if (!p.in_stream && p.bit == fn * 8 && p.n_streams) { next.finished = true; ended = true; break; }
            // (a header or a trailer at or behind the cut is walked all the same: the host reads them, and the next slice begins further on)
            bool need = false;
            BlockAt got;
            const Link l = chain_step(d, fn, file, p, [&](uint64_t lb, std::string& w) {
                BlockAt at;
                if (lb / 8 >= sc.cut && sc.cut < fn) return at;                // the cut: the next slice begins with this block
                while (next_cand < cand->size() && (*cand)[next_cand] < lb) next_cand++;
                if (next_cand >= cand->size() || (*cand)[next_cand] != lb) { w = "block magic at bit " + std::to_string(lb) + " is no candidate"; return at; }
                if (next_cand >= have) { need = true; return at; }
                const BlockReport& r = rep[next_cand];
                const uint64_t end_bit = (uint64_t)((int64_t)r.end_bit + bit_shift);
                if (slice_short() && (r.status == ST_ERR_OVERRUN || (r.status == ST_OK && end_bit > sc.end * 8))) {
                    w = "block at bit " + std::to_string(lb) + " starts in front of the slice's cut and runs past its overlap (no libbz2 encoder writes such a block)";
                    return at;
                }
                at.what = BlockAt::HAVE;
                at.cand = next_cand;
                at.r = &r;
                at.end_bit = end_bit;
                return at;
            }, why, &got);
            if (l == Link::DECLINED) break;
            if (l == Link::HOLD) { if (need) return false; ended = true; break; }
            if (l == Link::BLOCK) blocks.push_back(ChainBlock{(uint32_t)got.cand, file, (uint32_t)(p.n_streams - 1), got.r->n});
        }
        return true;
    }
};

}  // namespace bunzip2_stream_plan
}  // namespace sylph
