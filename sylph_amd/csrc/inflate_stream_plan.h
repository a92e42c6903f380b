// inflate_stream_plan.h — the bookkeeping of ONE SLICE of the streamed device inflate (csrc/inflate.hip, sylph_inflate_stream_*),
// host-compilable like inflate_plan.h, which it includes: tests/inflate_stream_plan_capi.cpp builds it with g++ and the CPU suite
// checks it against zlib (tests/test_inflate_stream_plan.py).
//
// sylph_inflate_files handles a file in one piece: all compressed bytes on the device, 32 B of cell scratch per byte.  The stream runs
// the same phases over one slice of the compressed bytes per call and hands what lies between two calls to the next one:
//   * the CARRY of a file: the bit where its chain continues (a block's start inside a member, or the byte of the next member's
//     header), whether that is inside a member, the member's length and raw CRC register so far, whether the first block of the next
//     slice has a window, and whether the file is finished;
//   * THE CUT (slice_cut, slice_walk): a slice uploads the bytes [pos, min(file end, pos + slice_bytes + overlap)), pos = the
//     carry's byte.  The chain is walked from the carry's bit, members, trailers, ISIZE and host-inflated small members as in
//     chain_walk, and ends in front of the first chain block that starts at or behind pos + slice_bytes, or that ran out of input
//     because the SLICE ended there (the decoder's ST_ERR_OVERRUN, a block that ends behind the uploaded bytes, a header cut by their
//     end).  Where the FILE ends there, that is damage, as it is for the whole file.  A slice whose first block does not fit says
//     `grow`: the caller doubles the slice, MAX_GROW times at most;
//   * a member that spans slices has its CRC register continued (crc_continue: crc_shift by the bytes the slice added) and is checked
//     against its trailer in the slice where it ends.
// The last 32 KiB of a file's text is the window in front of its next slice's first block (inflate.hip keeps it).
#pragma once
#include "inflate_plan.h"

namespace sylph {
namespace inflate_stream_plan {

using namespace inflate_plan;

constexpr uint64_t MIN_SLICE = 64ull << 10;          // "inflate_slice_bytes" is at least this
constexpr uint64_t DEFAULT_SLICE = 256ull << 20;        // profiles/inflate_stream.txt
constexpr uint32_t MAX_GROW = 6;                     // a slice is doubled this often at most for a first block that does not fit
constexpr uint64_t HEADER_MAX_BYTES = 600;           // a dynamic block's header is shorter (inflate.hip: GZ_PAD_WORDS)

// the bytes uploaded behind the nominal cut, so that a block that starts in front of it has its end on the device
inline uint64_t slice_overlap(uint64_t slice_bytes) { return std::min<uint64_t>(std::max<uint64_t>(slice_bytes / 2, 32ull << 10), 1ull << 20); }

struct Carry {
    uint64_t bit = 0;            // where the chain continues, in bits of the file
    bool in_member = false;      // bit is a block's start inside a member (else: byte bit / 8 holds the next member's header)
    uint64_t member_len = 0;     // in_member: that member's output so far ...
    uint32_t crc_raw = 0;        // ... and its raw CRC register (started at 0) over it
    bool have_window = false;    // the first block of the next slice may copy from the text in front of it
    bool finished = false;       // the file has no more bytes to give
};

// file bytes of a slice: [pos, end) travel, the chain stops in front of the first block at or behind `cut`
struct SliceCut { uint64_t pos, cut, end; };
inline SliceCut slice_cut(const Carry& c, uint64_t file_bytes, uint64_t slice_bytes) {
    SliceCut s;
    s.pos = std::min<uint64_t>(c.bit / 8, file_bytes);
    s.cut = s.pos + std::min<uint64_t>(slice_bytes, file_bytes - s.pos);
    s.end = s.cut + std::min<uint64_t>(slice_overlap(slice_bytes), file_bytes - s.cut);
    return s;
}

struct SliceMember {
    uint64_t out_begin, out_end;   // its bytes among the slice's new bytes
    uint32_t crc, isize;           // from the trailer (ends)
    bool on_host;
    bool ends;                     // the member's trailer was reached in this slice
    uint64_t len_before;           // bytes and raw CRC register the earlier slices gave it
    uint32_t crc_before;
};
struct SliceWalk {
    std::vector<ChainBlock> blocks;        // member: index into members; out_off: among the slice's new bytes
    std::vector<SliceMember> members;      // in order; they tile [0, total)
    std::vector<HostPiece> host;           // gz_begin / gz_end: bytes of the file
    uint64_t total = 0;                    // new bytes of text
    Carry next;                            // entry state of the next slice (crc_raw of an open member: the caller's, once the CRCs are in)
    bool grow = false;                     // nothing fitted: the same carry again with a larger slice
    std::string why;                       // non-empty: damage (or nothing this road takes): the stream is given up
};

// the register of a member after a slice added `n_new` bytes whose own raw register (started at 0) is `raw_new`
inline uint32_t crc_continue(const uint32_t* x2n, uint32_t raw_before, uint32_t raw_new, uint64_t n_new) { return crc_shift(x2n, raw_before, n_new) ^ raw_new; }

// gz: the file whole, in host memory (headers, trailers and small members are read there).  cand_bits: sorted, unique candidate start
// bits IN THE FILE that the slice's scan found (the carry's bit among them when it is a block's start, and the first member's first
// block whatever its type); res_of[i]: where candidate i's report lies in res; res[..].end_bit + bit_shift = the bit in the file.
// host_inflate(begin, &end, &n_out) as in chain_walk, in bytes of the file.
template <class HostInflate>
SliceWalk slice_walk(const uint8_t* gz, uint64_t file_bytes, const Carry& in, const SliceCut& sc, const std::vector<uint64_t>& cand_bits,
                     const uint32_t* res_of, const BlockResult* res, int64_t bit_shift, HostInflate&& host_inflate) {
    SliceWalk w;
    Carry c = in;
    const bool slice_short = sc.end < file_bytes;              // the slice ended before the file did
    bool progress = false;
    auto cut_here = [&] { if (!progress) w.grow = true; };
    auto close_open_member = [&] {
        if (c.in_member && !w.members.empty() && !w.members.back().ends && !w.members.back().on_host) w.members.back().out_end = w.total;
    };
    if (c.finished) { w.next = c; return w; }
    if (c.in_member) w.members.push_back(SliceMember{0, 0, 0, 0, false, false, c.member_len, c.crc_raw});
    bool first_of_member = false;
    uint64_t header_bit = 0;                                   // first_of_member: where that member's header lies
    while (true) {
        if (!c.in_member) {
            const uint64_t p = c.bit / 8;
            if (p == file_bytes && p) { c.finished = true; break; }
            if (p >= sc.cut && sc.cut < file_bytes) { cut_here(); break; }
            const size_t body = member_body(gz, (size_t)file_bytes, (size_t)p);
            if (!body) { w.why = "no gzip member header at byte " + std::to_string(p); return w; }
            if (body >= sc.cut && sc.cut < file_bytes) { cut_here(); break; }
            const uint64_t bit = (uint64_t)body * 8;
            auto it = std::lower_bound(cand_bits.begin(), cand_bits.end(), bit);
            if (it == cand_bits.end() || *it != bit) {
                if (slice_short && body + HEADER_MAX_BYTES > sc.end) { cut_here(); break; }     // (its header may be cut by the slice's end)
                size_t end = 0;
                uint64_t n_out = 0;
                if (!host_inflate((size_t)p, &end, &n_out)) { w.why = "member at byte " + std::to_string(p) + " does not start with a dynamic block and is not small"; return w; }
                if (n_out) w.host.push_back(HostPiece{(size_t)p, end, w.total, (uint32_t)w.members.size()});
                w.members.push_back(SliceMember{w.total, w.total + n_out, 0, 0, true, true, 0, 0});
                w.total += n_out;
                c.bit = (uint64_t)end * 8;
                progress = true;
            } else {
                header_bit = c.bit;
                c.in_member = true;
                c.bit = bit;
                c.member_len = 0;
                c.crc_raw = 0;
                first_of_member = true;
                w.members.push_back(SliceMember{w.total, w.total, 0, 0, false, false, 0, 0});
                continue;
            }
        } else {
            if (c.bit / 8 >= sc.cut && sc.cut < file_bytes) { cut_here(); break; }
            auto it = std::lower_bound(cand_bits.begin(), cand_bits.end(), c.bit);
            if (it == cand_bits.end() || *it != c.bit) {
                if (slice_short && c.bit / 8 + HEADER_MAX_BYTES > sc.end) { cut_here(); break; }
                w.why = "chain breaks at bit " + std::to_string(c.bit) + " (no candidate starts there)";
                return w;
            }
            const uint32_t ri = res_of[(size_t)(it - cand_bits.begin())];
            const BlockResult& r = res[ri];
            const bool ended = r.status == ST_NEXT_DYNAMIC || r.status == ST_FINAL;
            const uint64_t end_bit = ended ? (uint64_t)((int64_t)r.end_bit + bit_shift) : 0;
            if (slice_short && (r.status == ST_ERR_OVERRUN || (ended && end_bit > sc.end * 8))) { cut_here(); break; }
            if (!ended) { w.why = "block at bit " + std::to_string(c.bit) + ": decoder status " + std::to_string(r.status); return w; }
            if (first_of_member && (r.flags & 1)) { w.why = "block at bit " + std::to_string(c.bit) + " copies from before its member"; return w; }
            first_of_member = false;
            w.blocks.push_back(ChainBlock{ri, (uint32_t)(w.members.size() - 1), w.total, r.n_out, r.flags});
            w.total += r.n_out;
            c.member_len += r.n_out;
            progress = true;
            if (r.status == ST_NEXT_DYNAMIC) {
                if (end_bit <= c.bit) { w.why = "block at bit " + std::to_string(c.bit) + " does not move on"; return w; }
                c.bit = end_bit;
                continue;
            }
            const uint64_t trailer = (end_bit + 7) / 8;
            if (trailer + 8 > file_bytes) { w.why = "member trailer beyond the end of the file"; return w; }
            const uint8_t* t = gz + trailer;
            SliceMember& m = w.members.back();
            m.crc = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
            m.isize = t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
            m.out_end = w.total;
            m.ends = true;
            if ((uint32_t)c.member_len != m.isize) { w.why = "member ending at byte " + std::to_string(trailer) + ": ISIZE differs from the decoded length"; return w; }
            c.in_member = false;
            c.member_len = 0;
            c.crc_raw = 0;
            c.bit = (trailer + 8) * 8;
        }
        // behind a member
        const uint64_t p = c.bit / 8;
        if (p == file_bytes) { c.finished = true; break; }
        if (p > file_bytes) { w.why = "member runs past the end of the file"; return w; }
        if (!member_body(gz, (size_t)file_bytes, (size_t)p)) { w.why = "trailing bytes behind the last member"; return w; }
    }
    if (w.grow) { w.next = in; return w; }
    // cut between a member's header and its first block: the next slice begins with the header (that block has no window)
    if (c.in_member && first_of_member) { c.in_member = false; c.bit = header_bit; w.members.pop_back(); }
    close_open_member();
    c.have_window = c.in_member;
    w.next = c;
    return w;
}

}  // namespace inflate_stream_plan
}  // namespace sylph
