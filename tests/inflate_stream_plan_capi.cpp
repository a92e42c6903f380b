// C wrapper around sylph_amd/csrc/inflate_stream_plan.h for tests/test_inflate_stream_plan.py (g++ -lz, no HIP): the header
// inflate.hip's stream includes — the cut, the carry, the resumable chain walk, the CRC continued across slices — driven by the CPU
// MODEL of the device kernels of tests/inflate_plan_capi.cpp (included here, not copied), one slice at a time the way
// sylph_inflate_stream_next runs: scan and decode see the slice's bytes only, the window in front of a slice's first block is the last
// 32 KiB of the text so far.  Test infrastructure: the product never runs this.
#include "inflate_plan_capi.cpp"

#include "../sylph_amd/csrc/inflate_stream_plan.h"

using namespace sylph::inflate_stream_plan;

namespace {

// the whole file's chain by the whole-file model: block start bits and (as bits) the bytes behind every member's trailer
bool whole_chain(const uint8_t* gz, uint64_t n, std::vector<uint64_t>& block_bits, std::vector<uint64_t>& member_ends) {
    size_t p = 0;
    while (p < n) {
        const size_t body = member_body(gz, (size_t)n, p);
        if (!body) return false;
        uint64_t bit = (uint64_t)body * 8;
        if (!header_like(gz, (size_t)n, bit) && p != 0) {            // a small member: zlib
            z_stream zs;
            memset(&zs, 0, sizeof(zs));
            if (inflateInit2(&zs, 16 + MAX_WBITS) != Z_OK) return false;
            std::vector<uint8_t> o(1u << 20);
            zs.next_in = const_cast<Bytef*>(gz + p);
            zs.avail_in = (uInt)std::min<uint64_t>(n - p, 1u << 18);
            zs.next_out = o.data();
            zs.avail_out = (uInt)o.size();
            const bool ok = inflate(&zs, Z_FINISH) == Z_STREAM_END;
            const size_t used = zs.total_in;
            inflateEnd(&zs);
            if (!ok) return false;
            p += used;
            member_ends.push_back((uint64_t)p * 8);
            continue;
        }
        while (true) {
            std::vector<uint16_t> cells;
            const BlockResult r = model_decode(gz, (size_t)n, bit, true, ~(size_t)0, cells);
            block_bits.push_back(bit);
            if (r.status == ST_NEXT_DYNAMIC) { bit = r.end_bit; continue; }
            if (r.status != ST_FINAL) return false;
            p = (size_t)((r.end_bit + 7) / 8) + 8;
            break;
        }
        member_ends.push_back((uint64_t)p * 8);
    }
    return p == n;
}

}  // namespace

extern "C" {

// out: pos, cut, end
void isp_slice_cut(uint64_t bit, uint64_t file_bytes, uint64_t slice_bytes, uint64_t* out) {
    Carry c;
    c.bit = bit;
    const SliceCut s = slice_cut(c, file_bytes, slice_bytes);
    out[0] = s.pos; out[1] = s.cut; out[2] = s.end;
}
uint64_t isp_overlap(uint64_t slice_bytes) { return slice_overlap(slice_bytes); }
uint32_t isp_max_grow() { return MAX_GROW; }

// -> number of chain blocks (their start bits in block_bits) and members (the bits behind their trailers in member_ends), or -1
long long isp_whole_chain(const uint8_t* gz, uint64_t n, uint64_t* block_bits, uint64_t* member_ends, uint32_t cap, uint32_t* n_members) {
    std::vector<uint64_t> b, m;
    if (!whole_chain(gz, n, b, m) || b.size() > cap || m.size() > cap) return -1;
    std::copy(b.begin(), b.end(), block_bits);
    std::copy(m.begin(), m.end(), member_ends);
    *n_members = (uint32_t)m.size();
    return (long long)b.size();
}

// The sliced road on the CPU over one file.  -> bytes written to out, or -1 with the reason in err; *good = the bytes the slices
// before the failing one gave (they are in out).  trace: TRACE words per slice (see below), at most trace_cap slices; blocks: the start
// bits of the chain blocks in the order they were decoded into the text.
enum { TRACE = 12 };
long long isp_model_stream(const uint8_t* gz, uint64_t n, uint64_t slice_bytes, uint32_t ratio, uint32_t slack, uint8_t* out, uint64_t out_cap,
                           uint64_t* trace, uint32_t trace_cap, uint32_t* n_slices_out, uint64_t* blocks_out, uint32_t blocks_cap, uint32_t* n_blocks_out,
                           uint64_t* good, char* err, size_t errn) {
    uint32_t x2n[64], tab[256];
    crc_x2n_table(x2n);
    crc_byte_table(tab);
    Carry carry;
    uint64_t total = 0;
    uint32_t n_slices = 0, n_blocks = 0;
    *good = 0;
    *n_slices_out = 0;
    *n_blocks_out = 0;
    if (!member_body(gz, (size_t)n, 0)) { put_err("not a gzip file", err, errn); return -1; }
    while (!carry.finished) {
        uint64_t eff = slice_bytes;
        uint32_t grown = 0;
        SliceWalk w;
        SliceCut sc{};
        std::vector<uint64_t> cand;
        std::vector<std::vector<uint16_t>> cells;
        std::vector<std::vector<uint8_t>> host_bytes;
        std::vector<uint8_t> windowed;                 // per candidate: whether its block was decoded with a window in front of it
        for (;; grown++) {
            sc = slice_cut(carry, n, eff);
            // what the device sees: bytes [pos, end) of the file, zero behind them
            cand.clear();
            uint64_t entry = ~0ull;
            if (carry.in_member) entry = carry.bit;
            else if (carry.bit == 0) { const size_t body = member_body(gz, (size_t)n, 0); if (body < sc.end) entry = (uint64_t)body * 8; }
            for (uint64_t p = sc.pos * 8; p < sc.end * 8; p++)
                if (p == entry || header_like(gz, (size_t)sc.end, p)) cand.push_back(p);
            std::vector<BlockResult> res(cand.size());
            std::vector<uint32_t> res_of(cand.size());
            cells.assign(cand.size(), {});
            windowed.assign(cand.size(), 1);
            for (uint32_t k = 0; k < cand.size(); k++) {
                const DecodeJob j = decode_job(k, cand.data(), (uint32_t)cand.size(), sc.pos, sc.end, ratio, slack);
                const bool have_window = cand[k] == entry ? carry.have_window : true;
                windowed[k] = have_window;
                res[k] = model_decode(gz, (size_t)sc.end, j.start_bit, have_window, j.cap, cells[k]);
                res_of[k] = k;
            }
            host_bytes.clear();
            w = slice_walk(gz, n, carry, sc, cand, res_of.data(), res.data(), 0, [&](size_t p, size_t* end, uint64_t* n_out) {
                z_stream zs;
                memset(&zs, 0, sizeof(zs));
                if (inflateInit2(&zs, 16 + MAX_WBITS) != Z_OK) return false;
                std::vector<uint8_t> o(1u << 20);
                zs.next_in = const_cast<Bytef*>(gz + p);
                zs.avail_in = (uInt)std::min<uint64_t>(n - p, 1u << 18);
                zs.next_out = o.data();
                zs.avail_out = (uInt)o.size();
                const bool ok = inflate(&zs, Z_FINISH) == Z_STREAM_END;
                if (ok) { *end = p + zs.total_in; *n_out = zs.total_out; o.resize(zs.total_out); if (!o.empty()) host_bytes.push_back(o); }
                inflateEnd(&zs);
                return ok;
            });
            if (!w.why.empty()) { put_err(w.why, err, errn); return -1; }
            if (!w.grow) break;
            if (grown >= MAX_GROW) { put_err("a deflate block does not fit the slice, however often it was doubled", err, errn); return -1; }
            eff *= 2;
        }
        if (total + w.total > out_cap) { put_err("output buffer too small", err, errn); return -1; }
        // blocks that outgrew their region: again, with room for all of it
        const RedoPlan redo = redo_plan(w.blocks, cand.data());
        for (size_t q = 0; q < redo.jobs.size(); q++) {
            const ChainBlock& b = w.blocks[redo.which[q]];
            const bool have_window = windowed[b.cand] != 0;
            std::vector<uint16_t> again_cells;
            const BlockResult again = model_decode(gz, (size_t)sc.end, redo.jobs[q].start_bit, have_window, redo.jobs[q].cap, again_cells);
            if (again.n_out != b.n_out || (again.flags & 2)) { put_err("a block decoded a second time came out differently", err, errn); return -1; }
            cells[b.cand] = again_cells;
        }
        // the text: host pieces, then the blocks down the chain from the window the earlier slices left
        uint8_t* o0 = out + total;
        for (size_t i = 0; i < w.host.size(); i++) memcpy(o0 + w.host[i].out_off, host_bytes[i].data(), host_bytes[i].size());
        std::vector<uint8_t> win(WINDOW, 0);
        { const uint64_t have = std::min<uint64_t>(total, WINDOW); memcpy(win.data() + WINDOW - have, out + total - have, (size_t)have); }
        for (const ChainBlock& b : w.blocks) {
            const std::vector<uint16_t>& v = cells[b.cand];
            uint8_t* o = o0 + b.out_off;
            for (size_t i = 0; i < v.size(); i++) o[i] = v[i] < 256 ? (uint8_t)v[i] : win[v[i] - 256];
            if (v.size() >= WINDOW) memcpy(win.data(), o + v.size() - WINDOW, WINDOW);
            else { memmove(win.data(), win.data() + v.size(), WINDOW - v.size()); memcpy(win.data() + WINDOW - v.size(), o, v.size()); }
            if (n_blocks < blocks_cap) blocks_out[n_blocks] = cand[b.cand];
            n_blocks++;
        }
        // the members' CRCs, continued from the carry and into it
        uint64_t ended = 0, spanning = 0;
        for (const SliceMember& m : w.members) {
            if (m.on_host) continue;
            const uint64_t n_new = m.out_end - m.out_begin;
            const uint32_t reg = crc_continue(x2n, m.crc_before, crc_raw(tab, 0, o0 + m.out_begin, (size_t)n_new), n_new);
            if (!m.ends) { w.next.crc_raw = reg; continue; }
            ended++;
            spanning += m.len_before != 0;
            if (crc_finish(x2n, reg, m.len_before + n_new) != m.crc) { put_err("member: CRC-32 differs", err, errn); return -1; }
        }
        if (n_slices < trace_cap) {
            uint64_t* t = trace + (size_t)n_slices * TRACE;
            t[0] = sc.pos; t[1] = sc.cut; t[2] = sc.end;
            t[3] = carry.bit; t[4] = carry.in_member; t[5] = carry.member_len;
            t[6] = w.next.bit; t[7] = w.next.in_member; t[8] = w.next.member_len;
            t[9] = w.total; t[10] = grown; t[11] = spanning;
        }
        n_slices++;
        total += w.total;
        *good = total;
        carry = w.next;
    }
    *n_slices_out = n_slices;
    *n_blocks_out = n_blocks;
    return (long long)total;
}

}  // extern "C"
