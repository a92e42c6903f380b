// A stand-alone driver for the decoders' host-compilable headers (sylph_amd/csrc/stream_plan.h, inflate_plan.h, bunzip2_plan.h), to be
// built with -fsanitize=address,undefined together with the three *_plan_capi.cpp models and run on the CPU
// (tests/test_stream_plan.py does both): the CRC family in both bit orders, Segments, the gzip layout functions, and both chain walks
// over the files it is given.  usage: <multi-member .gz> <its text> <two-stream .bz2>.  Exits 0 and prints a line; a sanitizer report
// fails the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

#include "../sylph_amd/csrc/bunzip2_plan.h"
#include "../sylph_amd/csrc/inflate_plan.h"

extern "C" {
uint32_t sp_crc_pieces(int reflected, const uint8_t* p, uint64_t n, uint64_t piece);
uint32_t sp_crc_shift(int reflected, uint32_t reg, uint64_t n_bytes);
uint64_t sp_segments_find(const uint64_t* sizes, uint32_t n_files, uint64_t pos, uint64_t* total);
long long ip_model_inflate(const uint8_t* gz, uint64_t n, uint8_t* out, uint64_t out_cap, uint64_t* info, uint32_t ratio, uint32_t slack, char* err, size_t errn);
int bp_model_chain(const uint8_t* const* files, const uint64_t* sizes, uint32_t n_files, const uint64_t* extra, uint32_t n_extra, uint32_t batch, uint64_t* info,
                   uint32_t* crcs, uint32_t* ns, uint32_t* files_of, uint32_t cap, char* err, size_t err_cap);
}

namespace {

std::vector<uint8_t> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
void require(bool ok, const char* what) {
    if (!ok) { fprintf(stderr, "FAILED: %s\n", what); exit(1); }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s multi.gz text two-stream.bz2\n", argv[0]); return 2; }
    const std::vector<uint8_t> gz = slurp(argv[1]), text = slurp(argv[2]), bz = slurp(argv[3]);
    namespace ip = sylph::inflate_plan;
    namespace bp = sylph::bunzip2_plan;

    // the CRC family: pieces of any size give one value; shifts compose; the plan headers' names are the family's
    for (int reflected = 0; reflected < 2; reflected++) {
        for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)65, (uint64_t)text.size()}) {
            const uint32_t whole = sp_crc_pieces(reflected, text.data(), n, n + 1);
            for (uint64_t piece : {1, 7, 64}) require(sp_crc_pieces(reflected, text.data(), n, piece) == whole, "CRC from pieces");
        }
        require(sp_crc_shift(reflected, 0x12345678u, 0) == 0x12345678u, "shift by 0");
        require(sp_crc_shift(reflected, 0x12345678u, (1ull << 32) + 5) == sp_crc_shift(reflected, sp_crc_shift(reflected, 0x12345678u, 1ull << 32), 5), "shifts compose");
    }
    uint32_t x2n[64], tab[256];
    ip::crc_x2n_table(x2n);
    ip::crc_byte_table(tab);
    require(ip::crc_finish(x2n, ip::crc_raw(tab, 0, text.data(), text.size()), text.size()) == sp_crc_pieces(1, text.data(), text.size(), 64), "inflate_plan's CRC names");
    bp::crc_x2n_table(x2n);
    bp::crc_byte_table(tab);
    require(bp::crc_finish(x2n, bp::crc_raw(tab, 0, text.data(), text.size()), text.size()) == sp_crc_pieces(0, text.data(), text.size(), 64), "bunzip2_plan's CRC names");

    // Segments: three files and an empty one between them
    const uint64_t sizes[4] = {1, 18, 0, 5};
    uint64_t total = 0;
    const uint64_t want[] = {0, 0, 1, 1, 18, 1, 19, 3, 23, 3};
    for (int i = 0; i < 5; i++) require(sp_segments_find(sizes, 4, want[2 * i], &total) == want[2 * i + 1] && total == 24, "Segments::find");

    // the layout functions over the gzip file's own numbers
    const uint64_t body0 = ip::member_body(gz.data(), gz.size(), 0);
    require(body0 != 0, "a gzip member header");
    const ip::Segments one = ip::one_segment(gz.data(), gz.size());
    require(ip::region_ratio_from_isize(one, 16) <= 16, "region ratio");
    const std::vector<uint64_t> cand = {body0 * 8, body0 * 8 + 3, (body0 + 1) * 8, (gz.size() - 1) * 8 + 7};
    for (uint64_t ratio : {1, 9, 16}) {
        const ip::CellsLayout l = ip::cells_layout(gz.size() - body0, (uint32_t)cand.size(), ratio, 1024, 96, 1u << 20);
        uint64_t end = 0;
        for (uint32_t i = 0; i < cand.size(); i++) {
            const ip::DecodeJob j = ip::decode_job(i, cand.data(), (uint32_t)cand.size(), body0, gz.size(), ratio, 1024);
            require(j.region >= end && j.start_bit == cand[i] && j.have_window == (i != 0), "regions in order");
            end = j.region + j.cap;
        }
        require(end <= l.n_cells && l.spill_base % 64 == 0 && l.spill_base >= l.n_cells && l.total > l.spill_base, "the cells buffer holds the regions");
    }
    std::vector<ip::ChainBlock> blocks;
    for (uint32_t i = 0; i < 6; i++) blocks.push_back(ip::ChainBlock{i % 4, 0, 0, 1 + 63 * i, i % 2 ? 2u : 1u});
    const ip::RedoPlan redo = ip::redo_plan(blocks, cand.data());
    require(redo.jobs.size() == 3 && redo.region.size() == 6 && redo.cells % 64 == 0, "the second decode's packing");
    require(ip::window_group(1) == 8 && ip::window_group(65) == 9 && ip::window_group(10000) == 100, "window groups");

    // both chain walks, through the CPU models of the kernels' reports
    std::vector<uint8_t> out(text.size() + 16);
    uint64_t info[5] = {0};
    char err[256] = "";
    for (uint32_t ratio : {16u, 1u}) {                     // ratio 1: blocks outgrow their regions and are decoded again
        const long long n = ip_model_inflate(gz.data(), gz.size(), out.data(), out.size(), info, ratio, ratio == 1 ? 0 : 1024, err, sizeof(err));
        require(n == (long long)text.size() && memcmp(out.data(), text.data(), text.size()) == 0, err[0] ? err : "the gzip road's text");
        require(info[0] >= 3 && info[1] >= 2 && info[3] >= 1 && (ratio == 1) == (info[4] != 0), "members, blocks, host members, blocks decoded again");
    }
    const uint64_t gz_members = info[0];
    const uint8_t* files[2] = {bz.data(), bz.data()};
    const uint64_t bz_sizes[2] = {bz.size(), bz.size()};
    const uint64_t extra[2] = {40, bz.size() * 8 + 77};
    uint32_t crcs[64], ns[64], files_of[64];
    for (uint32_t batch : {1u, 3u, 1000u}) {
        require(bp_model_chain(files, bz_sizes, 2, extra, 2, batch, info, crcs, ns, files_of, 64, err, sizeof(err)) == 0, err[0] ? err : "the bzip2 chain");
        require(info[0] == 4 && info[1] >= 4 && info[1] <= 64 && files_of[0] == 0 && files_of[info[1] - 1] == 1, "streams and blocks of two files");
    }
    printf("stream sanitize run ok: %llu gzip members, %llu bzip2 blocks\n", (unsigned long long)gz_members, (unsigned long long)info[1]);
    return 0;
}
