// A stand-alone driver for the streamed bzip2 decoder's host-compilable header (sylph_amd/csrc/bunzip2_stream_plan.h), to be built with
// -fsanitize=address,undefined together with tests/bunzip2_stream_plan_capi.cpp (the CPU model, one slice at a time) and run on the CPU
// (tests/test_bunzip2_stream_plan.py does both).  usage: (good|bad <file.bz2> <streams> <blocks>)...  A good file must walk to its end
// at every slice size and batch, its blocks tiling the chain, with the streams and blocks the test counted with Python's bz2; a bad one
// must be declined.  Exits 0 and prints a line; a sanitizer report fails the run.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

extern "C" {
void* bsp_open(const uint8_t* const* files, const uint64_t* sizes, uint32_t n_files, uint64_t slice_bytes, uint64_t overlap, uint32_t batch);
void bsp_close(void* h);
int bsp_next(void* h, const uint8_t* advance, const uint64_t* extra, uint32_t n_extra, uint64_t* blk, uint32_t cap, uint32_t* n_blk, uint64_t* state,
             uint8_t* finished, uint64_t* info, char* err, size_t err_cap);
}

namespace {

std::vector<uint8_t> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
void require(bool ok, const char* what, const char* file) {
    if (!ok) { fprintf(stderr, "FAILED: %s (%s)\n", what, file); exit(1); }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 5 || (argc - 1) % 4) { fprintf(stderr, "usage: %s (good|bad file.bz2 streams blocks)...\n", argv[0]); return 2; }
    unsigned runs = 0;
    for (int a = 1; a + 3 < argc; a += 4) {
        const bool good_file = !strcmp(argv[a], "good");
        // (exactly as large as the file: a byte read behind it is a report)
        const std::vector<uint8_t> bz = slurp(argv[a + 1]);
        const uint64_t want_streams = strtoull(argv[a + 2], nullptr, 10), want_blocks = strtoull(argv[a + 3], nullptr, 10);
        for (uint64_t slice : {(uint64_t)64 << 10, (uint64_t)96 << 10, (uint64_t)256 << 10}) {
            for (uint32_t batch : {1u, 1000u}) {
                const uint8_t* files[1] = {bz.data()};
                const uint64_t sizes[1] = {bz.size()};
                // the small overlap puts blocks on and behind the slices' ends (the model then reports their overrun)
                for (uint64_t overlap : {(uint64_t)0, (uint64_t)48 << 10}) {
                    void* h = bsp_open(files, sizes, 1, slice, overlap, batch);
                    uint64_t blocks = 0, at = 32, state[6] = {0};
                    uint8_t finished = 0;
                    bool declined = false;
                    for (unsigned turn = 0; turn < 100000 && !finished; turn++) {
                        std::vector<uint64_t> blk(4 * 64);
                        uint32_t n_blk = 0;
                        uint64_t info[3];
                        char err[256] = "";
                        const uint64_t extra[4] = {0, state[0] / 8 * 8, 0, state[0] + 777};   // false candidates at the slice's first bits and further on
                        if (bsp_next(h, nullptr, extra, 2, blk.data(), 64, &n_blk, state, &finished, info, err, sizeof(err)) != 0) {
                            require(err[0] != 0, "a decline says why", argv[a + 1]);
                            declined = true;
                            break;
                        }
                        for (uint32_t i = 0; i < n_blk && i < 64; i++) {
                            require(blk[4 * i + 1] >= at && blk[4 * i + 2] > blk[4 * i + 1], "blocks follow one another", argv[a + 1]);
                            at = blk[4 * i + 2];
                        }
                        blocks += n_blk;
                    }
                    bsp_close(h);
                    if (good_file && overlap == 0) {
                        require(!declined && finished, "a good file walks to its end", argv[a + 1]);
                        require(state[4] == want_streams && state[5] == want_blocks && blocks == want_blocks, "streams and blocks are counted", argv[a + 1]);
                    } else if (!good_file) {
                        require(declined, "a damaged file is declined", argv[a + 1]);
                    }
                    runs++;
                }
            }
        }
    }
    printf("bunzip2 stream sanitize run ok: %u runs\n", runs);
    return 0;
}
