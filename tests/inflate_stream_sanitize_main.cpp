// A stand-alone driver for the streamed inflate's host-compilable header (sylph_amd/csrc/inflate_stream_plan.h), to be built with
// -fsanitize=address,undefined together with tests/inflate_stream_plan_capi.cpp (the CPU model, one slice at a time) and run on the CPU
// (tests/test_inflate_stream_plan.py does both).  usage: (good|bad <file.gz> <its text>)...  A good file must come out equal to its text
// at every slice size, a bad one must be declined with every byte handed out before that equal to the text's.  Exits 0 and prints a line;
// a sanitizer report fails the run.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

extern "C" long long isp_model_stream(const uint8_t* gz, uint64_t n, uint64_t slice_bytes, uint32_t ratio, uint32_t slack, uint8_t* out, uint64_t out_cap,
                                      uint64_t* trace, uint32_t trace_cap, uint32_t* n_slices_out, uint64_t* blocks_out, uint32_t blocks_cap,
                                      uint32_t* n_blocks_out, uint64_t* good, char* err, size_t errn);

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
    if (argc < 4 || (argc - 1) % 3) { fprintf(stderr, "usage: %s (good|bad file.gz text)...\n", argv[0]); return 2; }
    unsigned runs = 0;
    for (int a = 1; a + 2 < argc; a += 3) {
        const bool good_file = !strcmp(argv[a], "good");
        const std::vector<uint8_t> gz = slurp(argv[a + 1]), text = slurp(argv[a + 2]);
        for (uint64_t slice : {(uint64_t)64 << 10, (uint64_t)96 << 10, (uint64_t)256 << 10}) {
            for (uint32_t ratio : {16u, 1u}) {
                if (ratio == 1 && slice != ((uint64_t)64 << 10)) continue;      // (every block decoded a second time: once per file)
                // (exactly as large as the text: a byte written behind it is a report)
                std::vector<uint8_t> out(text.size());
                std::vector<uint64_t> trace(12 * 64), blocks(64);
                uint32_t n_slices = 0, n_blocks = 0;
                uint64_t good = 0;
                char err[256] = "";
                const long long n = isp_model_stream(gz.data(), gz.size(), slice, ratio, ratio == 1 ? 0 : 1024, out.data(), out.size(), trace.data(), 64, &n_slices,
                                                     blocks.data(), 64, &n_blocks, &good, err, sizeof(err));
                if (good_file) {
                    require(n == (long long)text.size() && !memcmp(out.data(), text.data(), text.size()), "a good file equals its text", argv[a + 1]);
                    require(n_slices >= 1 && good == text.size(), "slices are counted", argv[a + 1]);
                } else {
                    require(n < 0 && err[0], "a damaged file is declined", argv[a + 1]);
                    require(good <= text.size() && !memcmp(out.data(), text.data(), (size_t)good), "what came before the damage is the text", argv[a + 1]);
                }
                runs++;
            }
        }
    }
    printf("inflate stream sanitize run ok: %u runs\n", runs);
    return 0;
}
