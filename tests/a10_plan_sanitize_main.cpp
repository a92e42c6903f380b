// A stand-alone program over sylph_amd/csrc/a10_plan.h (through tests/a10_plan_capi.cpp), to be built with -fsanitize=address,undefined and
// run on the CPU (tests/test_a10_plan.py does both): the sequential model of the partitioned pass over synthetic samples — ordinary items
// with a fifth repeated, 400 copies of one occurrence among them (resolved by slices), 3,000 copies (the verdict word is bumped) — at two
// false-positive rates and three splits, each against "not the first operation of its reduced-key class".  Exits 0 and prints a line; a
// wrong mark, a missing slice or verdict, or a sanitizer report fails.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

extern "C" int ap_model_selfcheck(uint64_t seed, uint32_t n, uint32_t copies, uint64_t capacity, double fpr, uint32_t split, uint64_t* out);

int main() {
    int runs = 0;
    for (double fpr : {1e-4, 0.3})
        for (uint32_t split : {1u, 2u, 4u}) {
            uint64_t o[4];
            if (ap_model_selfcheck(11, 30000, 0, 100000, fpr, split, o) || o[0] || o[1] || !o[3]) return 3;                 // several ranges
            if (ap_model_selfcheck(12, 8000, 400, 100000, fpr, split, o) || o[0] || o[1] || o[2] < 2 || o[3] < 798) return 4;    // slices, good verdict
            if (ap_model_selfcheck(13, 8000, 3000, 100000, fpr, split, o) || !o[1]) return 5;                                   // bad verdict
            runs += 3;
        }
    printf("a10 plan sanitize run ok: %d samples through the range model\n", runs);
    return 0;
}
