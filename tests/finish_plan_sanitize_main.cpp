// A stand-alone program over sylph_amd/csrc/finish_plan.h (through tests/finish_plan_capi.cpp), to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_finish_plan.py does both): the walk of every run of the finish loop from
// every initial state, under every sequence of answers the device may give.  Every run must end (in a finished attempt, the device-wide
// replay or the finish=bucket failure) without visiting a state twice and without an action whose precondition does not hold, within
// the header's bound on the attempts.  Exits 0 and prints a line; a violation or a sanitizer report fails.
#include <cstdint>
#include <cstdio>

extern "C" {
int fp_max_attempts();
void fp_walk_all(int64_t* out);
}

int main() {
    int64_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    fp_walk_all(w);
    if (w[4] != 0) return 3;                                     // a state twice, or an action out of place
    if (w[0] == 0 || w[0] != w[1] + w[2] + w[3] || !w[1] || !w[2] || !w[3]) return 4;
    if (w[5] != fp_max_attempts() || w[6] < 0) return 5;         // attempts <= 1 + one-way transitions, and the bound is reached
    printf("finish plan sanitize run ok: %lld runs (%lld done, %lld device-wide, %lld refused), at most %lld attempts, longest run %lld steps\n",
           (long long)w[0], (long long)w[1], (long long)w[2], (long long)w[3], (long long)w[5], (long long)w[7]);
    return 0;
}
