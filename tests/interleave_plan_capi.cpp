// C wrapper around sylph_amd/csrc/interleave_plan.h for tests/test_interleave_plan.py and tests/interleave_plan_sanitize_main.cpp
// (g++, no HIP): the very header the mate-check kernel and the host's roads include.  ip_group_mates replays the kernel's walk — a
// group of GROUP_LANES lanes, their four votes per step, one MateScan — sequentially.  Test infrastructure: the product never runs this.
#include "../sylph_amd/csrc/interleave_plan.h"

using namespace sylph::interleave_plan;

extern "C" {

uint64_t ip_pairs_of(uint64_t n) { return pairs_of(n); }
uint64_t ip_kept_record(uint64_t n) { return kept_record(n); }
uint64_t ip_mean_record(uint64_t pair) { return mean_record(pair); }
uint64_t ip_mean_stride() { return MEAN_STRIDE; }
uint64_t ip_record_of(uint64_t pair, uint32_t mate) { return record_of(pair, mate); }
uint32_t ip_group_lanes() { return GROUP_LANES; }
uint64_t ip_id_len(const uint8_t* h, uint64_t n) { return id_len(h, n); }
int ip_mates(const uint8_t* a, uint64_t la, const uint8_t* b, uint64_t lb) { return mates(a, la, b, lb) ? 1 : 0; }
// headers (behind their '@' / '>'; with or without a line end) -> whether the records are mates, by the sequential rule
int ip_header_mates(const uint8_t* ha, uint64_t na, const uint8_t* hb, uint64_t nb) {
    return mates(ha, id_len(ha, na), hb, id_len(hb, nb)) ? 1 : 0;
}
// ... and by the kernel's walk; *steps: how many steps it took
int ip_group_mates(const uint8_t* ha, uint64_t na, const uint8_t* hb, uint64_t nb, uint32_t* steps) {
    const uint32_t ha_n = header_bytes(na), hb_n = header_bytes(nb);
    MateScan s;
    uint8_t carry = 0;
    uint32_t n_steps = 0;
    for (uint32_t base = 0;; base += GROUP_LANES) {
        uint32_t end_a = 0, end_b = 0, differ = 0, slash12 = 0;
        uint8_t front = carry;
        for (uint32_t l = 0; l < GROUP_LANES; l++) {
            const uint32_t x = base + l;
            const uint8_t ca = byte_at(ha, ha_n, x), cb = byte_at(hb, hb_n, x);
            end_a |= (uint32_t)is_id_end(ca) << l;
            end_b |= (uint32_t)is_id_end(cb) << l;
            differ |= (uint32_t)(ca != cb) << l;
            slash12 |= (uint32_t)lane_slash12(ca, cb, front, x) << l;
            front = ca;
        }
        carry = front;
        s.step(base, end_a, end_b, differ, slash12);
        n_steps++;
        if (s.done()) break;
    }
    if (steps) *steps = n_steps;
    return s.verdict() ? 1 : 0;
}

}  // extern "C"
