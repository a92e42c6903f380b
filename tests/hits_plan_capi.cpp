// C wrapper around sylph_amd/csrc/hits_plan.h for tests/test_hits_plan.py and tests/hits_plan_sanitize_main.cpp (g++, no HIP): the very
// header hits.hip's kernels and contain.hip's finish_driver include, plus two small models — where rows_scan_kernel puts a row into
// the two row lists, and what the kernels behind every step of the driver zero — so that every walk of the driver can be made on the CPU.
// Test infrastructure: the product never runs this.
#include <cstdint>
#include <vector>

#include "../sylph_amd/csrc/hits_plan.h"

using namespace sylph::hits_plan;

namespace {

// A state in one word: to_probe | sizes << 1 | force_sort << 2 | rows_taken << 3 | finish << 4 | probes << 5 (2 bits) | assembled << 7 |
// read << 8 | verdict << 9 (2 bits) | rc_dirty << 11 | cnt_dirty << 12
uint32_t pack(const State& s) {
    return (uint32_t)s.to_probe | (uint32_t)s.sizes << 1 | (uint32_t)s.force_sort << 2 | (uint32_t)s.rows_taken << 3 | (uint32_t)s.finish << 4 | s.probes << 5 |
           (uint32_t)s.assembled << 7 | (uint32_t)s.read << 8 | (uint32_t)s.verdict << 9 | (uint32_t)s.rc_dirty << 11 | (uint32_t)s.cnt_dirty << 12;
}
State unpack(uint32_t w) {
    return State{(w & 1) != 0, (Sizes)(w >> 1 & 1), (w >> 2 & 1) != 0, (w >> 3 & 1) != 0, (w >> 4 & 1) != 0, w >> 5 & 3, (w >> 7 & 1) != 0, (w >> 8 & 1) != 0,
                 (Verdict)(w >> 9 & 3), (w >> 11 & 1) != 0, (w >> 12 & 1) != 0};
}

// What is in device memory: are the row counters all zero, are the probe's two words.  A step first clears what its launcher finds
// flagged dirty, must then find zero what it needs zero, and leaves what its kernels leave — assuming hits wherever there can be some.
struct Memory {
    bool rc_zero, cnt_zero;
};
// the five kernels over a list whose verdict is v, with the device words handed over or not
void chain(Memory& m, Verdict v, bool device_words) {
    m.rc_zero = false;                       // hits_count_kernel
    m.rc_zero = true;                        // rows_scan_kernel: the counters of the non-empty rows back to zero (their cursors)
    if (v != Verdict::Rows) return;          // snap[2]: the scatter and the sort return at once, nothing is zeroed behind it
    m.rc_zero = false;                       // hits_scatter_kernel moves the cursors
    m.rc_zero = true;                        // rows_sort_kernel: every listed row's cursor ...
    if (device_words) m.cnt_zero = true;     // ... and the two words it was handed
}
// -> false: the step found something it needs zero not zero
bool run(Memory& m, const State& before, Step step, Verdict answer) {
    switch (step) {
    case Step::Probe:
    case Step::RegrowProbe:
        if (before.cnt_dirty) m.cnt_zero = true;
        if (!m.cnt_zero) return false;
        m.cnt_zero = false;
        return true;
    case Step::Assemble:
        if (before.rc_dirty) m.rc_zero = true;
        if (!m.rc_zero) return false;
        if (before.read) chain(m, before.verdict, false);     // host-known sizes; behind a probe the chain runs on the words: see ReadWords
        else m.rc_zero = false;
        return true;
    case Step::ReadWords:
        if (before.assembled) chain(m, answer, true);
        return true;
    default:
        return true;
    }
}

struct Walk {
    uint64_t runs = 0, bad = 0, fails = 0, longest = 0;
    uint32_t most_probes = 0, most_assemblies = 0;
    uint64_t ends[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    void from(State s, Memory m, uint32_t steps, uint32_t probes, uint32_t assemblies, uint32_t overflows) {
        if (steps > 16) { bad++; return; }                               // the loop would not end
        const Step step = next(s);
        const bool last = step == Step::Sorted || step == Step::CopyOut || step == Step::Done || step == Step::Fail;
        if (last) {
            runs++;
            ends[(int)step]++;
            if (steps + 1 > longest) longest = steps + 1;
            if (probes > most_probes) most_probes = probes;
            if (assemblies > most_assemblies) most_assemblies = assemblies;
            if ((step == Step::Fail) != (overflows == 2)) bad++;         // fails exactly when the second probe overflowed again
            if (step == Step::Fail) fails++;
            if (step != Step::Fail && !s.finish && step != Step::Done) bad++;
            if (step == Step::CopyOut && !(s.assembled && s.read && s.verdict == Verdict::Rows && row_road(s))) bad++;
            if (step == Step::Sorted && s.assembled && s.verdict == Verdict::Rows) bad++;   // an assembled block is never sorted again
            if ((!s.rc_dirty && !m.rc_zero) || (!s.cnt_dirty && !m.cnt_zero)) bad++;        // the record claims no more than is true
            return;
        }
        if (step == Step::Assemble && (!row_road(s) || (s.read && s.verdict != Verdict::Rows))) bad++;
        if ((step == Step::Probe || step == Step::RegrowProbe) && !s.to_probe) bad++;
        if (step == Step::Probe || step == Step::RegrowProbe) probes++;
        if (step == Step::Assemble) assemblies++;
        const int n_answers = step == Step::ReadWords ? 3 : 1;
        for (int a = 0; a < n_answers; a++) {
            const Verdict answer = step == Step::ReadWords ? (Verdict)a : Verdict::Rows;
            Memory m2 = m;
            if (!run(m2, s, step, answer)) { bad++; continue; }
            const State t = after(s, step, answer);
            if ((!t.rc_dirty && !m2.rc_zero && !(step == Step::Assemble && !s.read)) || (!t.cnt_dirty && !m2.cnt_zero)) bad++;
            from(t, m2, steps + 1, probes, assemblies, overflows + (step == Step::ReadWords && answer == Verdict::Regrow ? 1 : 0));
        }
    }
};

}  // namespace

extern "C" {

void hp_constants(uint32_t* out) {
    out[0] = ROWS_TPB; out[1] = ROWS_PER_THREAD; out[2] = ROWS_TILE; out[3] = SMALL_ROW; out[4] = MAX_VALUE_LDS; out[5] = HIT_SLOTS;
    out[6] = HIT_SLOTS_FULL; out[7] = STRETCH_ROUND; out[8] = MAX_PROBES;
}

uint32_t hp_hash_row(uint32_t row) { return hash_row(row); }
uint32_t hp_rc_at(uint32_t row, uint32_t mask) { return rc_at(row, mask); }
void hp_stretch_of(uint32_t n, uint32_t grid, uint32_t block, uint32_t* lo, uint32_t* hi) { stretch_of(n, grid, block, *lo, *hi); }

// The stretches of all `grid` workgroups over n hits: 0 = disjoint, in block order, covering [0, n), every start a multiple of 256 or n;
// else 1 + the first block that breaks it
uint32_t hp_stretch_check(uint32_t n, uint32_t grid) {
    uint32_t at = 0;
    for (uint32_t b = 0; b < grid; b++) {
        uint32_t lo, hi;
        stretch_of(n, grid, b, lo, hi);
        if (lo != at || hi < lo || hi > n || (lo % STRETCH_ROUND != 0 && lo != n)) return 1 + b;
        at = hi;
    }
    return at == n ? 0 : 1 + grid;
}

// rc_at over [0, R2): 1 = every counter taken exactly once
int hp_rc_bijection(uint32_t R2) {
    std::vector<bool> seen(R2, false);
    for (uint32_t r = 0; r < R2; r++) {
        const uint32_t a = rc_at(r, R2 - 1);
        if (a >= R2 || seen[a]) return 0;
        seen[a] = true;
    }
    return 1;
}
// the windows of 16 consecutive rows starting in [first, first + count) whose counters do NOT lie on 16 different 64-byte lines
uint64_t hp_rc_shared_lines(uint32_t R2, uint32_t first, uint32_t count) {
    uint64_t shared = 0;
    for (uint32_t i = 0; i < count; i++) {
        uint32_t line[16];
        bool twice = false;
        for (uint32_t j = 0; j < 16; j++) {
            line[j] = rc_at(first + i + j, R2 - 1) >> 4;
            for (uint32_t k = 0; k < j; k++) twice = twice || line[k] == line[j];
        }
        shared += twice;
    }
    return shared;
}

// out: taken, R, R2, rc_mask, n_tiles, list_cap, hit_grid, rc_bytes, meta_bytes, tile_sum_at, snap_at, lists_at
void hp_geometry(uint64_t n_rows, uint64_t cap, uint64_t n_guess, uint64_t* out) {
    const Geometry g = geometry(n_rows, cap, n_guess);
    out[0] = g.taken; out[1] = g.R; out[2] = g.R2; out[3] = g.rc_mask; out[4] = g.n_tiles; out[5] = g.list_cap; out[6] = g.hit_grid;
    out[7] = g.rc_bytes; out[8] = g.meta_bytes; out[9] = g.tile_sum_at; out[10] = g.snap_at; out[11] = g.lists_at;
}

uint64_t hp_first_capacity(uint64_t total) { return first_capacity(total); }
int hp_fits(uint64_t cap) { return fits(cap); }
int hp_verdict(uint32_t n_counted, uint32_t max_count, uint32_t cap) { return (int)verdict(n_counted, max_count, cap); }

// The two row lists as rows_scan_kernel fills them (row order; the kernel's order differs, its places do not: every list is one
// counter): rows of 1 .. SMALL_ROW hits from the front of the geometry's list_cap entries, longer ones from the back.
// 0 = every entry inside the region and written once, else 1 + the first row that breaks it.  out: the two lengths.
uint64_t hp_place_rows(const uint32_t* counts, uint64_t n_rows, uint64_t cap, uint32_t* out) {
    const Geometry g = geometry(n_rows, cap, cap);
    if (!g.taken) return ~0ull;
    std::vector<uint8_t> lists(g.list_cap, 0);
    uint32_t ps = 0, pb = 0;
    for (uint64_t r = 0; r < n_rows; r++) {
        if (counts[r] == 0) continue;
        const uint64_t at = counts[r] <= SMALL_ROW ? (uint64_t)ps++ : (uint64_t)g.list_cap - 1 - pb++;   // (wraps past the front: caught below)
        if (at >= g.list_cap || lists[at]) return 1 + r;
        lists[at] = 1;
    }
    out[0] = ps; out[1] = pb;
    return 0;
}

uint32_t hp_start(int to_probe, int sizes, int force_sort, int rows_taken, int finish, int rc_dirty, int cnt_dirty, int known) {
    return pack(start(to_probe != 0, (Sizes)sizes, force_sort != 0, rows_taken != 0, finish != 0, rc_dirty != 0, cnt_dirty != 0, (Verdict)known));
}
int hp_next(uint32_t w) { return (int)next(unpack(w)); }
uint32_t hp_after(uint32_t w, int step, int answer) { return pack(after(unpack(w), (Step)step, (Verdict)answer)); }
uint32_t hp_failed(uint32_t w) { return pack(failed(unpack(w))); }
int hp_behind_probe(uint32_t w) { return behind_probe(unpack(w)); }

// Every walk from every start — probe or host-known sizes (Rows or Sorted), either source of the sizes, forced sort or not, rows the
// assembly takes or not, finish or hit list only, every combination of the two flags with the memory they describe — under every
// sequence of answers.  out: walks, violations, walks that failed, longest walk in steps, most probes, most assemblies, then the walks
// ending in each Step
void hp_walk_all(uint64_t* out) {
    Walk w;
    for (uint32_t bits = 0; bits < 128; bits++)
        for (int known = (int)Verdict::Sorted; known <= (int)Verdict::Rows; known++) {
            const bool to_probe = bits & 1, rc_dirty = bits & 32, cnt_dirty = bits & 64;
            if (to_probe && known != (int)Verdict::Rows) continue;
            const State s = start(to_probe, (Sizes)(bits >> 1 & 1), bits & 4, bits & 8, bits & 16, rc_dirty, cnt_dirty, (Verdict)known);
            w.from(s, Memory{!rc_dirty, !cnt_dirty}, 0, 0, 0, 0);
        }
    out[0] = w.runs; out[1] = w.bad; out[2] = w.fails; out[3] = w.longest; out[4] = w.most_probes; out[5] = w.most_assemblies;
    for (int i = 0; i < 8; i++) out[6 + i] = w.ends[i];
}

}  // extern "C"
