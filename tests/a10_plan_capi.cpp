// C wrapper around sylph_amd/csrc/a10_plan.h for tests/test_a10_plan.py and tests/a10_plan_sanitize_main.cpp (g++, no HIP): the very
// header a10.hip includes, plus a SEQUENTIAL model of the partitioned pass written from the header's functions alone — operation words,
// class ranges, grid, and per workgroup: bits, second arrivals, upper-half set, candidates, class table, marks, with the slicing and the
// verdict.  a10_range_kernel is these steps with atomics.
// Test infrastructure: the product never runs this.
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "../sylph_amd/csrc/a10_plan.h"

using namespace sylph;
using namespace sylph::a10_plan;
using sylph::replay_plan::bucket_of_key;

namespace {

RangeGeom geom_of(const uint32_t* g) { return RangeGeom{g[0], g[1], g[2]}; }

// One workgroup (range c, part) of the range pass.  false: a slice stayed too full (the verdict word is bumped, the marks are no good).
bool range_part(const std::vector<uint64_t>& words, uint32_t c, uint32_t part, uint32_t B, RangeGeom geo, FilterGeom d, const uint64_t* recs, uint8_t* marked,
                uint32_t* max_P) {
    if (words.empty()) return true;
    const uint32_t lo_key = range_lo_key(c, B);
    uint32_t P = 1, p = 0;
    auto my_slot = [&](uint32_t res) {
        const RangeSlot s = range_slot(res, geo);
        return s.part == part && slice_of(s.local, P) == p ? s.local : RNG_FREE;
    };
    while (p < P) {
        if (P > *max_P) *max_P = P;
        std::vector<uint32_t> bits(RNG_SLOTS / 32, 0u), sec, list;
        for (const uint64_t w : words) {                                      // bits, second arrivals
            const uint32_t res = range_residue(w, lo_key), l = my_slot(res);
            if (l == RNG_FREE) continue;
            if (bits[l >> 5] & (1u << (l & 31u))) sec.push_back(res);
            bits[l >> 5] |= 1u << (l & 31u);
        }
        uint32_t n_over = 2u * (uint32_t)sec.size();
        bool over = sec.size() > RNG_CAND;
        if (!over) {
            std::vector<uint32_t> up(RNG_TAB, RNG_FREE);                      // the upper-half set
            for (const uint32_t res : sec) {
                uint32_t at = up_home(res);
                while (up[at] != RNG_FREE && up[at] != res) at = tab_next(at);
                up[at] = res;
            }
            for (const uint64_t w : words) {                                  // candidates
                const uint32_t res = range_residue(w, lo_key);
                if (my_slot(res) == RNG_FREE) continue;
                uint32_t at = up_home(res);
                while (up[at] != RNG_FREE && up[at] != res) at = tab_next(at);
                if (up[at] == res) list.push_back((uint32_t)w);
            }
            n_over = (uint32_t)list.size();
            over = n_over > RNG_CAND;
        }
        if (over) {
            P = next_slices(P, n_over);
            if (!P) return false;
            p = 0;
            continue;
        }
        std::vector<uint64_t> t_key(RNG_TAB, ~0ull), t_min(RNG_TAB, ~0ull), key(list.size());      // the class table
        std::vector<uint32_t> at(list.size());
        for (size_t i = 0; i < list.size(); i++) {
            const uint32_t opid = list[i];
            const uint64_t* r = recs + 4 * (size_t)(opid >> 1);
            const uint64_t g = reduced_key(d, item_hash(r[0], (opid & 1u) ? r[3] : r[2]));
            key[i] = op_key(r[1], opid & 1u);
            at[i] = class_home(g);
            while (t_key[at[i]] != ~0ull && t_key[at[i]] != g) at[i] = tab_next(at[i]);
            t_key[at[i]] = g;
            if (key[i] < t_min[at[i]]) t_min[at[i]] = key[i];
        }
        for (size_t i = 0; i < list.size(); i++)                              // marks
            if (t_min[at[i]] < key[i]) marked[list[i]] = 1;
        p++;
    }
    return true;
}

uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace

extern "C" {

uint32_t ap_map_bytes() { return (uint32_t)sizeof(BucketMap); }
void ap_constants(uint64_t* v) {
    const uint64_t k[] = {FX_K, GOLD, NO_OP, (uint64_t)MAX_FILTERS, TILE_OCC, OPS_BLK_PER_TILE, RNG_SLOT_BITS, RNG_CAND, RNG_TAB, RNG_WORDS, MAX_SPLIT, MAX_SLICES,
                          SLICE_STOP, MAX_COARSE, XCDS, RNG_TPB, RID_RANK_MAX, RID_MARKER_BIT, INVALID_HASH};
    for (size_t i = 0; i < sizeof(k) / sizeof(k[0]); i++) v[i] = k[i];
}
void ap_item_hash(const uint64_t* km, const uint64_t* marker, uint64_t n, uint64_t* out) {
    for (uint64_t i = 0; i < n; i++) out[i] = item_hash(km[i], marker[i]);
}
int ap_filter_geometry(uint64_t capacity, double fpr, int j, uint32_t* masks) {
    FilterGeom g;
    const bool ok = filter_geometry(capacity, fpr, j, &g) == 0;
    masks[0] = g.fp_mask;
    masks[1] = g.nb_mask;
    return ok ? 1 : 0;
}
void ap_reduced_key(const uint64_t* h, uint64_t n, uint32_t fp_mask, uint32_t nb_mask, uint64_t* out) {
    for (uint64_t i = 0; i < n; i++) out[i] = reduced_key(FilterGeom{fp_mask, nb_mask}, h[i]);
}
uint64_t ap_op_key(uint64_t rid, uint32_t w) { return op_key(rid, w); }
uint64_t ap_op_word(uint32_t fp_mask, uint32_t nb_mask, uint64_t km, uint64_t marker, uint32_t opid) { return op_word(FilterGeom{fp_mask, nb_mask}, km, marker, opid); }
void ap_table_geometry(uint64_t remaining, uint64_t* out) {
    const TableGeom t = table_geometry(remaining);
    out[0] = t.slots;
    out[1] = t.tab_shift;
}
uint32_t ap_table_home(uint64_t g, uint32_t tab_shift) { return table_home(g, tab_shift); }
int ap_fits(uint64_t n_slots, uint64_t n_expect_filter, uint64_t n_plain, uint64_t capacity) { return fits(n_slots, n_expect_filter, n_plain, capacity) ? 1 : 0; }
int ap_verdict_good(uint32_t too_full, uint32_t n_ops, uint64_t capacity) { return verdict_good(too_full, n_ops, capacity) ? 1 : 0; }
void ap_cut_tile(const uint32_t* counts, uint32_t n_tiles, uint64_t cap, uint64_t* out) {
    const Cut c = cut_tile(counts, n_tiles, cap);
    out[0] = c.tile;
    out[1] = c.before;
}
void ap_class_map(uint64_t n_expect, uint32_t range_words, BucketMap* out) { *out = class_map(n_expect, range_words); }
uint64_t ap_class_range(uint32_t B) { return class_range(B); }
void ap_class_of_keys(const BucketMap* bm, const uint32_t* keys, uint64_t n, uint32_t* out) {
    for (uint64_t i = 0; i < n; i++) out[i] = bucket_of_key(keys[i], *bm);
}
void ap_range_lo_keys(uint32_t B, const uint32_t* c, uint64_t n, uint32_t* out) {
    for (uint64_t i = 0; i < n; i++) out[i] = range_lo_key(c[i], B);
}
void ap_range_geometry(uint32_t B, uint32_t split, uint32_t* out) {
    const RangeGeom g = range_geometry(B, split);
    out[0] = g.split;
    out[1] = g.all_slots;
    out[2] = g.slot_mult;
}
void ap_range_slots(const uint32_t* res, uint64_t n, const uint32_t* geo, uint32_t* part, uint32_t* local) {
    for (uint64_t i = 0; i < n; i++) {
        const RangeSlot s = range_slot(res[i], geom_of(geo));
        part[i] = s.part;
        local[i] = s.local;
    }
}
void ap_slice_of(const uint32_t* local, uint64_t n, uint32_t P, uint32_t* out) {
    for (uint64_t i = 0; i < n; i++) out[i] = slice_of(local[i], P);
}
uint32_t ap_next_slices(uint32_t P, uint32_t n_over) { return next_slices(P, n_over); }
void ap_range_of_blocks(uint32_t n_blocks, uint32_t split, uint32_t* c, uint32_t* part) {
    for (uint32_t b = 0; b < n_blocks; b++) {
        const RangeBlock r = range_of_block(b, split);
        c[b] = r.c;
        part[b] = r.part;
    }
}
uint32_t ap_range_grid(uint32_t B, uint32_t split) { return range_grid(B, split); }
void ap_table_homes(const uint64_t* v, uint64_t n, uint32_t* up, uint32_t* cls) {
    for (uint64_t i = 0; i < n; i++) {
        up[i] = up_home((uint32_t)v[i]);
        cls[i] = class_home(v[i]);
    }
}

// The partitioned pass over n occurrence records {hash, rid, m0, m1}: marked[2 i + w] = operation w of occurrence i was found contained;
// tail = the two verdict words; stats = {ranges, largest slice count any workgroup used, workgroups run}.  < 0: refused.
int ap_partitioned_pass(const uint64_t* recs, uint32_t n, uint64_t capacity, double fpr, uint32_t split, uint8_t* marked, uint32_t* tail, uint32_t* stats) {
    FilterGeom d;
    if (filter_geometry(capacity, fpr, 0, &d) || split < 1 || split > MAX_SPLIT) return -1;
    const BucketMap bm = class_map(n, RNG_WORDS);
    std::vector<std::vector<uint64_t>> range(bm.B);
    tail[0] = tail[1] = 0;
    for (uint32_t i = 0; i < n; i++) {                                        // the operation words, grouped by class range
        const uint64_t* r = recs + 4 * (size_t)i;
        if (r[0] == INVALID_HASH || !(r[1] & RID_MARKER_BIT)) continue;
        for (uint32_t w = 0; w < 2; w++) {
            const uint64_t word = op_word(d, r[0], r[2 + w], 2u * i + w);
            range[bucket_of_key((uint32_t)(word >> 32), bm)].push_back(word);
            tail[1]++;
        }
    }
    const RangeGeom geo = range_geometry(bm.B, split);
    stats[0] = bm.B;
    stats[1] = 1;
    stats[2] = 0;
    for (uint32_t b = 0; b < range_grid(bm.B, split); b++) {
        const RangeBlock blk = range_of_block(b, split);
        if (blk.c >= bm.B) continue;
        stats[2]++;
        if (!range_part(range[blk.c], blk.c, blk.part, bm.B, geo, d, recs, marked, &stats[1])) tail[0]++;
    }
    return 0;
}

// A synthetic sample from a seed — n occurrences of two per record, a fifth of them repeats of others, then `copies` copies of one
// occurrence spread among them — through the model and against "not the first operation of its reduced-key class by op_key".
// out = {operations marked wrongly, verdict word 0, largest slice count, operations marked}.  (what the stand-alone sanitizer program runs)
int ap_model_selfcheck(uint64_t seed, uint32_t n, uint32_t copies, uint64_t capacity, double fpr, uint32_t split, uint64_t* out) {
    std::vector<uint64_t> recs(4 * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        uint64_t* r = &recs[4 * (size_t)i];
        r[0] = splitmix(seed) >> 2;
        r[2] = splitmix(seed);
        r[3] = splitmix(seed);
    }
    for (uint32_t i = 0; i < n / 5; i++) {
        const size_t to = splitmix(seed) % n, from = splitmix(seed) % n;
        for (int f : {0, 2, 3}) recs[4 * to + f] = recs[4 * from + f];
    }
    for (uint32_t i = 0; i < copies; i++) {
        const size_t to = (size_t)i * (n / copies);
        for (int f : {0, 2, 3}) recs[4 * to + f] = recs[f];
    }
    for (uint32_t i = 0; i < n; i++) recs[4 * (size_t)i + 1] = RID_MARKER_BIT | ((uint64_t)(1u - (i & 1u)) << RID_RANK_SHIFT) | (i >> 1);
    std::vector<uint8_t> marked(2 * (size_t)n, 0);
    uint32_t tail[2], stats[3];
    if (ap_partitioned_pass(recs.data(), n, capacity, fpr, split, marked.data(), tail, stats) < 0) return -1;
    FilterGeom d;
    filter_geometry(capacity, fpr, 0, &d);
    std::unordered_map<uint64_t, uint64_t> first;
    for (uint32_t op = 0; op < 2 * n; op++) {
        const uint64_t* r = &recs[4 * (size_t)(op >> 1)];
        const uint64_t g = reduced_key(d, item_hash(r[0], r[2 + (op & 1u)])), key = op_key(r[1], op & 1u);
        auto it = first.emplace(g, key).first;
        if (key < it->second) it->second = key;
    }
    out[0] = out[3] = 0;
    for (uint32_t op = 0; op < 2 * n; op++) {
        const uint64_t* r = &recs[4 * (size_t)(op >> 1)];
        const bool want = first[reduced_key(d, item_hash(r[0], r[2 + (op & 1u)]))] < op_key(r[1], op & 1u);
        out[0] += want != (marked[op] != 0);
        out[3] += marked[op];
    }
    out[1] = tail[0];
    out[2] = stats[1];
    return 0;
}

}  // extern "C"
