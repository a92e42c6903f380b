// C wrapper around sylph_amd/csrc/replay_plan.h for tests/test_replay_plan.py (g++, no HIP): the very header partition.h and
// replay_bucket.h include — the bucket map of the replay, evaluated for arrays of buckets, keys and distances.  Test infrastructure:
// the product never runs this.
#include "../sylph_amd/csrc/replay_plan.h"

using namespace sylph::replay_plan;

extern "C" {

// CAP_SMALL, CAP_MID, CAP_LARGE, LANE_CAP, LANE_CFG, N_CFG, IDX_BITS, SEG_LIMIT, then the capacity of every configuration index
void rp_constants(int32_t* out) {
    const int32_t head[8] = {CAP_SMALL, CAP_MID, CAP_LARGE, LANE_CAP, LANE_CFG, N_CFG, IDX_BITS, (int32_t)SEG_LIMIT};
    for (int i = 0; i < 8; i++) out[i] = head[i];
    for (int i = 0; i < N_CFG; i++) out[8 + i] = (int32_t)cap_of_cfg(i);
}
uint32_t rp_map_bytes() { return (uint32_t)sizeof(BucketMap); }
void rp_make_bucket_map(uint32_t c, uint32_t n_all, uint32_t bucket_target, uint64_t max_index, BucketMap* out) {
    *out = make_bucket_map(c, n_all, bucket_target, max_index);
}
void rp_bucket_lows(const BucketMap* bm, const uint32_t* b, uint64_t n, uint64_t* lo_key, uint64_t* lo_hash) {
    for (uint64_t i = 0; i < n; i++) {
        lo_key[i] = bucket_lo_key(b[i], bm->mult, bm->inv_mult);
        lo_hash[i] = bucket_lo_hash(b[i], bm->mult, bm->sh);
    }
}
void rp_bucket_of_keys(const BucketMap* bm, const uint32_t* key, uint64_t n, uint32_t* out) {
    for (uint64_t i = 0; i < n; i++) out[i] = bucket_of_key(key[i], *bm);
}
void rp_sub_ranges(const uint32_t* res, uint64_t n, uint32_t sub_mult, uint32_t cap, uint32_t* out) {
    for (uint64_t i = 0; i < n; i++) out[i] = sub_range_of(res[i], sub_mult, cap);
}

}  // extern "C"
