// C entry points over sylph_amd/csrc/pipeline_plan.h — the very header pipeline_core.h and pipeline.hip decide with — for
// tests/test_pipeline_plan.py (ctypes).  Tables instead of single calls where the test exhausts a space.
#include "../sylph_amd/csrc/pipeline_plan.h"

using namespace sylph::pipeline_plan;

extern "C" {

// Every vector of `len` states out of {Queued, Sketching, Sketched} (base-3 digits of its number, first sample = lowest digit)
// x every set of flush points in `masks` (bit b: a point at first + b), in that order: out = n | go << 8.
void pp_batch_table(uint32_t max_batch, int sharded, uint32_t len, uint64_t first, const uint32_t* masks, uint32_t n_masks, uint16_t* out) {
    uint32_t n_vectors = 1;
    for (uint32_t i = 0; i < len; i++) n_vectors *= 3;
    for (uint32_t v = 0; v < n_vectors; v++) {
        JobState st[16];
        for (uint32_t i = 0, rest = v; i < len; i++, rest /= 3) st[i] = (JobState)(rest % 3);
        for (uint32_t m = 0; m < n_masks; m++) {
            uint64_t flush[32];
            size_t n_flush = 0;
            for (uint32_t b = 0; b < 32; b++)
                if (masks[m] >> b & 1) flush[n_flush++] = first + b;
            const Batch r = next_batch([&](size_t i) { return st[i]; }, len, max_batch, sharded != 0, first, flush, n_flush);
            *out++ = (uint16_t)(r.n | (r.go ? 256u : 0u));
        }
    }
}
int pp_wait_for_fuller(uint32_t batch, uint32_t min_batch, uint32_t max_batch, uint32_t batch_wait_us, int sharded, uint64_t coming) {
    return wait_for_fuller(batch, min_batch, max_batch, batch_wait_us, sharded != 0, [&] { return coming; });
}
int pp_next_would_block(int sharded, int front_profiled, int flush_beyond_front, uint64_t unprofiled, uint32_t max_batch) {
    return next_would_block(sharded != 0, front_profiled != 0, flush_beyond_front != 0, unprofiled, max_batch);
}
int pp_flush_point_spent(uint64_t point, uint64_t first_unprofiled) { return flush_point_spent(point, first_unprofiled); }
void pp_slots(const uint8_t* good, uint32_t n, int probe_ok, int32_t* out) {
    Slots slots{probe_ok != 0};
    for (uint32_t i = 0; i < n; i++) out[i] = slots.take(good[i] != 0);
}
int pp_pick_replica(const int32_t* device, const uint32_t* outstanding, const uint32_t* depth, uint32_t n, int want_device) {
    Replica r[16];
    for (uint32_t i = 0; i < n; i++) r[i] = Replica{device[i], outstanding[i], depth[i]};
    return pick_replica(r, n, want_device);
}
int pp_no_replica_on_device() { return NO_REPLICA_ON_DEVICE; }
int pp_all_full() { return ALL_FULL; }
// what a config field left 0 becomes, for (n_workers, depth, max_batch) as given: out = workers, depth, max_batch, min_batch, batch_wait_us
void pp_defaults(uint32_t n_workers, uint32_t depth, uint32_t max_batch, uint32_t* out) {
    out[0] = workers_or_default(n_workers);
    out[1] = depth_or_default(depth, out[0]);
    out[2] = max_batch_or_default(max_batch);
    out[3] = DEFAULT_MIN_BATCH;
    out[4] = DEFAULT_BATCH_WAIT_US;
}
uint32_t pp_router_depth(uint32_t child_depth, uint32_t replicas) { return router_depth(child_depth, replicas); }
int pp_sharded_depth_ok(uint32_t depth, uint32_t max_batch) { return sharded_depth_ok(depth, max_batch); }

}  // extern "C"
