// pipeline_plan.h — everything the sample pipeline DECIDES (pipeline_core.h runs its threads and queues over these functions,
// pipeline.hip does the GPU work), host-compilable and pure: the next probe batch, the short wait for a fuller one, whether a call
// of sylph_pipeline_next could ever be woken, the slots inside a shared result block, the router's choice of a replica, and the
// defaults include/sylph_hip.h quotes.  tests/test_pipeline_plan.py walks every small case of each.
#pragma once

#include <cstddef>
#include <cstdint>

namespace sylph {
namespace pipeline_plan {

// ---- the defaults (sylph_pipeline_config: a field left 0) ----
constexpr uint32_t DEFAULT_WORKERS = 3, DEFAULT_MAX_BATCH = 8, DEFAULT_DEPTH_BEYOND_WORKERS = 5;
constexpr uint32_t DEFAULT_MIN_BATCH = 1, DEFAULT_BATCH_WAIT_US = 400;       // the options "min_batch" / "batch_wait_us"
inline uint32_t workers_or_default(uint32_t n_workers) { return n_workers ? n_workers : DEFAULT_WORKERS; }
inline uint32_t max_batch_or_default(uint32_t max_batch) { return max_batch ? max_batch : DEFAULT_MAX_BATCH; }
inline uint32_t depth_or_default(uint32_t depth, uint32_t n_workers) { return depth ? depth : n_workers + DEFAULT_DEPTH_BEYOND_WORKERS; }
inline uint32_t router_depth(uint32_t child_depth, uint32_t replicas) { return child_depth * replicas; }
// sharded: a full batch of the exchange must fit among the outstanding samples, or it could never form
inline bool sharded_depth_ok(uint32_t depth, uint32_t max_batch) { return depth >= max_batch; }

// A sample's way through the pipeline; only ever forwards.
enum class JobState : uint8_t { Queued, Sketching, Sketched, Profiled };

// ---- the next probe batch ----
// `state(i)`, i < n: the samples in submission order from the first one that is not profiled (sequence number `first`).
// `flush`: the pending flush points in the order they were made (ascending) — a point is the number of samples that had been
// submitted when sylph_pipeline_flush was called, so the samples below it may go in a batch smaller than max_batch.
// Unsharded: the consecutive sketched samples, at most max_batch, as soon as there is one.
// Sharded: the ranks must enter the exchange with the same batches whatever the timing of their workers, so the SIZE is a function
// of the call sequence alone — max_batch, or what lies below the oldest flush point beyond `first` — and the batch goes when
// exactly that many samples are sketched.  (A later flush never moves an earlier boundary: the points queue up.)
struct Batch {
    uint32_t n;      // samples in the batch (sharded: also while it cannot go yet)
    bool go;
};
template <class StateAt>
Batch next_batch(StateAt&& state, size_t n, uint32_t max_batch, bool sharded, uint64_t first, const uint64_t* flush, size_t n_flush) {
    uint64_t want = max_batch;
    for (size_t i = 0; sharded && i < n_flush; i++)
        if (flush[i] > first) { if (flush[i] - first < want) want = flush[i] - first; break; }
    uint32_t run = 0;
    while (run < n && run < want && state(run) == JobState::Sketched) run++;
    if (!sharded) return Batch{run, run > 0};
    return Batch{(uint32_t)want, want > 0 && run == want};
}
// a flush point is spent once the profiled samples have reached it
inline bool flush_point_spent(uint64_t point, uint64_t first_unprofiled) { return point <= first_unprofiled; }

// ---- the short wait for a fuller batch ("min_batch", "batch_wait_us") ----
// A fuller launch is cheaper per table, so a batch below min(min_batch, max_batch) waits a little for the samples that are queued
// or being sketched — never for samples nobody has submitted, and never on a sharded pipeline (its batches are fixed).
// `coming()` counts those samples; it is only asked when everything else says wait (it walks the outstanding jobs).
template <class Coming>
bool wait_for_fuller(uint32_t batch, uint32_t min_batch, uint32_t max_batch, uint32_t batch_wait_us, bool sharded, Coming&& coming) {
    return !sharded && batch_wait_us && batch < (min_batch < max_batch ? min_batch : max_batch) && coming() > 0;
}

// ---- would sylph_pipeline_next block for ever? ----
// Only a sharded pipeline can: its profile thread waits for a batch of a fixed size, and with the front sample not profiled, no
// flush point beyond it and fewer than max_batch samples unprofiled, no worker's progress can complete one.
inline bool next_would_block(bool sharded, bool front_profiled, bool flush_beyond_front, uint64_t unprofiled, uint32_t max_batch) {
    return sharded && !front_profiled && !flush_beyond_front && unprofiled < max_batch;
}

// ---- slots in a batch's shared result block ----
// The probe runs over the batch's good samples (those whose sketch did not fail), in batch order: they get consecutive slots.  A
// failed sample gets none, and a failed probe fails every good sample of its batch.
struct Slots {
    bool probe_ok;
    uint32_t next = 0;
    int take(bool good) { return good && probe_ok ? (int)next++ : -1; }      // -> the sample's slot, or -1
};

// ---- the router's choice ----
// Among the replicas on `device` (-1: any) the one with the fewest samples outstanding that is below its depth.
struct Replica {
    int device;
    uint32_t outstanding, depth;
};
constexpr int NO_REPLICA_ON_DEVICE = -1, ALL_FULL = -2;
inline int pick_replica(const Replica* r, size_t n, int device) {
    int best = NO_REPLICA_ON_DEVICE;
    for (size_t i = 0; i < n; i++) {
        if (device >= 0 && r[i].device != device) continue;
        if (r[i].outstanding >= r[i].depth) { if (best < 0) best = ALL_FULL; continue; }
        if (best < 0 || r[i].outstanding < r[(size_t)best].outstanding) best = (int)i;
    }
    return best;
}

}  // namespace pipeline_plan
}  // namespace sylph
