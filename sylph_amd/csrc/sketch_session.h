// sketch_session.h — state of one read-sketch session (shared by sketch.hip and replay_lds.hip).
#pragma once
#include <algorithm>

#include "common.h"
#include "a10_plan.h"
#include "finish_plan.h"
#include "replay_plan.h"
#include "seed_plan.h"

namespace sylph {
// rid: bit 63 = the record (pair) has dedup markers; bit 62 = approximate dedup only (a10.hip): the filter reported one of the
// occurrence's two (k-mer, markers) items as present; bits 42..61 = paired records with markers only: the occurrence's place in
// its record's EMISSION order (device_common.h emission_rank — the order extract_markers pushed the record's seeds in, which is the
// order sketch.rs:828-867 hands them to the dedup: it decides nothing for the exact set, and for the filter which of two items of
// one pair meets the other); bits 0..41 = global record index (file order; mate = bit 0).
// (RID_MARKER_BIT, RID_A10_BIT, RID_RANK_SHIFT, RID_RANK_MAX, RID_MASK and INVALID_HASH: a10_plan.h, which compiles without HIP)
// One surviving seed occurrence.  Array-of-structs (32 B, one sector) because finish() gathers occurrences through a sort
// permutation: four scattered 8 B reads per occurrence cost 4x the HBM sectors of one 32 B read.
struct alignas(32) OccRec { uint64_t hash, rid, m0, m1; };
}  // namespace sylph

namespace sylph {
void flush_pending_slots(sylph_sketch* sk);   // reads.hip
using replay_plan::key_shift;                 // replay_plan.h: key = hash >> key_shift(c), the 32-bit bucket key of an occurrence
// dedup: DEDUP_EXACT (dup_removal_lsh_full_exact), DEDUP_NONE (--no-dedup), DEDUP_FILTER (dup_removal_lsh_full: the marker test is
// the RID_A10_BIT a10_mark left in the records)
constexpr int DEDUP_EXACT = 0, DEDUP_NONE = 1, DEDUP_FILTER = 2;
void generic_replay(sylph_ctx* ctx, const uint64_t* d_hash, const OccRec* d_recs, uint32_t n_all, bool paired, int dedup,
                    DevBuf& out_k, DevBuf& out_c, uint64_t& n_out, uint64_t& removed_out);   // replay_generic.hip
// finish_plan.h: the finish is one loop (sketch.hip sketch_finish_impl) that asks the plan what to do next, does it, and feeds the answer back
using FinishOutcome = finish_plan::Outcome;
using FilterMarks = finish_plan::Marks;
// replay_lds.hip: ONE attempt at bucket partition + in-LDS replay.  It reads the seeding verdict, the filter verdict and its own tail in one
// block and says what happened; it undoes nothing and starts nothing over.  On a good seeding verdict the slots' count is recorded (pend)
// and good filter marks are accepted before it returns, whatever it returns.
FinishOutcome finish_bucketed(sylph_sketch* sk);
// reads.hip: one lane per record, seeding + markers fused; false = it declines the batch, having taken nothing
bool push_short_reads(sylph_sketch* sk, const uint8_t* d_bases, uint32_t phase, const uint64_t* d_off, uint64_t n_records, uint64_t n_bases, int enc);
void a10_mark(sylph_sketch* sk);              // a10.hip: marks the records (partitioned pass where one filter suffices, else the phase walk)
bool a10_verdict(sylph_sketch* sk, const uint32_t words[2]);   // a10.hip: are the partitioned pass's marks good, by its two verdict words?  Good marks are accepted (FilterMarks::Settled); nothing else happens
void a10_remark_walk(sylph_sketch* sk);       // a10.hip: the phase walk over a sample whose verdict was bad; leaves it dense
// A single-end session whose records carry no dedup markers so far (long reads: sketch.rs:922-927 passes no marker above 400
// bases; --no-dedup) keeps only the hashes of its occurrences — nothing the replay looks at besides the hash exists for them
// (no marker, no mate) — and finish() counts them without occurrence records.  The first batch that may carry markers (or a
// finish that needs the records after all) writes the records of what is there: OccRec{hash, 0, 0, 0}.
void materialise_plain_records(sylph_sketch* sk);   // sketch.hip
}

namespace sylph {
// The occurrences of the last short-read batch, still in the per-block slots the seeding kernel wrote them to (reads.hip).
// A sample that arrives in ONE batch — the device-resident case — never has them compacted: finish() partitions straight from
// the slots (replay_lds.hip).  A further batch, a batch with overflowing blocks, or the device-wide finish move them to the
// dense file-order arrays first (flush_pending_slots).
struct PendingSlots {
    bool live = false;
    uint32_t n_blk = 0, slot_cap = 0, n = 0;   // blocks, slots per block, occurrences in the region (deferred: an upper bound)
    // Deferred (round 4): the seeding kernel's verdict — a record too long for it, a block that overflowed its slots, the number of
    // occurrences — has NOT been read back yet.  Only for a session whose caller keeps the batch's memory valid until finish
    // ("borrow_until_finish": the pipeline's device batches, bench.py): finish_bucketed sizes everything from `n_expect` / `n`
    // (estimate / upper bound), takes every count from device memory, and reads the verdict together with its own tail block —
    // one host round trip per sample instead of two.  A bad verdict is the finish loop's to act on (finish_plan.h: redo_deferred_batch).
    bool deferred = false;
    uint32_t n_expect = 0;
    const uint8_t* bases = nullptr;            // the borrowed batch, for the redo
    uint32_t phase = 0;
    const uint64_t* off = nullptr;
    uint64_t n_records = 0, n_bases = 0;
    int enc = 0;
};
void resolve_deferred_slots(sylph_sketch* sk);   // reads.hip: reads the verdict now (block total + flags); may redo the batch
void redo_deferred_batch(sylph_sketch* sk);      // sketch.hip: the deferred batch once more, through the ordinary (checked) push
// Where the occurrences lie and how many there are, for everything that sizes a pass over them (a10_mark, a10_mark_partitioned,
// finish_bucketed).  A deferred batch has no count on the host: an upper bound for what arrays must hold, and TWO expectations, kept
// apart because results (which pass marks; the bucket geometry) depend on each: the seeding plan's for geometry, an eighth more for
// the question whether one filter takes every operation.
struct Occurrences {
    finish_plan::Place place;
    uint64_t n_slots;          // the region a pass walks: the batch's slots (blocks x slots per block), or the dense arrays
    uint32_t n_cap;            // what arrays sized by occurrence must hold (deferred: an upper bound)
    uint32_t n_expect;         // geometry: the count; deferred: the expected count, at least 1
    uint64_t n_expect_filter;  // fits-one-filter test: the count; deferred: the expectation + 1/8
    uint64_t n_plain;          // the first n_plain have no OccRec (marker-less single-end batches)
    bool slotted() const { return place != finish_plan::Place::Dense; }
    bool deferred() const { return place == finish_plan::Place::Deferred; }
};
}  // namespace sylph

struct sylph_sketch {
    sylph_ctx* ctx;
    uint32_t c, k;
    int paired, no_dedup, avx2_compat;
    bool finished = false;
    bool borrow_until_finish = false;   // the caller keeps device batches valid until finish (sylph_sketch_set_option; see PendingSlots)
    double dedup_fpr = 0.;              // > 0 (paired sessions): the reference's default dedup over a cuckoo filter of this false-positive probability (a10.hip)
    uint64_t dedup_capacity = 10000000; // its initial capacity (sketch.rs:800)
    // a10.hip: None = the records carry no marks (yet / any more: the slots that held them were given up), Unread = marked by the
    // partitioned pass, whose verdict words (a10_tail: buckets that overflowed, operations found) nobody has read yet, Settled = for good
    sylph::FilterMarks a10_marks = sylph::FilterMarks::None;
    int a10_force = 0;                  // session/test knob ("a10": 0 auto, 1 always the walk, 2 the partitioned pass wherever one filter suffices)
    bool filter_dedup() const { return paired && !no_dedup && dedup_fpr > 0.; }
    int dedup_mode() const { return no_dedup ? sylph::DEDUP_NONE : (filter_dedup() ? sylph::DEDUP_FILTER : sylph::DEDUP_EXACT); }
    uint64_t rec_base = 0;         // records pushed so far
    uint64_t n_occ = 0;            // occurrences (valid + invalid) appended so far
    uint64_t n_plain = 0;          // the first n_plain of them have no OccRec (marker-less single-end batches, see materialise_plain_records)
    sylph::DevBuf hash;                   // hash of every occurrence, file order (sort key)
    sylph::DevBuf recs;                   // OccRec of every occurrence, file order
    sylph::DevBuf slot_bases[2], slot_off[2];   // device slots of the host-batch pipeline (copy stream fills one, kernels read the other)
    sylph::DevBuf slot_rec, slot_key, slot_meta;   // reads.hip: per-block occurrence slots (OccRec | 32-bit bucket key) and block tables
    sylph::PendingSlots pend;
    sylph::DevBuf batch_ascii;            // a packed batch expanded to ASCII for the position-kernel path
    sylph::DevBuf fq_bases, fq_off;       // fastq.hip: the batch sylph_sketch_push_fastq gathered from FASTQ text (valid until the next such push)
    sylph::DevBuf out_k, out_c;           // final table
    uint64_t n_out = 0, dup_removed = 0;
    sylph::DevBuf counters;               // 16 u32 words; in use: CNT_SURVIVORS, CNT_MARKED (below); each is cleared by the path that uses it
    sylph::DevBuf a10_tail;               // a10.hip: verdict words of the partitioned pass (see a10_marks)
    sylph::Occurrences occurrences() const {
        using sylph::finish_plan::Place;
        if (!pend.live) return {Place::Dense, n_occ, (uint32_t)n_occ, (uint32_t)n_occ, n_occ, n_plain};
        const uint64_t region = (uint64_t)pend.n_blk * pend.slot_cap;
        if (!pend.deferred) return {Place::Known, region, pend.n, pend.n, pend.n, n_plain};
        return {Place::Deferred, region, pend.n, std::max<uint32_t>(1, pend.n_expect), (uint64_t)pend.n_expect + pend.n_expect / 8, n_plain};
    }
    // The session gives up the slots of its (deferred) batch — and with them whatever marks the filter pass left in their records.
    sylph::PendingSlots drop_pending_slots() {
        const sylph::PendingSlots d = pend;
        pend = sylph::PendingSlots{};
        a10_marks = sylph::FilterMarks::None;
        return d;
    }
    explicit sylph_sketch(sylph_ctx* cx)
        : ctx(cx), hash(cx), recs(cx), slot_bases{sylph::DevBuf(cx), sylph::DevBuf(cx)}, slot_off{sylph::DevBuf(cx), sylph::DevBuf(cx)},
          slot_rec(cx), slot_key(cx), slot_meta(cx), batch_ascii(cx), fq_bases(cx), fq_off(cx), out_k(cx), out_c(cx), counters(cx), a10_tail(cx) {}
};

namespace sylph {
// Words of sylph_sketch::counters (u32 index).  CNT_SURVIVORS: the unordered position kernel's count of survivors (seeds_sorted_by_pos's
// d_count).  CNT_MARKED: marker_lengths_kernel's flag — bit 0 set when some record of the batch has a length that carries a dedup
// marker.  Apart: the count comes back inside seeds_sorted_by_pos while the flag, written before it, is still waiting to be read.
constexpr uint32_t CNT_SURVIVORS = 0, CNT_MARKED = 6;
// the block tables the short-read kernel left in the session's slot_meta buffer (seed_plan.h SlotMeta)
inline seed_plan::SlotMeta slot_meta_of(sylph_sketch* sk, uint32_t n_blk) { return seed_plan::SlotMeta(sk->slot_meta.as<uint32_t>(), n_blk); }
}  // namespace sylph
