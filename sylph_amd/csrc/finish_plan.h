// finish_plan.h — what a read-sketch session's finish does next (sketch.hip sketch_finish_impl), host-compilable: a pure function of
// where the occurrences lie, what the filter pass has left in their records, and what the last answer from the device was.  Three late
// answers meet in the finish — the seeding kernel's deferred verdict, the partitioned filter pass's verdict, the bucket replay's own
// tail — and each bad one means "undo something and start over"; this header is the only place that says in which order and how often.
// tests/test_finish_plan.py walks every state and every sequence of answers.
#pragma once

namespace sylph {
namespace finish_plan {

// Where the occurrences lie: in the slots of the session's one batch with the seeding kernel's verdict (and their number) still on
// the device, in those slots with the verdict read, or in the dense file-order arrays.  Only ever forwards: Deferred -> Known -> Dense.
enum class Place { Deferred, Known, Dense };
// What the filter dedup has left in the occurrence records (a10.hip): nothing (yet / any more: the slots that held the marks were
// given up), the partitioned pass's marks whose verdict words nobody has read, marks for good.
enum class Marks { None, Unread, Settled };
enum class Mode { Auto, Generic, Bucket };        // the ctx option "finish": the bucket path with the device-wide fallback / without the bucket path / without the fallback
// The last answer from the device: of the last attempt at the bucket path (replay_lds.hip finish_bucketed reads all three verdicts in
// its one tail block) or of a verdict read on its own.  It stays until the next answer.
enum class Outcome {
    None,            // nothing asked yet
    Done,            // the table is there (the driver stops; the plan is not asked again)
    Declined,        // not a sample for the bucket path (inconsistent bounds, overflowing buckets beyond what it patches); every verdict was read and was good
    SeedingBad,      // (of Deferred only) the batch was not one for the short-read kernel: nothing else of the tail means anything
    MarksBad,        // (of Unread only) the partitioned pass's marks are no good; the seeding verdict, if any, was good and is recorded
    NeedsRecords,    // (of a plain prefix only) k-mers deeper than the count kernels take: the usual kernels, on occurrence records
};
enum class Action {
    Mark,                // a10_mark: the partitioned pass where one filter suffices (-> Unread, place kept), else the walk (-> Settled, Dense)
    Attempt,             // finish_bucketed, once
    RedoDeferred,        // the deferred batch through the checked push (-> Known or Dense; the marks go with the slots: -> None)
    RemarkWalk,          // the phase walk over a sample the partitioned pass marked badly (-> Settled, Dense)
    WriteRecords,        // materialise_plain_records (-> no plain prefix)
    ReadSeedingVerdict,  // on its own, as a further push does: resolve_deferred_slots (-> Known, or redone at once: RedoDeferred's effect)
    ReadFilterVerdict,   // on its own: the two words (-> Settled, or the answer MarksBad)
    Replay,              // flush the slots, then the device-wide replay: the end
    Fail,                // "bucket finish overflowed and finish=bucket forbids the fallback": the end
};

struct State {
    Place place;
    Marks marks;
    bool plain;          // the first occurrences have no records (marker-less single-end batches)
    bool filter;         // the session dedups over the filter (paired, dedup_fpr > 0): the records need marks
    Mode mode;
    bool c_lt_2;         // c = 1: valid hashes reach the top bit that marks invalid occurrences; the bucket path takes no such sample
};

// The order is today's, and the results depend on it:
//  * a bad seeding verdict is handled before anybody looks at the filter verdict — the marks went into the slots that are given up;
//  * the walk leaves the sample dense, so the attempt after it partitions the arrays, not the slots;
//  * the device-wide replay runs on settled marks, a read seeding verdict (its flush cannot redo the batch any more) and records.
// Termination: an attempt is only repeated behind RedoDeferred, RemarkWalk or WriteRecords, and each of them makes a transition that
// no action undoes (Deferred -> Known/Dense, Unread -> Settled by the walk on a dense sample which no redo can touch any more, plain
// prefix -> records), so there are at most 1 + 3 attempts; Declined is never followed by another one.  Every other action moves place
// or marks forwards or is the end.
constexpr int MAX_ATTEMPTS = 4;

inline Action next(const State& s, Outcome last) {
    if (last == Outcome::SeedingBad && s.place == Place::Deferred) return Action::RedoDeferred;
    if (s.filter && s.marks == Marks::None) return Action::Mark;
    if (last == Outcome::MarksBad && s.marks == Marks::Unread) return Action::RemarkWalk;
    if (last == Outcome::NeedsRecords && s.plain) return Action::WriteRecords;
    if (s.mode != Mode::Generic && !s.c_lt_2 && last != Outcome::Declined) return Action::Attempt;
    if (s.mode == Mode::Bucket) return Action::Fail;
    // the device-wide path: what the attempt would have read with its tail is read on its own, the seeding verdict first
    if (s.place == Place::Deferred) return Action::ReadSeedingVerdict;
    if (s.filter && s.marks == Marks::Unread) return Action::ReadFilterVerdict;
    if (s.plain) return Action::WriteRecords;
    return Action::Replay;
}

}  // namespace finish_plan
}  // namespace sylph
