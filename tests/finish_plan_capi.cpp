// C wrapper around sylph_amd/csrc/finish_plan.h for tests/test_finish_plan.py and tests/finish_plan_sanitize_main.cpp (g++, no HIP): the
// very header sketch.hip's sketch_finish_impl includes, plus a model of what every action can do to the session — the answers the
// device may give — so that every run of the finish loop can be walked on the CPU.
// Test infrastructure: the product never runs this.
#include <cstdint>
#include <vector>

#include "../sylph_amd/csrc/finish_plan.h"

using namespace sylph::finish_plan;

namespace {

// A state and the last answer in one word: place + 3 marks + 9 plain + 18 filter + 36 mode + 108 c_lt_2 + 216 last
constexpr uint32_t N_STATES = 216;
uint32_t pack(const State& s, Outcome last) {
    return (uint32_t)s.place + 3u * (uint32_t)s.marks + 9u * s.plain + 18u * s.filter + 36u * (uint32_t)s.mode + 108u * s.c_lt_2 + N_STATES * (uint32_t)last;
}
State state_of(uint32_t w) {
    return State{(Place)(w % 3), (Marks)(w / 3 % 3), (w / 9 % 2) != 0, (w / 18 % 2) != 0, (Mode)(w / 36 % 3), (w / 108 % 2) != 0};
}
Outcome last_of(uint32_t w) { return (Outcome)(w / N_STATES); }

// What `a` can leave behind when it is done in (s, last): every (state, last answer) the device's answers allow.  An attempt that ends
// the finish reports last = Done.  false = the action cannot be done here at all (its precondition does not hold).
bool successors(State s, Outcome last, Action a, std::vector<uint32_t>& out) {
    out.clear();
    auto put = [&](State t, Outcome l) { out.push_back(pack(t, l)); };
    auto with = [](State t, Place p, Marks m) { t.place = p; t.marks = m; return t; };
    switch (a) {
    case Action::Mark:                                   // the partitioned pass where the occurrences lie, or the walk (which flushes the slots)
        if (!s.filter || s.marks != Marks::None) return false;
        put(with(s, s.place, Marks::Unread), last);
        put(with(s, Place::Dense, Marks::Settled), last);
        return true;
    case Action::Attempt: {
        if (s.mode == Mode::Generic || s.c_lt_2) return false;
        for (int wrote = 0; wrote <= (s.plain ? 1 : 0); wrote++) {        // a tiny marker-less sample gets its records written on the way
            State t = s;
            if (wrote) t.plain = false;
            put(t, Outcome::Done);
            if (t.place == Place::Deferred) put(t, Outcome::SeedingBad);  // nothing recorded
            if (t.place == Place::Deferred) t.place = Place::Known;       // the seeding verdict was good: recorded first
            if (t.marks == Marks::Unread) put(t, Outcome::MarksBad);
            if (t.marks == Marks::Unread) t.marks = Marks::Settled;
            put(t, Outcome::Declined);
            if (t.plain) put(t, Outcome::NeedsRecords);
        }
        return true;
    }
    case Action::RedoDeferred:                           // the checked push leaves the batch in slots again, or dense; the marks went with the old slots
        if (s.place != Place::Deferred) return false;
        put(with(s, Place::Known, Marks::None), last);
        put(with(s, Place::Dense, Marks::None), last);
        return true;
    case Action::RemarkWalk:
        if (s.marks != Marks::Unread) return false;
        put(with(s, Place::Dense, Marks::Settled), last);
        return true;
    case Action::WriteRecords:
        if (!s.plain) return false;
        s.plain = false;
        put(s, last);
        return true;
    case Action::ReadSeedingVerdict:                     // good (no occurrence at all: no slots either), or bad and redone at once
        if (s.place != Place::Deferred) return false;
        put(with(s, Place::Known, s.marks), last);
        put(with(s, Place::Dense, s.marks), last);
        put(with(s, Place::Known, Marks::None), last);
        put(with(s, Place::Dense, Marks::None), last);
        return true;
    case Action::ReadFilterVerdict:
        if (s.marks != Marks::Unread || s.place == Place::Deferred) return false;   // (the seeding verdict first: the marks go with the slots)
        put(with(s, s.place, Marks::Settled), last);
        put(s, Outcome::MarksBad);
        return true;
    case Action::Replay:                                 // settled marks, a flush that cannot redo the batch, records
        return (!s.filter || s.marks == Marks::Settled) && s.place != Place::Deferred && !s.plain;
    case Action::Fail:
        return s.mode == Mode::Bucket;
    }
    return false;
}

bool one_way(Action a) { return a == Action::RedoDeferred || a == Action::RemarkWalk || a == Action::WriteRecords; }

struct Walk {
    uint64_t runs = 0, done = 0, replay = 0, fail = 0, bad = 0, longest = 0;
    int64_t most_attempts = 0, least_slack = 1 << 20;           // slack = 1 + one-way transitions - attempts
    std::vector<uint32_t> seen;                                  // (state, last) words on the current run
    void from(uint32_t w, int attempts, int transitions) {
        for (uint32_t v : seen) if (v == w) { bad++; return; }   // a state visited twice: the loop would not end
        seen.push_back(w);
        const State s = state_of(w);
        const Action a = next(s, last_of(w));
        std::vector<uint32_t> succ;
        if (!successors(s, last_of(w), a, succ)) bad++;
        else if (a == Action::Replay || a == Action::Fail) end(a == Action::Replay ? replay : fail, attempts, transitions);
        else {
            if (a == Action::Attempt) attempts++;
            if (one_way(a)) transitions++;
            for (uint32_t v : succ) {
                if (last_of(v) == Outcome::Done && a == Action::Attempt) {
                    seen.push_back(v);
                    end(done, attempts, transitions);
                    seen.pop_back();
                } else from(v, attempts, transitions);
            }
        }
        seen.pop_back();
    }
    void end(uint64_t& kind, int attempts, int transitions) {
        runs++; kind++;
        if (seen.size() > longest) longest = seen.size();
        if (attempts > most_attempts) most_attempts = attempts;
        if (1 + transitions - attempts < least_slack) least_slack = 1 + transitions - attempts;
    }
};

}  // namespace

extern "C" {

int fp_max_attempts() { return MAX_ATTEMPTS; }

int fp_next(uint32_t w) { return (int)next(state_of(w), last_of(w)); }

// The words `action` can leave behind (at most 16), -1 when it cannot be done in w
int fp_successors(uint32_t w, int action, uint32_t* out) {
    std::vector<uint32_t> succ;
    if (!successors(state_of(w), last_of(w), (Action)action, succ)) return -1;
    for (uint32_t i = 0; i < succ.size(); i++) out[i] = succ[i];
    return (int)succ.size();
}

// Every run from every initial state (last = None): runs, of them ended by a finished attempt / the device-wide replay / the
// finish=bucket failure, violations (a state visited twice, an action whose precondition does not hold), the most attempts of a run,
// the least 1 + one-way transitions - attempts of a run, the longest run in steps
void fp_walk_all(int64_t* out) {
    Walk w;
    for (uint32_t s = 0; s < N_STATES; s++) w.from(s, 0, 0);
    out[0] = (int64_t)w.runs; out[1] = (int64_t)w.done; out[2] = (int64_t)w.replay; out[3] = (int64_t)w.fail; out[4] = (int64_t)w.bad;
    out[5] = w.most_attempts; out[6] = w.least_slack; out[7] = (int64_t)w.longest;
}

}  // extern "C"
