// interleave_plan.h — the bookkeeping of an INTERLEAVED paired read file (mate 1, mate 2, mate 1, ...), free of HIP: which records of
// such a file are pairs, where a window of it is cut, which records the running mean of the read lengths walks over, what a record's id
// is and when two ids are those of mates.  The mate-check kernels (read_text.h mates_kernel, launched by fastq.hip and fasta.hip)
// include this header, and so do the host's roads (host/sample_feed.cpp, host/feed.cpp): there is one spelling of the rule.
// tests/test_interleave_plan.py compiles the same header with g++ (tests/interleave_plan_capi.cpp) and holds it against a numpy
// restatement; tests/interleave_plan_sanitize_main.cpp walks the same cases under AddressSanitizer and UBSan.
//
// The meaning of `--interleaved F` is `-1 A -2 B`, A = records 0, 2, 4, ... of F and B = records 1, 3, 5, ...: pair i is records 2 i and
// 2 i + 1, a last record without a mate is dropped (the lock-step readers drop a surplus mate-1 record: sketch.rs:813-815), and the mean
// read length runs over the mate-1 records, the even ones (sketch.rs:824-826).
//
// The id of a record is its header line without the leading '@' / '>' up to, not including, the first space or tab; a '\r' or the
// line end ends it too.  Records 2 i and 2 i + 1 are mates if their ids are equal, or if the first ends in "/1", the second in "/2"
// and everything in front is equal.  Nothing else pairs: "SRR1.1" / "SRR1.2" are two spots.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SY_IL_HD __host__ __device__ __forceinline__
#else
#define SY_IL_HD inline
#endif

namespace sylph {
namespace interleave_plan {

// ---- records and pairs ---------------------------------------------------------------------------------------------------------------
SY_IL_HD uint64_t pairs_of(uint64_t n_records) { return n_records / 2; }
// the first record that belongs to no pair of these n records (always even): a window's text is kept from where it begins
SY_IL_HD uint64_t kept_record(uint64_t n_records) { return 2 * (n_records / 2); }
// the running mean walks over mate 1 of every pair: record mean_record(i), i = 0 .. pairs_of(n) - 1
constexpr uint64_t MEAN_STRIDE = 2;
SY_IL_HD uint64_t mean_record(uint64_t pair) { return MEAN_STRIDE * pair; }
// the record of a pair's mate (0 or 1)
SY_IL_HD uint64_t record_of(uint64_t pair, uint32_t mate) { return 2 * pair + mate; }

// ---- ids and mates -------------------------------------------------------------------------------------------------------------------
SY_IL_HD bool is_id_end(uint8_t c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }
// header: the n bytes of a header line behind its '@' / '>' (with or without its line end) -> the length of the id
SY_IL_HD uint64_t id_len(const uint8_t* header, uint64_t n) {
    uint64_t l = 0;
    while (l < n && !is_id_end(header[l])) l++;
    return l;
}
// a, b: the ids of records 2 i and 2 i + 1 (la, lb bytes)
SY_IL_HD bool mates(const uint8_t* a, uint64_t la, const uint8_t* b, uint64_t lb) {
    if (la != lb) return false;
    uint64_t same = 0;
    while (same < la && a[same] == b[same]) same++;
    if (same == la) return true;
    return la >= 2 && same == la - 1 && a[la - 2] == '/' && a[la - 1] == '1' && b[la - 1] == '2';
}

// ---- the same rule, a group of lanes at a time ------------------------------------------------------------------------------------------
// The kernel gives every pair a group of GROUP_LANES lanes and walks both headers GROUP_LANES bytes per step, lane l at byte
// base + l of each: one coalesced read per header and step, no byte read twice, and nothing read behind the step in which an id ends.
// A byte behind the end of a header reads as a space (byte_at), so a header of 0 bytes ends its id in step 0 and one longer than
// the group's stride takes more steps.  Per step the group's lanes vote four masks (bit l = lane l):
//   end_a, end_b   the lane's byte of header a / b ends an id
//   differ         the two bytes differ
//   slash12        a's byte is '1', b's is '2' and a's byte in front of it is '/'   (the byte in front of lane 0: the last of the step before)
// and every lane of the group advances the same MateScan with them.  done(): no further step can change the verdict.
constexpr uint32_t GROUP_LANES = 32;
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t MAX_HEADER = 1u << 30;                // a longer header is read as this long (positions stay 32-bit)
SY_IL_HD uint32_t header_bytes(uint64_t n) { return n < MAX_HEADER ? (uint32_t)n : MAX_HEADER; }
SY_IL_HD uint8_t byte_at(const uint8_t* header, uint32_t n, uint32_t x) { return x < n ? header[x] : (uint8_t)' '; }
SY_IL_HD bool lane_slash12(uint8_t a, uint8_t b, uint8_t a_front, uint32_t x) { return x >= 1 && a == '1' && b == '2' && a_front == '/'; }
SY_IL_HD uint32_t lowest_bit(uint32_t m) { return (uint32_t)__builtin_ctz(m); }

struct MateScan {
    uint32_t la = NONE, lb = NONE;        // the ids' lengths once their ends have been seen
    uint32_t differ_at = NONE;            // the one position in front of both ends at which the ids differ
    bool slash = false, fail = false;     // that position is a "/1" against a "/2"; more than one such position
    SY_IL_HD void step(uint32_t base, uint32_t end_a, uint32_t end_b, uint32_t differ, uint32_t slash12) {
        if (la == NONE && end_a) la = base + lowest_bit(end_a);
        if (lb == NONE && end_b) lb = base + lowest_bit(end_b);
        const uint32_t limit = la < lb ? la : lb;                        // positions in front of it lie in both ids
        const uint32_t live = limit >= base + GROUP_LANES ? ~0u : (limit <= base ? 0u : (1u << (limit - base)) - 1u);
        differ &= live;
        if (!differ) return;
        if (differ_at != NONE || (differ & (differ - 1u))) { fail = true; return; }
        const uint32_t l = lowest_bit(differ);
        differ_at = base + l;
        slash = (slash12 >> l & 1u) != 0;
        if (!slash) fail = true;                                         // only a "/1" against a "/2" may differ
    }
    SY_IL_HD bool done() const { return fail || la != NONE || lb != NONE; }
    // (an id that ends where the other goes on: la != lb, one of them still NONE)
    SY_IL_HD bool verdict() const { return !fail && la != NONE && la == lb && (differ_at == NONE || (slash && differ_at + 1 == la)); }
};

}  // namespace interleave_plan
}  // namespace sylph
