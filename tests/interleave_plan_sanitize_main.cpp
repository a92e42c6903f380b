// A stand-alone program over sylph_amd/csrc/interleave_plan.h (through tests/interleave_plan_capi.cpp), to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_interleave_plan.py does both).  It walks the named cases of the mate
// rule (equal ids, /1 /2, /2 /1, .1 .2, x/1 y/2, /1 /2 alone, empty ids, space and tab, a header that is all id, lengths 0, 1 and
// 2, '\r') and a few thousand generated header pairs of 0 .. 100 bytes, every header in a heap block of exactly its size so that a
// read past its end is reported, and holds the kernel's group walk against the sequential rule; then pairs_of / kept_record at
// 0 .. 5 and near 2^32 and 2^64.  Exits 0 and prints a line; a mismatch or a sanitizer report fails.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

extern "C" {
uint64_t ip_pairs_of(uint64_t n);
uint64_t ip_kept_record(uint64_t n);
uint64_t ip_mean_record(uint64_t pair);
uint64_t ip_id_len(const uint8_t* h, uint64_t n);
int ip_mates(const uint8_t* a, uint64_t la, const uint8_t* b, uint64_t lb);
int ip_header_mates(const uint8_t* ha, uint64_t na, const uint8_t* hb, uint64_t nb);
int ip_group_mates(const uint8_t* ha, uint64_t na, const uint8_t* hb, uint64_t nb, uint32_t* steps);
uint32_t ip_group_lanes();
}

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return state;
}

struct Exact {                                           // a header in a block of exactly its size
    uint8_t* p;
    uint64_t n;
    explicit Exact(const std::string& s) : p(new uint8_t[s.size()]), n(s.size()) { memcpy(p, s.data(), n); }
    Exact(const Exact&) = delete;
    ~Exact() { delete[] p; }
};

static int check(const std::string& a, const std::string& b, int want, uint64_t& yes, uint64_t& multi_step) {
    Exact ea(a), eb(b);
    uint32_t steps = 0;
    const int seq = ip_header_mates(ea.p, ea.n, eb.p, eb.n), grp = ip_group_mates(ea.p, ea.n, eb.p, eb.n, &steps);
    if (seq != grp || (want >= 0 && seq != want)) {
        fprintf(stderr, "'%s' / '%s': sequential %d, group walk %d, wanted %d\n", a.c_str(), b.c_str(), seq, grp, want);
        return 1;
    }
    yes += seq;
    multi_step += steps > 1;
    return 0;
}

int main() {
    uint64_t cases = 0, yes = 0, multi = 0;
    struct Named { const char *a, *b; int want; };
    const Named named[] = {
        {"read7", "read7", 1}, {"read7/1", "read7/2", 1}, {"read7/2", "read7/1", 0}, {"SRR1.1", "SRR1.2", 0}, {"x/1", "y/2", 0},
        {"/1", "/2", 1}, {"", "", 1}, {"", "a", 0}, {"a", "", 0}, {"1", "2", 0}, {"a", "a", 1}, {"a", "b", 0}, {"ab", "ab", 1},
        {"a1", "a2", 0}, {"r desc one", "r desc two", 1}, {"r\tdesc", "r other", 1}, {"r 1", "s 1", 0}, {"r/1 x", "r/2\ty", 1},
        {"r\r", "r", 1}, {"r/1\r\n", "r/2\r\n", 1}, {"r\n", "r x\n", 1}, {"r/1x", "r/2x", 0}, {"r/1", "r/1", 1}, {"r/2", "r/2", 1},
        {"r/1", "r/3", 0}, {"r/1", "r/22", 0}, {" x", " y", 1}, {"ra", "r", 0},
    };
    for (const Named& c : named) { if (check(c.a, c.b, c.want, yes, multi)) return 2; cases++; }
    const uint32_t G = ip_group_lanes();
    const char alphabet[] = "ACGT01219/._: \t";
    for (int i = 0; i < 6000; i++) {
        const uint32_t kind = (uint32_t)(rnd64() % 6);
        uint64_t la = rnd64() % 101;
        const uint64_t edges[8] = {0, 1, 2, G - 1, G, G + 1, 2 * G, 2 * G + 1};
        if (i % 7 == 0) la = edges[rnd64() % 8];
        std::string a, b;
        for (uint64_t j = 0; j < la; j++) a += alphabet[rnd64() % (sizeof(alphabet) - 1)];
        b = a;
        if (kind == 1 && !b.empty()) b[rnd64() % b.size()] = 'Z';                         // one byte differs anywhere
        if (kind == 2) { const uint64_t at = la ? rnd64() % la : 0; a.insert(at, "/1"); b.insert(at, "/2"); }
        if (kind == 3) { a += "/1"; b += "/2"; }
        if (kind == 4) { a += "/1 left"; b += "/2\tright"; }
        if (kind == 5) b += alphabet[rnd64() % (sizeof(alphabet) - 1)];                   // one id goes on
        if (check(a, b, -1, yes, multi)) return 3;
        cases++;
    }
    // every length of a long id around the group's stride: all id, no end byte in the header
    for (uint32_t n = 0; n <= 3 * G + 1; n++) {
        const std::string id(n, 'q');
        if (check(id, id, 1, yes, multi) || check(id + "/1", id + "/2", 1, yes, multi) || check(id + "/1", id + "/1 ", 1, yes, multi) ||
            check(id + "a", id + "b", 0, yes, multi))
            return 4;
        cases += 4;
    }
    for (uint64_t n : {0ull, 1ull, 2ull, 3ull, 4ull, 5ull, (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 1, ~0ull - 1, ~0ull}) {
        if (ip_pairs_of(n) != n / 2 || ip_kept_record(n) != n - n % 2 || ip_kept_record(n) != 2 * ip_pairs_of(n)) return 5;
        if (n < (1ull << 62) && ip_mean_record(n) != 2 * n) return 6;
    }
    const uint8_t none = 0;
    if (ip_id_len(&none, 0) != 0 || ip_mates(&none, 0, &none, 0) != 1) return 7;
    printf("interleave plan sanitize run ok: %llu cases, %llu mates, %llu of more than one step\n", (unsigned long long)cases,
           (unsigned long long)yes, (unsigned long long)multi);
    return 0;
}
