// A stand-alone program over sylph_amd/csrc/fasta_reads_plan.h (through tests/fasta_reads_plan_capi.cpp), to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_fasta_reads_plan.py does both): it makes its own files of records —
// lengths 0, 1, 15, 16, 17, 4095, 4096, 4097 and 20,000, runs of one-base records, empty records in rows — gathers single and paired
// batches of every sub-range shape with the model of fa_batch_kernel and compares them with a plain concatenation, and holds the window
// rule at every cut of a small text against a count of its own.  Exits 0 and prints a line; a mismatch or a sanitizer report fails the run.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" {
uint64_t fr_batch_total(const uint64_t* ro_a, const uint64_t* ro_b, uint64_t first, uint64_t n_items);
uint64_t fr_batch_map(const uint64_t* ro_a, const uint64_t* ro_b, uint64_t first, uint64_t n_items, uint8_t* mate, uint64_t* rec, uint64_t* src,
                      uint32_t* max_pieces);
int fr_batch_gather(const uint8_t* ja, uint64_t n_a, const uint64_t* ro_a, const uint8_t* jb, uint64_t n_b, const uint64_t* ro_b, uint64_t first,
                    uint64_t n_items, uint8_t* out, uint64_t cap);
int fr_window(const uint8_t* text, uint64_t n, int final, uint64_t* records, uint64_t* consumed);
}

namespace {
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }

struct File {
    std::vector<uint64_t> off{0};
    std::vector<uint8_t> bases;
    void add(uint64_t len) {
        for (uint64_t i = 0; i < len; i++) bases.push_back("ACGTN"[rnd() % 5]);
        off.push_back(bases.size());
    }
};
File make_file(int variant) {
    File f;
    const uint64_t lens[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 20000, 0, 0, 0, 33};
    for (int i = 0; i < 40; i++) f.add(1);
    for (const uint64_t l : lens) f.add(variant ? l + (l ? 1 : 0) : l);
    for (int i = 0; i < 30; i++) f.add(rnd() % 200);
    for (int i = 0; i < 20; i++) f.add(0);
    f.add(variant ? 7 : 300);
    return f;
}
int check_batch(const File& a, const File* b, uint64_t first, uint64_t n_items) {
    std::vector<uint8_t> want;
    for (uint64_t i = first; i < first + n_items; i++) {
        want.insert(want.end(), a.bases.begin() + a.off[i], a.bases.begin() + a.off[i + 1]);
        if (b) want.insert(want.end(), b->bases.begin() + b->off[i], b->bases.begin() + b->off[i + 1]);
    }
    const uint64_t total = fr_batch_total(a.off.data(), b ? b->off.data() : nullptr, first, n_items);
    if (total != want.size()) return 10;
    const uint64_t cap = (total + 15) / 16 * 16;
    uint8_t* out = (uint8_t*)aligned_alloc(16, cap + 16);       // exactly what the stores may touch (+ 16 so that cap == 0 allocates)
    memset(out, 0xAB, cap + 16);
    const int rc = fr_batch_gather(a.bases.data(), a.bases.size(), a.off.data(), b ? b->bases.data() : nullptr, b ? b->bases.size() : 0,
                                   b ? b->off.data() : nullptr, first, n_items, out, cap);
    int bad = rc ? 11 : 0;
    if (!bad && total && memcmp(out, want.data(), total)) bad = 12;
    for (uint64_t i = total; !bad && i < cap; i++) if (out[i] != 0) bad = 13;          // the last lane's surplus bytes are zeros
    free(out);
    if (bad) return bad;
    std::vector<uint8_t> mate(total + 1);
    std::vector<uint64_t> rec(total + 1), src(total + 1);
    uint32_t pieces = 0;
    if (fr_batch_map(a.off.data(), b ? b->off.data() : nullptr, first, n_items, mate.data(), rec.data(), src.data(), &pieces)) return 14;
    if (pieces > 16) return 15;
    for (uint64_t q = 0; q < total; q++) {
        const File& f = mate[q] ? *b : a;
        if (rec[q] < first || rec[q] >= first + n_items || src[q] < f.off[rec[q]] || src[q] >= f.off[rec[q] + 1] || f.bases[src[q]] != want[q]) return 16;
    }
    return 0;
}
}  // namespace

int main() {
    const File a = make_file(0), b = make_file(1);
    const uint64_t n = a.off.size() - 1;
    uint64_t batches = 0;
    const uint64_t ranges[][2] = {{0, n}, {0, 0}, {0, 1}, {3, 40}, {40, 9}, {39, 12}, {48, 1}, {n - 21, 21}, {n - 1, 1}, {n, 0}, {17, n - 17}};
    for (const auto& r : ranges)
        for (int paired = 0; paired < 2; paired++) {
            const int rc = check_batch(a, paired ? &b : nullptr, r[0], r[1]);
            if (rc) { fprintf(stderr, "batch [%llu, +%llu) paired=%d: %d\n", (unsigned long long)r[0], (unsigned long long)r[1], paired, rc); return rc; }
            batches++;
        }
    const std::string text = ">r1 first\nACGT\nAC\n>r2\n>r3\r\nGGCC\r\n\r\nTT\r\n>r4 > @\nA\n>r5\nACGTACGTACGTACGTACGTAC\nGT\n>last\nTTTT\r";
    uint64_t cuts = 0;
    for (uint64_t cut = 0; cut <= text.size(); cut++)
        for (int final = 0; final < 2; final++) {
            uint64_t headers = 0, last_at = 0, records = 0, consumed = 0;
            for (uint64_t i = 0; i < cut; i++) if (text[i] == '>' && (i == 0 || text[i - 1] == '\n')) { headers++; last_at = i; }
            const int rc = fr_window((const uint8_t*)text.data(), cut, final, &records, &consumed);
            const bool refused = cut == 0 && final;
            if ((rc != 0) != refused) return 20;
            if (rc) continue;
            const uint64_t want_rec = final ? headers : (headers ? headers - 1 : 0), want_used = final ? cut : (headers >= 2 ? last_at : 0);
            if (records != want_rec || consumed != want_used) return 21;
            cuts++;
        }
    printf("fasta reads sanitize run ok: %llu batches, %llu windows\n", (unsigned long long)batches, (unsigned long long)cuts);
    return 0;
}
