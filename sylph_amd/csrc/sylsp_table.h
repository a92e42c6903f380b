// sylsp_table.h — a sample's (k-mer, count) table made on the device from the entries of a .sylsp file (sylsp.hip); internal.
#pragma once
#include "common.h"

struct sylph_table {
    sylph_ctx* ctx = nullptr;
    sylph::DevBuf kmers, counts;      // the table: n entries, k-mers strictly ascending
    uint64_t n = 0;
    int was_ascending = 1;            // the entries came strictly ascending: the table is the unpacked arrays, nothing was sorted
};

namespace sylph {
// sylph_table_from_entries without the ABI's wrapping (throws); pipeline.hip calls the extern "C" function
sylph_table* table_from_entries_impl(sylph_ctx* ctx, const void* entries, uint64_t n_entries, int mem);
}  // namespace sylph
