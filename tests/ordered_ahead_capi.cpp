// C entry points over the decisions of sylph_amd/host/ordered_ahead.hpp — the very header cmd_contain.cpp prepares its samples
// ahead with — for tests/test_ordered_ahead.py (ctypes).
#include <cstdint>

#include "../sylph_amd/host/ordered_ahead.hpp"

using namespace sylph_host::ordered_ahead;

extern "C" {

uint64_t oa_ahead_limit(uint64_t n_workers) { return ahead_limit(n_workers); }
uint64_t oa_pipeline_depth(uint64_t limit) { return pipeline_depth(limit); }
int oa_gate_open(uint64_t j, uint64_t released, uint64_t limit, int cancelled) { return gate_open(j, released, limit, cancelled != 0); }
int oa_must_wait(uint64_t outstanding, uint64_t submitted, uint64_t done) { return must_wait(outstanding, submitted, done); }

}  // extern "C"
