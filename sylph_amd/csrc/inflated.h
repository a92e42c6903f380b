// inflated.h — the handle behind sylph_inflated: a text decoded on the device, from gzip (inflate.hip) or bzip2 (bunzip2.hip).
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "common.h"

struct sylph_inflated {
    sylph_ctx* ctx = nullptr;
    void* buf = nullptr;                  // hipMalloc'ed: 256 bytes of zero padding, the text, 256 bytes of zero padding
    uint64_t n = 0;
    uint64_t n_members = 0, n_blocks = 0, n_candidates = 0, n_host_members = 0, n_redone = 0;
    std::vector<std::pair<uint64_t, uint64_t>> files;   // [begin, end) of every file's text in the whole text
    const uint8_t* text() const { return (const uint8_t*)buf + 256; }
};
