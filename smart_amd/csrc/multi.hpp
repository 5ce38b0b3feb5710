// multi.hpp — the arguments of hor_multi_scan (k_horm.hip): several Horspool patterns of one length counted in ONE
// pass over the text.  Host-only types; included by k_horm.hip and by api.cpp, which queues the launches that share a pass.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sg {

constexpr int kMultiMax = 8;  // patterns per pass

// What the patterns of a pass have in common — text, range, length, back halo — and, per pattern, its blob (pattern +
// u16 tab[256], as launch_hor reads it) and its result slot.  The two arrays are only ever indexed with compile-time
// constants: entries np .. kMultiMax-1 are not read.
struct MultiArgs {
    const uint8_t* text;        // device pointer to text byte 0
    uint64_t s_begin, s_end;    // start positions to count, as ScanArgs
    uint32_t m;                 // pattern length
    uint32_t halo;              // back halo H = min(m-1, kHaloMax)
    uint32_t np;                // patterns in this pass, 1 <= np <= kMultiMax
    const uint8_t* blob[kMultiMax];
    unsigned long long* count[kMultiMax];
};

// The launcher of k_horm.hip, reached through a pointer that the unit's own static initialiser sets: api.cpp holds
// the pointer (null: no launch is ever queued), so a program that includes api.cpp without k_horm.hip still links.
extern hipError_t (*g_hor_multi)(const MultiArgs& a, int num_cus, hipStream_t stream);

}  // namespace sg
