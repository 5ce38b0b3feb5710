// multi.hpp — the arguments of hor_multi_scan (k_horm.hip): several Horspool patterns of one length counted in ONE
// pass over the text.  Included by k_horm.hip and by api.cpp, which queues the launches that share a pass.
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

// The skip table that the patterns of a pass share (Wu-Manber, blocks of two bytes): one entry per slot, indexed by the
// LAST TWO bytes of a window.  Low half: how far the window end may move — the least m-2-i over every pattern P of the
// pass and every position i <= m-3 whose gram (P[i], P[i+1]) falls into the slot; m-1 where no gram does (the next
// window may still overlap this one by its last byte).  High half: bit g for every pattern g whose LAST gram
// (P[m-2], P[m-1]) falls into the slot — the windows that are compared.  Grams that collide in a slot only lower a
// shift or add a comparison, so any slot function counts right.  The rule is written once, for the kernel and for
// the host program that checks it (tests/coalesce_gram_check.cpp).
constexpr uint32_t kGramSlots = 2048;  // 8 KB of LDS: with the tile and the tails, five workgroups per CU stay below 160 KB
constexpr uint32_t kGramCap = 64;      // a lane owns 64 window ends: a longer shift leaves its segment just the same

// the slot of the gram (prev, last).  Injective for alphabets up to 37 symbols; byte pairs spread over all slots
__host__ __device__ inline uint32_t gram_slot(uint32_t prev, uint32_t last) { return (prev * 37u + last) & (kGramSlots - 1u); }
// the shift of a slot no gram reaches
__host__ __device__ inline uint32_t gram_default(uint32_t m) { return m - 1u < kGramCap ? m - 1u : kGramCap; }
// the shift the gram at pattern position i allows, 0 <= i <= m - 3: at least 1
__host__ __device__ inline uint32_t gram_shift(uint32_t m, uint32_t i) { return m - 2u - i; }
// the first position whose gram is entered: those before it allow gram_default(m) or more
__host__ __device__ inline uint32_t gram_first(uint32_t m) { return m - 1u > kGramCap ? m - 1u - kGramCap : 0u; }
// an entry's halves
__host__ __device__ inline uint32_t gram_entry_shift(uint32_t ent) { return ent & 0xFFFFu; }
__host__ __device__ inline uint32_t gram_entry_patterns(uint32_t ent) { return ent >> 16; }
__host__ __device__ inline uint32_t gram_entry_pattern_bit(uint32_t g) { return 0x10000u << g; }

// The launcher of k_horm.hip, reached through a pointer that the unit's own static initialiser sets: api.cpp holds
// the pointer (null: no launch is ever queued), so a program that includes api.cpp without k_horm.hip still links.
extern hipError_t (*g_hor_multi)(const MultiArgs& a, int num_cus, hipStream_t stream);

}  // namespace sg
