// multi.hpp — the arguments of hor_multi_scan (k_horm.hip): several Horspool patterns of one length counted in ONE
// pass over the text.  Included by k_horm.hip and by api.cpp, which queues the launches that share a pass.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sg {

constexpr int kMultiMax = 32;  // patterns per pass: four to each of the eight class bits of a skip-table entry (below)

// The end of a pattern as a launch carries it BY VALUE: the bytes from position gram_first(m) (below) to m - 1 — every
// gram the skip table enters and the at most 17 bytes a lane compares in LDS — at the front of a row, zeros behind
// them.  At most kGramCap + 1 = 65 bytes; the row is padded to a multiple of 16.  The plan keeps its row on the host
// from smartgpu_plan_create on, the launch queue copies it, and the kernel builds the tails and the table from the
// rows in its arguments: no workgroup reads a pattern from memory before its first tile is on the way.
constexpr uint32_t kTailRow = 80;

// What the patterns of a pass have in common — text, range, length, back halo — and, per pattern, its row (above), its
// blob (pattern + u16 tab[256], as launch_hor reads it: read only where a window is completed in memory, m - 1 > halo)
// and its result slot.  The two pointer arrays are only ever indexed with compile-time constants.  Entries
// np .. kMultiMax-1 are not read.
struct MultiArgs {
    const uint8_t* text;        // device pointer to text byte 0
    uint64_t s_begin, s_end;    // start positions to count, as ScanArgs
    uint32_t m;                 // pattern length
    uint32_t halo;              // back halo H = min(m-1, kHaloMax)
    uint32_t np;                // patterns in this pass, 1 <= np <= kMultiMax
    const uint8_t* blob[kMultiMax];
    unsigned long long* count[kMultiMax];
    uint8_t tail[kMultiMax][kTailRow];
};
// the kernel takes MultiArgs and two more arguments, a u64 and a u32, by value: HIP passes at most 4096 bytes
static_assert(sizeof(MultiArgs) + 8 + 4 <= 4096, "MultiArgs, tile_first and ntiles fit the kernel argument segment");

// The skip table that the patterns of a pass share (Wu-Manber, blocks of two bytes): one entry per slot, indexed by the
// LAST TWO bytes of a window.  Low half: how far the window end may move — the least m-2-i over every pattern P of the
// pass and every position i <= m-3 whose gram (P[i], P[i+1]) falls into the slot; m-1 where no gram does (the next
// window may still overlap this one by its last byte).  High half: bit g & 7 — the CLASS of pattern g — for every
// pattern g whose LAST gram (P[m-2], P[m-1]) falls into the slot: a window that ends in such a slot is compared with
// the patterns c, c + 8, c + 16, c + 24 below np of every class c whose bit is set.  A pass of at most eight has one
// pattern per class, and the bit names the pattern.  Grams that collide in a slot, and class mates that are not the
// pattern, only lower a shift or add a comparison (every comparison is a whole one), so any slot function counts right.  The rule is written once, for the kernel and for
// the host program that checks it (tests/coalesce_gram_check.cpp).
// 16 KB of LDS: with the tile and the tails of 32 patterns a workgroup takes 33.8 KB, and the four per CU that the pass
// runs with (k_horm.hip: horm_wgs) stay below 160 KB.  32 patterns of m = 32 enter 37 % of 2048 slots and 20 % of 4096:
// measured per pattern in a pass of 32, 0.0060 ms against 0.0063 at m = 32 and no slower at m = 16, 64, 256 or in a
// pass of eight (profiles/coalesce/RESULTS.md, "Up to 32 patterns in a pass")
constexpr uint32_t kGramSlots = 4096;
constexpr uint32_t kGramCap = 64;      // a lane owns 64 window ends: a longer shift leaves its segment just the same

// the slot of the gram (prev, last).  Injective for alphabets up to 37 symbols; byte pairs spread over all slots
__host__ __device__ inline uint32_t gram_slot(uint32_t prev, uint32_t last) { return (prev * 37u + last) & (kGramSlots - 1u); }
// the shift of a slot no gram reaches
__host__ __device__ inline uint32_t gram_default(uint32_t m) { return m - 1u < kGramCap ? m - 1u : kGramCap; }
// the shift the gram at pattern position i allows, 0 <= i <= m - 3: at least 1
__host__ __device__ inline uint32_t gram_shift(uint32_t m, uint32_t i) { return m - 2u - i; }
// the first position whose gram is entered: those before it allow gram_default(m) or more
__host__ __device__ inline uint32_t gram_first(uint32_t m) { return m - 1u > kGramCap ? m - 1u - kGramCap : 0u; }
// an entry's parts: the shift in byte 0 (at most kGramCap), the class bits in byte 2
__host__ __device__ inline uint32_t gram_entry_shift(uint32_t ent) { return ent & 0xFFu; }
__host__ __device__ inline uint32_t gram_entry_patterns(uint32_t ent) { return (ent >> 16) & 0xFFu; }
__host__ __device__ inline uint32_t gram_entry_pattern_bit(uint32_t g) { return 0x10000u << g; }  // g < 8
__host__ __device__ inline uint32_t gram_entry_class_bit(uint32_t g) { return gram_entry_pattern_bit(g & 7u); }  // g < kMultiMax
constexpr uint32_t kGramClasses = 8;  // the patterns of class c: c, c + kGramClasses, ... below np
// Bytes 1 and 3 tell a slot hit from a gram hit without a compare: a pattern ORs gram_entry_tag(P[m-2]) into its slot
// with its bit — `prev` in byte 1, its complement in byte 3 — and a window whose last two bytes fall into the slot is
// compared only if every bit of ITS tag is there.  Slot and prev determine last (the slot is 37 prev + last mod
// kGramSlots, and last < 256 <= kGramSlots), so with one last gram in a slot this asks for the gram itself; with
// several, bits of both kinds add up and more windows pass, never fewer.  An entry without a pattern has no tag bit:
// nothing passes.
__host__ __device__ inline uint32_t gram_entry_tag(uint32_t prev) { return (prev << 8) | ((prev ^ 0xFFu) << 24); }
__host__ __device__ inline uint32_t gram_entry_hit(uint32_t ent, uint32_t prev) { return (gram_entry_tag(prev) & ~ent) == 0 ? gram_entry_patterns(ent) : 0u; }


// a row: how many bytes it holds, the fill rule, and the byte at pattern position i, gram_first(m) <= i <= m - 1
__host__ __device__ inline uint32_t tail_stored(uint32_t m) { return m - gram_first(m); }
static_assert(kGramCap + 1 <= kTailRow && kTailRow % 16 == 0, "a row holds kGramCap grams and is padded to 16 bytes");
__host__ __device__ inline void tail_fill(uint8_t* row, const uint8_t* P, uint32_t m)
{
    const uint32_t first = gram_first(m), n = tail_stored(m);
    for (uint32_t j = 0; j < kTailRow; ++j) row[j] = j < n ? P[first + j] : (uint8_t)0;
}
__host__ __device__ inline uint32_t tail_at(const uint8_t* row, uint32_t m, uint32_t i) { return row[(int32_t)i - (int32_t)gram_first(m)]; }
// the gram at pattern positions i and i + 1 in ONE read of two bytes (they are neighbours in the row, at any
// alignment): position i in the low byte.  gram_first(m) <= i <= m - 2
__host__ __device__ inline uint32_t tail_gram_at(const uint8_t* row, uint32_t m, uint32_t i)
{
    uint16_t two;
    __builtin_memcpy(&two, row + ((int32_t)i - (int32_t)gram_first(m)), 2);
    return two;
}

// The launcher of k_horm.hip, reached through a pointer that the unit's own static initialiser sets: api.cpp holds
// the pointer (null: no launch is ever queued), so a program that includes api.cpp without k_horm.hip still links.
extern hipError_t (*g_hor_multi)(const MultiArgs& a, int num_cus, hipStream_t stream);

}  // namespace sg
