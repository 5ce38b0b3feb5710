// multi.hpp — the arguments of hor_multi_scan (k_horm.hip): several Horspool patterns of one length counted in ONE
// pass over the text.  Included by k_horm.hip and by api.cpp, which queues the launches that share a pass.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace sg {

constexpr int kMultiMax = 32;  // the widest pass smartgpu_coalesce_wide sets (api.cpp); a pass takes up to kPassMax patterns
constexpr int kPassMax = 96;   // patterns per pass at the most; what a length's rows leave room for is pass_width(m) below

// The end of a pattern as a launch carries it BY VALUE: the bytes from position gram_first(m) (below) to m - 1 — every
// gram the skip table enters and the at most 17 bytes a lane compares in LDS — at the front of a row, zeros behind
// them.  At most kGramCap + 1 = 65 bytes; the row is padded to a multiple of 16.  The plan keeps its row on the host
// from smartgpu_plan_create on, the launch queue copies it, and the kernel builds the table from the rows in its
// arguments: no workgroup reads a pattern from memory before its first tile is on the way.
constexpr uint32_t kTailRow = 80;  // the longest row; a pass stores its rows at tail_stride(m), their own length

// What the patterns of a pass have in common — text, range, length, back halo — and one byte area that holds, for the
// W = pass_width(m) patterns a pass of this length can take: u64 blob[W] (pattern + u16 tab[256], as launch_hor reads
// it: read only where a window is completed in memory, m - 1 > halo) | u64 count[W] (the result slots) | W rows at
// stride tail_stride(m).  Where the parts lie depends on m alone, not on np; entries np .. W-1 are not read.  The
// kernel reads the pointers from the area AS NUMBERS (multi_blob, multi_count).
constexpr uint32_t kMultiArea = 4032;
struct alignas(16) MultiArgs {
    const uint8_t* text;        // device pointer to text byte 0
    uint64_t s_begin, s_end;    // start positions to count, as ScanArgs
    uint32_t m;                 // pattern length
    uint32_t halo;              // back halo H = min(m-1, kHaloMax)
    uint32_t np;                // patterns in this pass, 1 <= np <= width
    uint32_t width;             // pass_width(m); long_width(m) in a long pass (below)
    uint32_t stride;            // tail_stride(m)
    uint32_t reserved;          // the area's layout: kMultiByValue or kMultiLong (the area starts at a multiple of 16: a thread copies 16 bytes of rows at a time)
    uint8_t area[kMultiArea];
};
// the kernel takes MultiArgs and two more arguments, a u64 and a u32, by value: HIP passes at most 4096 bytes
static_assert(sizeof(MultiArgs) + 8 + 4 <= 4096, "MultiArgs, tile_first and ntiles fit the kernel argument segment");
static_assert(offsetof(MultiArgs, area) % 16 == 0 && sizeof(MultiArgs) == offsetof(MultiArgs, area) + kMultiArea, "the area is 16-byte aligned and ends the arguments");

// The skip table that the patterns of a pass share (Wu-Manber, blocks of two bytes): ONE BYTE per slot, indexed by the
// LAST TWO bytes of a window.  Bits 0-6: how far the window end may move — the least m-2-i over every pattern P of the
// pass and every position i <= m-3 whose gram (P[i], P[i+1]) falls into the slot; m-1 where no gram does (the next
// window may still overlap this one by its last byte); at most kGramCap = 64.  Bit 7 (kGramHit): the LAST gram
// (P[m-2], P[m-1]) of some pattern of the pass falls into the slot.  A window that ends in such a slot follows the
// chain of its gram's BUCKET (gram_bucket: kGramBuckets heads, a link per pattern) and is compared, whole, with every
// pattern on it.  Grams that collide in a slot only lower a shift, and patterns that share a bucket only add a
// comparison, so any slot and any bucket function counts right.  The rule is written once, for the kernel and for the
// host program that checks it (tests/coalesce_pass_check.cpp).
// 16384 byte slots take the 16 KB of LDS that 4096 u32 slots took.  The slot function is exact on symbols below 128, so
// on such a text a slot hit is a gram hit and a shift is lowered only by a gram of the pass itself: a walk of the text
// takes fewer steps with 84 patterns in these slots than with 32 in the 4096 (profiles/coalesce/RESULTS.md).
constexpr uint32_t kGramSlots = 16384;
constexpr uint32_t kGramCap = 64;      // a lane owns 64 window ends: a longer shift leaves its segment just the same
constexpr uint32_t kGramHit = 0x80;    // a byte entry's bit 7
constexpr uint32_t kGramBuckets = 512;

// The slot of the gram (prev, last): (f(prev) + last) mod kGramSlots, so that slot and prev determine last.  Injective
// on symbols below 128 (128 prev + last); a prev of 128 or more is folded 85 slots away from prev - 128, so that a text
// of both halves of the byte range does not put (prev, last) and (prev - 128, last) into one slot.
__host__ __device__ inline uint32_t gram_slot(uint32_t prev, uint32_t last) { return (prev * 128u + (prev >> 7) * 85u + last) & (kGramSlots - 1u); }
// the bucket of the gram: the top bits of a multiplicative hash of its slot (grams of one slot share a bucket)
__host__ __device__ inline uint32_t gram_bucket(uint32_t prev, uint32_t last) { return (gram_slot(prev, last) * 0x9E3779B1u) >> 23; }
static_assert(kGramBuckets == 1u << (32 - 23), "gram_bucket keeps the top nine bits");
// a byte entry's parts
__host__ __device__ inline uint32_t gram_byte_shift(uint32_t b) { return b & (kGramHit - 1u); }
__host__ __device__ inline uint32_t gram_byte_hit(uint32_t b) { return b & kGramHit; }
// the shift of a slot no gram reaches
__host__ __device__ constexpr uint32_t gram_default(uint32_t m) { return m - 1u < kGramCap ? m - 1u : kGramCap; }
// the shift the gram at pattern position i allows, 0 <= i <= m - 3: at least 1
__host__ __device__ constexpr uint32_t gram_shift(uint32_t m, uint32_t i) { return m - 2u - i; }
// the first position whose gram is entered: those before it allow gram_default(m) or more
__host__ __device__ constexpr uint32_t gram_first(uint32_t m) { return m - 1u > kGramCap ? m - 1u - kGramCap : 0u; }
static_assert(kGramCap < kGramHit, "a shift fits the seven bits below the hit bit");

// The FORMER entry, a u32 per slot: the shift in byte 0, eight class bits in byte 2, a tag of the last gram's first byte
// in bytes 1 and 3.  hor_multi_scan no longer uses these; they are kept, self-consistent, for the committed host checks
// (tests/coalesce_gram_check.cpp, coalesce_tail_check.cpp, coalesce_wide_check.cpp), which build u32 tables with them.
__host__ __device__ inline uint32_t gram_entry_shift(uint32_t ent) { return ent & 0xFFu; }
__host__ __device__ inline uint32_t gram_entry_patterns(uint32_t ent) { return (ent >> 16) & 0xFFu; }
__host__ __device__ inline uint32_t gram_entry_pattern_bit(uint32_t g) { return 0x10000u << g; }  // g < 8
__host__ __device__ inline uint32_t gram_entry_class_bit(uint32_t g) { return gram_entry_pattern_bit(g & 7u); }  // g < kMultiMax
constexpr uint32_t kGramClasses = 8;  // the patterns of class c: c, c + kGramClasses, ... below np
__host__ __device__ inline uint32_t gram_entry_tag(uint32_t prev) { return (prev << 8) | ((prev ^ 0xFFu) << 24); }
__host__ __device__ inline uint32_t gram_entry_hit(uint32_t ent, uint32_t prev) { return (gram_entry_tag(prev) & ~ent) == 0 ? gram_entry_patterns(ent) : 0u; }


// a row: how many bytes it holds, the fill rule, and the byte at pattern position i, gram_first(m) <= i <= m - 1
__host__ __device__ constexpr uint32_t tail_stored(uint32_t m) { return m - gram_first(m); }
static_assert(kGramCap + 1 <= kTailRow && kTailRow % 16 == 0, "a row holds kGramCap grams and is padded to 16 bytes");
__host__ __device__ inline void tail_fill(uint8_t* row, const uint8_t* P, uint32_t m)
{
    const uint32_t first = gram_first(m), n = tail_stored(m);
    for (uint32_t j = 0; j < kTailRow; ++j) row[j] = j < n ? P[first + j] : (uint8_t)0;
}
// (a row of any stride: what is stored lies at its front)
__host__ __device__ inline uint32_t tail_at(const uint8_t* row, uint32_t m, uint32_t i) { return row[(int32_t)i - (int32_t)gram_first(m)]; }
// the gram at pattern positions i and i + 1 in ONE read of two bytes (they are neighbours in the row, at any
// alignment): position i in the low byte.  gram_first(m) <= i <= m - 2
__host__ __device__ inline uint32_t tail_gram_at(const uint8_t* row, uint32_t m, uint32_t i)
{
    uint16_t two;
    __builtin_memcpy(&two, row + ((int32_t)i - (int32_t)gram_first(m)), 2);
    return two;
}

// A pass stores a row at its own length, rounded to 16, and takes as many patterns as the area has room for: two
// pointers and a row each.  96 up to m = 16, 84 up to m = 32, 63 up to m = 48, 50 up to m = 64, 42 beyond.
__host__ __device__ constexpr uint32_t tail_stride(uint32_t m) { return (tail_stored(m) + 15u) & ~15u; }
__host__ __device__ constexpr uint32_t pass_width(uint32_t m)
{
    return kMultiArea / (16u + tail_stride(m)) < (uint32_t)kPassMax ? kMultiArea / (16u + tail_stride(m)) : (uint32_t)kPassMax;
}
static_assert(tail_stride(3) == 16 && tail_stride(4096) == kTailRow && pass_width(16) == 96 && pass_width(17) == 84 && pass_width(32) == 84 &&
              pass_width(64) == 50 && pass_width(65) == 42 && pass_width(4096) == 42 && pass_width(65) >= (uint32_t)kMultiMax,
              "every length has room for the 32 patterns smartgpu_coalesce_wide may ask for");
// where the parts of the area lie for a pass of length m (W = pass_width(m)); g < W
__host__ __device__ inline uint32_t multi_blob_at(uint32_t g) { return 8u * g; }
__host__ __device__ inline uint32_t multi_count_at(uint32_t W, uint32_t g) { return 8u * W + 8u * g; }
__host__ __device__ inline uint32_t multi_rows_at(uint32_t W) { return 16u * W; }
// put pattern g's pointers and its row (kTailRow bytes, as tail_fill leaves them) into a pass's arguments
inline void multi_set(MultiArgs& a, uint32_t g, const uint8_t* blob, unsigned long long* count, const uint8_t* row)
{
    __builtin_memcpy(a.area + multi_blob_at(g), &blob, 8);
    __builtin_memcpy(a.area + multi_count_at(a.width, g), &count, 8);
    __builtin_memcpy(a.area + multi_rows_at(a.width) + g * a.stride, row, a.stride);
}

// A LONG pass: more patterns than the arguments have room for by value.  The two pointers of a pattern are 16 bytes, so
// the area alone holds 252 pairs; the bytes of a row already lie in memory, at the front of every plan's blob
// ([pattern, kPatternBytes][tables]): a long pass carries u64 blob[LW] | u64 count[LW], LW = long_width(m), and NO rows,
// and the kernel's prologue reads each row from blob[g] + gram_first(m) — one dependent read per workgroup, before the
// first tile is asked for.  MultiArgs::reserved says which layout the area has; width is LW, so multi_blob_at and
// multi_count_at hold for both.  What bounds LW: the area, a thread per pattern, and the LDS of a workgroup when four
// are resident on a CU (40960 bytes each): the table, the heads, a link and a sum per pattern, the rows, the tile.
constexpr uint32_t kMultiByValue = 0, kMultiLong = 1;  // MultiArgs::reserved
constexpr uint32_t kMultiThreads = 256;                // hor_multi_scan's workgroup (k_horm.hip asserts it)
constexpr uint32_t kMultiTileLds = 16448;              // a tile with its halo: round64(48 + 16384 + 16)
constexpr uint32_t kMultiLdsBudget = 40960;
__host__ __device__ constexpr uint32_t round64(uint32_t x) { return (x + 63u) & ~63u; }
__host__ __device__ constexpr bool long_fits(uint32_t m, uint32_t np)
{
    return np * 16u <= kMultiArea && np + 4u <= kMultiThreads &&
           kGramSlots + 4u * kGramBuckets + 8u * np + round64(np * tail_stride(m)) + kMultiTileLds <= kMultiLdsBudget;
}
__host__ __device__ constexpr uint32_t long_search(uint32_t m)
{
    uint32_t np = 0;
    while (long_fits(m, np + 1u)) ++np;  // (what fits is monotone in np)
    return np;
}
// (the search runs when this is compiled, once per row stride: the queue asks for the width at every launch)
constexpr uint32_t kLongWidth[5] = {long_search(16), long_search(32), long_search(48), long_search(64), long_search(65)};
constexpr uint32_t long_width(uint32_t m) { return kLongWidth[tail_stride(m) / 16u - 1u]; }
static_assert(tail_stride(16) == 16 && tail_stride(32) == 32 && tail_stride(48) == 48 && tail_stride(64) == 64 && tail_stride(65) == 80, "one width per stride");
static_assert(long_width(3) == 252 && long_width(16) == 252 && long_width(17) == 152 && long_width(32) == 152 && long_width(33) == 108 &&
              long_width(48) == 108 && long_width(49) == 84 && long_width(64) == 84 && long_width(65) == 68 && long_width(4096) == 68,
              "the long width of every row stride");
static_assert(long_width(16) > pass_width(16) && long_width(32) > pass_width(32) && long_width(48) > pass_width(48) &&
              long_width(64) > pass_width(64) && long_width(65) > pass_width(65), "a long pass is wider than a by-value pass at every length");
constexpr uint32_t kLongMax = long_width(3);  // the most entries a key gathers
// The LDS of a long pass: u8 gram[kGramSlots] | u32 heads[kGramBuckets] | np rows | u32 next[np] | u32 sums[np] | pad to
// 64 | tile.  The rows come first so that they stay 16-byte aligned for any np; rounding the sum of rows, links and
// sums takes no more than long_fits allows (both are multiples of 64, and this one rounds once).
__host__ __device__ constexpr uint32_t long_head(uint32_t np, uint32_t stride) { return kGramSlots + 4u * kGramBuckets + round64(np * (stride + 8u)); }
static_assert(long_head(252, 16) + kMultiTileLds <= kMultiLdsBudget && long_head(152, 32) + kMultiTileLds <= kMultiLdsBudget &&
              long_head(108, 48) + kMultiTileLds <= kMultiLdsBudget && long_head(84, 64) + kMultiTileLds <= kMultiLdsBudget &&
              long_head(68, 80) + kMultiTileLds <= kMultiLdsBudget, "the widest long pass of every row stride leaves four workgroups per CU resident");
// put pattern g's pointers into a long pass's arguments (a.width == long_width(a.m))
inline void multi_set_long(MultiArgs& a, uint32_t g, const uint8_t* blob, unsigned long long* count)
{
    __builtin_memcpy(a.area + multi_blob_at(g), &blob, 8);
    __builtin_memcpy(a.area + multi_count_at(a.width, g), &count, 8);
}

// The launcher of k_horm.hip, reached through a pointer that the unit's own static initialiser sets: api.cpp holds
// the pointer (null: no launch is ever queued), so a program that includes api.cpp without k_horm.hip still links.
extern hipError_t (*g_hor_multi)(const MultiArgs& a, int num_cus, hipStream_t stream);

}  // namespace sg
