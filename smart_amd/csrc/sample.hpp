// sample.hpp — the SAMPLE of a text and the arguments of hor_sample_scan (k_hors.hip): host + device, shared by the
// kernel, by api.cpp (which owns a text's sample and queues the passes) and by the host check
// (tests/coalesce_sample_check.cpp).
//
// A Horspool shift of m - 1 bytes skips nothing on a GPU whose memory arrives in 128-byte lines: hor_multi_scan
// fetches every byte of the text to look at one in eight.  Which bytes a pass looks at can be decided when the text is
// CREATED (a text is never written again): next to a text lie the kSampleGram = 4 bytes at every kSampleStride = 28th
// position, n / 7 bytes in all.  sample[k] is the little-endian dword T[28k .. 28k + 4), for every k with
// 28k < n + 28; bytes past n come from the text's zeroed back pad.
//
// Why a pass over the sample alone counts exactly.  Let s be a window of m >= kSampleMinM = 31 bytes.  The first
// multiple of 28 at or after s is p = s + i with 0 <= i <= 27, and p + 3 <= s + 30 <= s + m - 1: the gram at p lies
// inside the window and equals P[i .. i + 4) when the window matches.  A pass enters, for each of its patterns, the
// grams at offsets i in [0, 28) ONLY, so a window is offered exactly once — through that one sample — even when it
// holds two samples or more (m >= 59).  A bit filter and chained buckets, both indexed by a hash of the gram, find the
// entries of a sample's gram; both may alias freely, because an entry is followed only when its stored gram EQUALS the
// sample's, and a window is counted only when T[s .. s + m) equals the whole pattern in memory.  The same pattern
// twice in a pass has two sets of entries and two counters.
#pragma once
#include "multi.hpp"

namespace sg {

constexpr uint32_t kSampleStride = 28;
constexpr uint32_t kSampleGram = 4;
constexpr uint32_t kSampleMinM = kSampleStride + kSampleGram - 1;  // 31: every window this long holds a sampled gram whole
static_assert(kSampleStride % 4 == 0 && kSampleGram == 4, "every sampled gram is an aligned dword of the text");

// the dwords of a text's sample, and the allocation: whole 16-byte quads (a lane of the scan loads one) and one more
__host__ __device__ constexpr uint64_t sample_count(uint64_t n) { return (n + 2 * kSampleStride - 1) / kSampleStride; }
__host__ __device__ constexpr uint64_t sample_alloc_dwords(uint64_t n) { return ((sample_count(n) + 3) & ~3ull) + 4; }
static_assert(sample_count(0) == 1 && sample_count(1) == 2 && sample_count(28) == 2 && sample_count(29) == 3, "k runs over 28k < n + 28");

// The pass.  hor_sample_scan takes hor_multi_scan's MultiArgs in both layouts (multi.hpp) with rows of its own: a
// by-value row holds the pattern's FIRST kSampleMinM bytes — every gram the pass enters — padded to kSampleRow; a long
// pass reads them from the front of the pattern's blob.  MultiArgs::stride is kSampleRow, ::width the widths below,
// ::halo is not used.
constexpr uint32_t kSampleRow = 32;
__host__ __device__ inline void sample_head_fill(uint8_t* row, const uint8_t* P, uint32_t m)
{
    for (uint32_t j = 0; j < kSampleRow; ++j) row[j] = j < m && j < kSampleMinM ? P[j] : (uint8_t)0;
}
// the gram at offset i of a row, 0 <= i < kSampleStride
__host__ __device__ inline uint32_t sample_row_gram(const uint8_t* row, uint32_t i)
{
    uint32_t g;
    __builtin_memcpy(&g, row + i, 4);
    return g;
}

// The filter: 2^19 bits indexed by a multiplicative hash of the gram.  A pass of 152 patterns enters 4256 grams: under
// one bit in a hundred is set, and on a text of 7-bit symbols about 1 % of the samples pass (the host check prints it).
constexpr uint32_t kSampleFilterBits = 19;
constexpr uint32_t kSampleFilterWords = 1u << (kSampleFilterBits - 5);
__host__ __device__ inline uint32_t sample_hash(uint32_t gram) { return (gram * 0x9E3779B1u) >> (32 - kSampleFilterBits); }
__host__ __device__ inline uint32_t sample_filter_word(uint32_t h) { return h >> 5; }
__host__ __device__ inline uint32_t sample_filter_bit(uint32_t h) { return 1u << (h & 31u); }
// The chains: the top 12 bits of the same hash choose one of 4096 heads (u32: LDS has no 16-bit exchange); an entry is
// the gram and a word of pattern j (8 bits), offset i (5 bits) and the next entry + 1 (16 bits; 0 ends the chain).
constexpr uint32_t kSampleBuckets = 4096;
__host__ __device__ inline uint32_t sample_bucket(uint32_t h) { return h >> (kSampleFilterBits - 12); }
struct SampleEntry { uint32_t gram, link; };
__host__ __device__ inline uint32_t sample_link(uint32_t j, uint32_t i, uint32_t next) { return j | (i << 8) | (next << 16); }
__host__ __device__ inline uint32_t sample_link_pattern(uint32_t link) { return link & 0xFFu; }
__host__ __device__ inline uint32_t sample_link_offset(uint32_t link) { return (link >> 8) & 0x1Fu; }
__host__ __device__ inline uint32_t sample_link_next(uint32_t link) { return link >> 16; }

// The window an entry (., i) offers at sample position p: s = p - i, counted when it lies in [s_begin, s_end).
__host__ __device__ inline bool sample_window(uint64_t p, uint32_t i, uint64_t s_begin, uint64_t s_end, uint64_t* s)
{
    if (p < i) return false;
    *s = p - i;
    return *s >= s_begin && *s < s_end;
}
// The samples a range of windows needs: s_begin <= p <= s_end - 1 + 27, as 16-byte quads [first, end).
__host__ __device__ inline uint64_t sample_quad_first(uint64_t s_begin) { return (s_begin + kSampleStride - 1) / kSampleStride / 4; }
__host__ __device__ inline uint64_t sample_quad_end(uint64_t s_end) { return (s_end + kSampleStride - 2) / kSampleStride / 4 + 1; }

// A workgroup's LDS: u32 filter[2^14] | u32 heads[4096] | SampleEntry entries[28 np] | u32 sums[np].  One workgroup of
// 1024 threads per CU; the CU's 160 KB bound the widths together with the arguments' area: a by-value pass holds
// 4032 / (16 + 32) = 84 patterns at every length, a long pass the 252 pointer pairs the area has room for.
constexpr uint32_t kSampleThreads = 1024;
constexpr uint32_t kSampleLdsMax = 160u * 1024u;
__host__ __device__ constexpr uint32_t sample_lds(uint32_t np) { return 4u * kSampleFilterWords + 4u * kSampleBuckets + np * kSampleStride * 8u + 4u * np; }
constexpr uint32_t kSampleWidth = kMultiArea / (16u + kSampleRow);
constexpr uint32_t kSampleLongWidth = kMultiArea / 16u;
static_assert(kSampleWidth == 84 && kSampleLongWidth == 252 && kSampleLongWidth <= kLongMax, "a key gathers at most kLongMax entries");
static_assert(kSampleLongWidth <= 256 && kSampleLongWidth * kSampleStride < 65536, "a pattern fits the link's 8 bits, an entry index its 16");
static_assert(sample_lds(kSampleLongWidth) <= kSampleLdsMax && kSampleLongWidth <= kSampleThreads, "the widest pass fits one CU's LDS, a thread per pattern");
static_assert(kSampleMinM <= kSampleRow && kSampleRow % 16 == 0, "a row holds every gram a pass enters");

// put pattern g's pointers and its head row into a by-value pass's arguments (a.width == kSampleWidth)
inline void sample_set(MultiArgs& a, uint32_t g, const uint8_t* blob, unsigned long long* count, const uint8_t* row)
{
    __builtin_memcpy(a.area + multi_blob_at(g), &blob, 8);
    __builtin_memcpy(a.area + multi_count_at(a.width, g), &count, 8);
    __builtin_memcpy(a.area + multi_rows_at(a.width) + g * kSampleRow, row, kSampleRow);
}

// The launchers of k_hors.hip, reached through pointers that the unit's own static initialiser sets and api.cpp holds
// (null: no text gets a sample and no pass is sampled), as g_hor_multi.  grid: workgroups, 0 = one per CU.
extern hipError_t (*g_hor_sample)(const MultiArgs& a, const uint32_t* sample, int num_cus, int grid, hipStream_t stream);
extern hipError_t (*g_sample_build)(const uint8_t* text, uint64_t n, uint32_t* sample, int num_cus, hipStream_t stream);

}  // namespace sg
