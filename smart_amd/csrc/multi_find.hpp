// multi_find.hpp — the arguments of hor_multi_find (k_hormf.hip): the POSITIONS of up to find_width(m) patterns of one
// length in ONE pass over a byte text, on multi.hpp's table rule, walk and candidate chains.  Included by k_hormf.hip and
// by api.cpp (smartgpu_find_batch64), which stages a call's patterns and sends its passes.
#pragma once
#include "multi.hpp"

namespace sg {

// An occurrence of pattern g of a pass at start s is ONE entry, (s << kFindBatchShift) | (base + g): base is the index of
// the pass's first pattern in the call's set.  Every pass of a call appends to one buffer behind one cursor, in no order;
// the host sorts the entries into the patterns' slices (multi_find_host.hpp).  So a call takes at most 2^18 patterns, and
// the range it searches ends below byte 2^46.
constexpr uint32_t kFindBatchShift = 18;
constexpr uint32_t kFindBatchMaxK = 1u << kFindBatchShift;
constexpr uint64_t kFindBatchMaxEnd = 1ull << (64 - kFindBatchShift);  // off + n stays BELOW this

// The patterns of a call travel through the device's pinned staging buffer (kStagingBytes of it, api.cpp: DeviceCtx) into
// the arena: K rows — tail_fill's bytes at tail_stride(m), what the table is built from and what a lane compares in LDS —
// and, where a window is completed in memory (m - 1 > kHaloMax), the K whole patterns at a pitch of find_pitch(m) bytes
// (a multiple of 16: a compare reads 16 bytes at a time and stays inside the pattern's own pitch).
constexpr uint32_t kHaloMaxFind = 16;  // kernels.hpp: kHaloMax (k_hormf.hip asserts that they agree; this header stays host-clean)
constexpr size_t kStagingBytes = size_t(32) << 20;
__host__ __device__ constexpr uint32_t find_pitch(uint32_t m) { return (m + 15u) & ~15u; }
__host__ __device__ constexpr bool find_in_memory(uint32_t m) { return m - 1u > kHaloMaxFind; }
// bytes staged per pattern
__host__ __device__ constexpr uint32_t find_batch_bytes(uint32_t m) { return tail_stride(m) + (find_in_memory(m) ? find_pitch(m) : 0u); }
// the most patterns one call takes at length m: what the staging buffer holds, and 2^18 at the most
__host__ __device__ constexpr uint32_t find_batch_max(uint32_t m)
{
    return kStagingBytes / find_batch_bytes(m) < kFindBatchMaxK ? (uint32_t)(kStagingBytes / find_batch_bytes(m)) : kFindBatchMaxK;
}
static_assert(find_batch_max(3) == kFindBatchMaxK && find_batch_max(32) == kFindBatchMaxK && find_batch_max(300) == 87381 && find_batch_max(4096) == 8035,
              "the bound include/smartgpu.h documents");

// The output STAGE of a workgroup, in LDS: kFindStage entries and the words of the flush.  A lane that has verified an
// occurrence takes a slot of the stage with an LDS atomic; between two tiles the workgroup reserves what the stage holds
// with ONE atomicAdd on the cursor and writes it out.  A lane that finds the stage full reserves one slot of the output
// itself.
constexpr uint32_t kFindStage = 128;
constexpr uint32_t kFindStageLds = 8u * kFindStage + 64u;  // the entries | u32 taken | u32 pad | u64 base | pad to 64

// A pass is as wide as the LDS allows when four workgroups are resident on a CU (kMultiLdsBudget each): the table, the
// heads, np rows with a link and a sum each, the stage, the tile — multi.hpp's long pass plus the stage.
__host__ __device__ constexpr uint32_t find_head(uint32_t np, uint32_t stride) { return kGramSlots + 4u * kGramBuckets + round64(np * (stride + 8u)) + kFindStageLds; }
__host__ __device__ constexpr bool find_fits(uint32_t m, uint32_t np)
{
    // a thread per pattern, a pass's rows in two 16-byte pieces per thread
    return np <= kMultiThreads && np * tail_stride(m) <= 2u * kMultiThreads * 16u && find_head(np, tail_stride(m)) + kMultiTileLds <= kMultiLdsBudget;
}
__host__ __device__ constexpr uint32_t find_search(uint32_t m)
{
    uint32_t np = 0;
    while (find_fits(m, np + 1u)) ++np;  // (what fits is monotone in np)
    return np;
}
constexpr uint32_t kFindWidth[5] = {find_search(16), find_search(32), find_search(48), find_search(64), find_search(65)};
constexpr uint32_t find_width(uint32_t m) { return kFindWidth[tail_stride(m) / 16u - 1u]; }
static_assert(find_width(3) == 208 && find_width(16) == 208 && find_width(17) == 124 && find_width(32) == 124 && find_width(33) == 89 && find_width(48) == 89 &&
              find_width(49) == 69 && find_width(64) == 69 && find_width(65) == 56 && find_width(4096) == 56, "the pass width of every row stride");
static_assert(kFindStageLds % 64 == 0 && find_head(208, 16) + kMultiTileLds <= kMultiLdsBudget && find_head(56, 80) + kMultiTileLds <= kMultiLdsBudget,
              "the widest pass leaves four workgroups per CU resident, and the tile stays 64-byte aligned");

// What hor_multi_find receives, by value: nothing of it grows with the pass.
struct MultiFindArgs {
    const uint8_t* text;          // device pointer to text byte 0
    uint64_t s_begin, s_end;      // start positions to list, as ScanArgs
    uint32_t m;                   // pattern length, >= 3
    uint32_t halo;                // back halo H = min(m - 1, kHaloMax)
    uint32_t np;                  // patterns in this pass, 1 <= np <= find_width(m)
    uint32_t base;                // the index of the pass's first pattern in the call's set
    const uint8_t* rows;          // device: the pass's np rows at tail_stride(m), 16-byte aligned
    const uint8_t* pats;          // device: the pass's np whole patterns at find_pitch(m); read only where m - 1 > halo
    unsigned long long* counts;   // device: the CALL's counts (pre-zeroed); the pass adds to counts[base + g]
    unsigned long long* out;      // device: the call's entries, or null with cap == 0
    unsigned long long cap;       // entries `out` has room for
    unsigned long long* cursor;   // device: every occurrence found, stored or not (pre-zeroed, shared by the call's passes)
};

// The launcher of k_hormf.hip, reached through a pointer that the unit's own static initialiser sets (as g_hor_multi):
// null — the unit is not linked — and smartgpu_find_batch64 answers SMARTGPU_ERR_HIP; it never falls back to anything.
extern hipError_t (*g_hor_multi_find)(const MultiFindArgs& a, int num_cus, hipStream_t stream);

}  // namespace sg
