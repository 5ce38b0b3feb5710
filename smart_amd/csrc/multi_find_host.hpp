// multi_find_host.hpp — what smartgpu_find_batch64 (api.cpp) decides on the host behind hor_multi_find's launches: the
// entries of a call, (s << kFindBatchShift) | pattern index in no order at all, as K ascending slices of positions.  Host
// only: no HIP call, no error text — tests/find_batch_check.cpp runs it without a device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace sg {

constexpr uint32_t kFindBatchIndexBits = 18;  // multi_find.hpp: kFindBatchShift (api.cpp asserts that they agree)

// entries[0 .. total): the call's entries as the passes' workgroups reached the cursor.  counts[k]: what the kernel
// counted for pattern k.  Afterwards starts[k] = counts[0] + .. + counts[k - 1] (K + 1 of them) and
// entries[starts[k] .. starts[k + 1]) are the positions of pattern k, ascending, the index stripped: a counting sort by
// index, then a sort of each slice.  false — the entries are not what the kernel can have written, and they are left in
// no particular state: an index >= K, a position outside [lo, hi], a pattern whose entries are not counts[k], the counts
// not `total` together, or a position twice in one slice.
inline bool order_find_batch(uint64_t* entries, uint64_t total, uint32_t K, const uint64_t* counts, uint64_t lo, uint64_t hi, uint64_t* starts)
{
    constexpr uint64_t kIndexMask = (1ull << kFindBatchIndexBits) - 1u;
    starts[0] = 0;
    for (uint32_t k = 0; k < K; ++k) {
        if (counts[k] > total - starts[k]) return false;
        starts[k + 1] = starts[k] + counts[k];
    }
    if (starts[K] != total) return false;
    std::vector<uint64_t> fill(starts, starts + K);  // the next free place of every slice
    std::vector<uint64_t> sorted(total);
    for (uint64_t i = 0; i < total; ++i) {
        const uint64_t k = entries[i] & kIndexMask, s = entries[i] >> kFindBatchIndexBits;
        if (k >= K || s < lo || s > hi) return false;
        if (fill[k] == starts[k + 1]) return false;  // more entries than the pattern's count
        sorted[fill[k]++] = s;
    }
    // (every slice is full: the slices hold `total` places together and none took more than its own)
    for (uint32_t k = 0; k < K; ++k) {
        uint64_t* const first = sorted.data() + starts[k];
        uint64_t* const last = sorted.data() + starts[k + 1];
        std::sort(first, last);
        if (std::adjacent_find(first, last) != last) return false;
    }
    std::copy(sorted.begin(), sorted.end(), entries);
    return true;
}

}  // namespace sg
