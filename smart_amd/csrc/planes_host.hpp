// planes_host.hpp — what the packed-text calls of match_calls.cpp decide on the host before (the pattern as planes) and after
// (what a find's cursor means, the find's entries in order) a launch.  Host only: no HIP call, no error text —
// tests/packed_host_check.cpp runs it all without a device.  The planes' layout is planes.hpp's.
#pragma once
#include "planes.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace sg {

// The pattern as planes: bit j % 32 of X0[j / 32], X1[j / 32] = bits 0 / 1 of the code of P[j] among the text's `values`
// (ascending, nvalues of them); kPatWords dwords each, zero beyond m.  A byte the text does not hold is FOREIGN: its code
// bits are zero and, when SKIP is given (kPatWords dwords, PlaneMisArgs), its bit there is set.  Returns their number
// (without mismatches: > 0 means no occurrence).
inline uint32_t encode_pattern(const uint8_t values[4], int nvalues, const uint8_t* P, uint32_t m, uint32_t* X0, uint32_t* X1, uint32_t* SKIP)
{
    int code_of[256];
    for (int c = 0; c < 256; ++c) code_of[c] = -1;
    for (int k = 0; k < nvalues; ++k) code_of[values[k]] = k;
    std::memset(X0, 0, 4 * kPatWords);
    std::memset(X1, 0, 4 * kPatWords);
    if (SKIP) std::memset(SKIP, 0, 4 * kPatWords);
    uint32_t foreign = 0;
    for (uint32_t j = 0; j < m; ++j) {
        const int c = code_of[P[j]];
        if (c < 0) {
            if (SKIP) SKIP[j >> 5] |= 1u << (j & 31);
            ++foreign;
            continue;
        }
        X0[j >> 5] |= static_cast<uint32_t>(c & 1) << (j & 31);
        X1[j >> 5] |= static_cast<uint32_t>(c >> 1) << (j & 31);
    }
    return foreign;
}

constexpr size_t kSetWords = 4 * kPatWords;  // a set pattern's four membership planes

// The set pattern as membership planes: bit j % 32 of Y[c * kPatWords + j / 32] = position j accepts code c; kSetWords
// dwords, zero beyond m.  A position that accepts every value of the text gets ALL its bits (planes.hpp: no instruction).
// *empty: the number of positions that accept nothing; fill_empty (PlaneSetMisArgs: a mismatch in every window, counted
// here) gives them all their bits as well, otherwise they keep none.  *full: every position accepts everything.
// Returns -1, or the first position whose set names a code >= nvalues (Y, *empty and *full are then unfinished).
inline int encode_sets(int nvalues, const uint8_t* sets, uint32_t m, bool fill_empty, uint32_t* Y, uint32_t* empty, bool* full)
{
    const uint32_t all = (1u << nvalues) - 1u;
    std::memset(Y, 0, 4 * kSetWords);
    *empty = 0;
    *full = true;
    for (uint32_t j = 0; j < m; ++j) {
        uint32_t s = sets[j];
        if (s & ~all) return static_cast<int>(j);
        if (s != all) *full = false;
        if (s == 0) ++*empty;
        if (s == all || (s == 0 && fill_empty)) s = 0xFu;
        for (uint32_t c = 0; c < 4; ++c)
            if (s >> c & 1u) Y[c * kPatWords + (j >> 5)] |= 1u << (j & 31);
    }
    return -1;
}

// planes_find's output in ascending order.  It is a sequence of spans (planes.hpp): each ascending and contiguous, each the
// survivors of its own kFindSpan start positions counted from the range's first chunk, in the order the waves reserved them.
// So the spans are found in one pass (the span number changes), ordered by it — one entry per span, not per position;
// s_last is the last start position of the range — and moved only when they are out of order.  All `have` entries must be present (count <= cap).
// shift: the entries hold their position above `shift` low bits (planes_mis_find: the distance) and are ordered whole.
// false: the entries are not such spans (refused by the callers, never reported).
inline bool order_spans(uint64_t* pos, uint64_t have, uint64_t s_begin, uint64_t s_last, uint32_t shift = 0)
{
    static_assert((kFindSpan & (kFindSpan - 1)) == 0, "span number by division");
    const uint64_t base = s_begin / 128 * 128;
    struct Span { uint64_t key, begin, len; };
    std::vector<Span> spans;
    bool ascending = true;
    for (uint64_t i = 0; i < have; ++i) {
        const uint64_t key = ((pos[i] >> shift) - base) / kFindSpan;
        if (!spans.empty() && spans.back().key == key) {
            if (pos[i] <= pos[i - 1]) return false;  // not what planes_find writes (a retuned kernel whose spans are no longer these?)
            ++spans.back().len;
            continue;
        }
        if (!spans.empty() && key < spans.back().key) ascending = false;
        spans.push_back({key, i, 1});
    }
    if (ascending) return true;
    std::vector<uint64_t> tmp(have);
    uint64_t at = 0;
    const uint64_t nkeys = (s_last - base) / kFindSpan + 1;
    if (nkeys <= 16 * spans.size() + 4096) {
        // many short spans (a pattern that occurs in every tenth span: a sort of 130,000 keys took most of the call): the
        // span numbers are unique and bounded, so a table indexed by them orders the spans in one pass
        constexpr uint64_t kNone = ~0ull;
        std::vector<uint64_t> by_key(nkeys, kNone);
        for (size_t i = 0; i < spans.size(); ++i) {
            if (spans[i].key >= nkeys || by_key[spans[i].key] != kNone) return false;  // outside the range, or a span in two pieces
            by_key[spans[i].key] = i;
        }
        for (uint64_t k = 0; k < nkeys; ++k) {
            if (by_key[k] == kNone) continue;
            const Span& sp = spans[by_key[k]];
            std::memcpy(&tmp[at], pos + sp.begin, sp.len * sizeof(uint64_t));
            at += sp.len;
        }
    } else {
        std::sort(spans.begin(), spans.end(), [](const Span& x, const Span& y) { return x.key < y.key; });
        for (size_t i = 1; i < spans.size(); ++i)
            if (spans[i].key == spans[i - 1].key) return false;  // a span in two pieces
        for (const Span& sp : spans) {
            std::memcpy(&tmp[at], pos + sp.begin, sp.len * sizeof(uint64_t));
            at += sp.len;
        }
    }
    std::memcpy(pos, tmp.data(), have * sizeof(uint64_t));
    return true;
}

// The entries of a find whose kernel keeps no order at all (planes_editl_find), (e << shift) | D(e) as the waves' pieces
// reached the cursor: sorted, then refused (false) unless they are distinct end positions of [lo, hi] with distances <= k.
inline bool order_editl(uint64_t* entries, uint64_t count, uint64_t lo, uint64_t hi, uint32_t k, uint32_t shift)
{
    std::sort(entries, entries + count);
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t e = entries[i] >> shift;
        if (e < lo || e > hi || (entries[i] & ((1u << shift) - 1u)) > k) return false;
        if (i && e == entries[i - 1] >> shift) return false;
    }
    return true;
}

// What the cursor of a find means once the device has answered.  total: the cursor, every occurrence counted whether it
// was stored or not; bound: the positions an occurrence can have; cap: the caller's room; room_got: the device buffer the
// kernel stored into, min(cap, bound) entries, or 0 when the device had no memory for them (the call still counts).
enum class FindOutcome {
    kBeyondBound,  // total > bound: a poisoned cursor, refused and never reported
    kComplete,     // every occurrence is in the device buffer: copy the list and order it (nothing to copy at total = 0)
    kOverCap,      // more occurrences than the caller has room for: the count alone
    kNoRoom,       // the caller's room would do, the device had none: the count alone
};
inline FindOutcome find_outcome(uint64_t total, uint64_t bound, uint64_t room_got, uint64_t cap)
{
    if (total > bound) return FindOutcome::kBeyondBound;
    if (total > cap) return FindOutcome::kOverCap;
    if (total > room_got) return FindOutcome::kNoRoom;
    return FindOutcome::kComplete;
}

}  // namespace sg
