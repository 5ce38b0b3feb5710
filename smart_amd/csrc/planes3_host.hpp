// planes3_host.hpp — what the calls of match_calls.cpp on a THREE-PLANE packed text decide on the host before a launch: the
// pattern as eight membership planes.  Host only: no HIP call, no error text — tests/packed_wide_check.cpp runs it all
// without a device.  The layout is planes3.hpp's; the find's spans are ordered by planes_host.hpp's order_spans.
#pragma once
#include "planes3.hpp"

#include <cstring>

namespace sg {

// The set pattern as membership planes: bit j % 32 of Y[c * kPatWords + j / 32] = position j accepts code c, c < 8;
// kSet8Words dwords, zero beyond m.  A position that accepts every value of the text gets ALL EIGHT bits (planes3.hpp: no
// instruction).  *empty: the number of positions that accept nothing; fill_empty (a mismatch in every window, counted
// here) gives them all eight bits as well, otherwise they keep none.  *full: every position accepts everything.
// Returns -1, or the first position whose set names a code >= nvalues (Y, *empty and *full are then unfinished).
inline int encode_sets8(int nvalues, const uint8_t* sets, uint32_t m, bool fill_empty, uint32_t* Y, uint32_t* empty, bool* full)
{
    const uint32_t all = (1u << nvalues) - 1u;
    std::memset(Y, 0, 4 * kSet8Words);
    *empty = 0;
    *full = true;
    for (uint32_t j = 0; j < m; ++j) {
        uint32_t s = sets[j];
        if (s & ~all) return static_cast<int>(j);
        if (s != all) *full = false;
        if (s == 0) ++*empty;
        if (s == all || (s == 0 && fill_empty)) s = 0xFFu;
        for (uint32_t c = 0; c < 8; ++c)
            if (s >> c & 1u) Y[c * kPatWords + (j >> 5)] |= 1u << (j & 31);
    }
    return -1;
}

// A byte pattern as sets over the text's `values` (ascending, nvalues of them): sets[j] = the singleton of the code of
// P[j], or the empty set for a byte the text does not hold (FOREIGN).  Returns the number of foreign positions.
inline uint32_t pattern_sets8(const uint8_t values[8], int nvalues, const uint8_t* P, uint32_t m, uint8_t* sets)
{
    int code_of[256];
    for (int c = 0; c < 256; ++c) code_of[c] = -1;
    for (int k = 0; k < nvalues; ++k) code_of[values[k]] = k;
    uint32_t foreign = 0;
    for (uint32_t j = 0; j < m; ++j) {
        const int c = code_of[P[j]];
        sets[j] = c < 0 ? uint8_t(0) : static_cast<uint8_t>(1u << c);
        foreign += c < 0;
    }
    return foreign;
}

// The byte pattern as membership planes: pattern_sets8 through encode_sets8 (m <= SMARTGPU_XSIZE).  Returns the number of
// foreign positions; fill_foreign gives them all eight bits (not compared: the host counts them), otherwise none.
inline uint32_t encode_pattern8(const uint8_t values[8], int nvalues, const uint8_t* P, uint32_t m, bool fill_foreign, uint32_t* Y)
{
    uint8_t sets[SMARTGPU_XSIZE];
    const uint32_t foreign = pattern_sets8(values, nvalues, P, m, sets);
    uint32_t empty = 0;
    bool full = false;
    (void)encode_sets8(nvalues, sets, m, fill_foreign, Y, &empty, &full);  // (a singleton of a code < nvalues: never refused)
    return foreign;
}

}  // namespace sg
