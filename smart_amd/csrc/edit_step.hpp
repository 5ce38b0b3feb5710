// edit_step.hpp — one column of the edit-distance search of the packed texts (smartgpu_psearch_edit64, pedit.hpp):
// Myers' bit-vector recurrence in Hyyrö's form, on WORDS dwords.  Host and device: planes_edit_scan / planes_edit_find
// (k_pedit.hip) run it per text symbol and lane, tests/packed_edit_check.cpp runs it on the CPU against the plain DP.
// No HIP call, no other header of the library.
//
// The column of Sellers' DP D[0..m][e] (D[0][e] = 0: a match may start anywhere) is held as its vertical differences:
// bit i - 1 of Pv / Mv says D[i][e] - D[i-1][e] is +1 / -1.  A column before which nothing was read is D[i] = i
// (edit_fresh).  edit_step consumes one text symbol through Eq — bit j set: pattern position j accepts it — and returns
// D[m][e] - D[m][e-1], which the caller adds to its score (m after edit_fresh).  Bits from m on, in the last dword, hold
// what the additions carry into them; nothing below depends on them.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SG_HOST_DEVICE __host__ __device__
#else
#define SG_HOST_DEVICE
#endif

namespace sg {

template <int WORDS>
SG_HOST_DEVICE inline void edit_fresh(uint32_t (&pv)[WORDS], uint32_t (&mv)[WORDS])
{
    for (int w = 0; w < WORDS; ++w) {
        pv[w] = ~0u;
        mv[w] = 0u;
    }
}

// top = m - 1: the bit whose horizontal difference is the score's (top < 32 * WORDS)
template <int WORDS>
SG_HOST_DEVICE inline int edit_step(uint32_t (&pv)[WORDS], uint32_t (&mv)[WORDS], const uint32_t (&eq)[WORDS], uint32_t top)
{
    static_assert(WORDS == 1 || WORDS == 2, "one dword for m <= 32, two for m <= 64");
    uint32_t xv[WORDS], ph[WORDS], mh[WORDS];
    uint32_t carry = 0;
    for (int w = 0; w < WORDS; ++w) {
        const uint32_t x = eq[w] & pv[w];
        const uint32_t s1 = x + pv[w];     // (Eq & Pv) + Pv over all WORDS dwords: the carry runs from dword to dword
        const uint32_t s = s1 + carry;
        carry = static_cast<uint32_t>(s1 < x) | static_cast<uint32_t>(s < s1);
        const uint32_t xh = (s ^ pv[w]) | eq[w];
        xv[w] = eq[w] | mv[w];
        ph[w] = mv[w] | ~(xh | pv[w]);
        mh[w] = pv[w] & xh;
    }
    const bool hi = WORDS == 2 && top >= 32;  // (a select, not an indexed read: the device keeps ph / mh in registers)
    const uint32_t pt = hi ? ph[WORDS - 1] : ph[0], mt = hi ? mh[WORDS - 1] : mh[0];
    const int delta = static_cast<int>((pt >> (top & 31u)) & 1u) - static_cast<int>((mt >> (top & 31u)) & 1u);
    // the SEARCH form: row 0 is all zeros, so no 1 enters the shifted Ph (the distance form ORs one in)
    for (int w = WORDS - 1; w > 0; --w) {
        ph[w] = ph[w] << 1 | ph[w - 1] >> 31;
        mh[w] = mh[w] << 1 | mh[w - 1] >> 31;
    }
    ph[0] <<= 1;
    mh[0] <<= 1;
    for (int w = 0; w < WORDS; ++w) {
        pv[w] = mh[w] | ~(xv[w] | ph[w]);
        mv[w] = ph[w] & xv[w];
    }
    return delta;
}

}  // namespace sg
