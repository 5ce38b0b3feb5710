// edit_align.hpp — start position and alignment of ONE edit-distance occurrence of the packed texts (smartgpu_palign_edit64,
// palign.hpp): the DISTANCE form of the recurrence of edit_step.hpp, the value of a cell from a stored column, and the
// traceback.  Host and device: planes_edit_align (k_palign.hip) runs it per lane, tests/packed_align_check.cpp runs the same
// text on the CPU against a scalar DP.  No HIP call, no other header of the library but edit_step.hpp (edit_fresh).
//
// The matrix is the REVERSED one: the reversed pattern against the text read backward from the end position e,
//     D'[i][j] = ed(P[m-i .. m), T[e-j+1 .. e]),   D'[0][j] = j,  D'[i][0] = i,
// so D'[m][j] is the distance of the whole pattern to the j symbols that end at e: the smallest j with the smallest
// D'[m][j] is the match's length J, its start e - J + 1 the LARGEST nearest start.  Column j is held as its vertical
// differences (Pv_j, Mv_j), as in edit_step.hpp; column 0 is edit_fresh.  The caller passes the masks of the REVERSED pattern.
#pragma once
#include "edit_step.hpp"

namespace sg {

// edit_step with row 0 counting: D'[0][j] = j, so a 1 enters the shifted Ph.  Returns D'[m][j] - D'[m][j-1].
template <int WORDS>
SG_HOST_DEVICE inline int edit_step_dist(uint32_t (&pv)[WORDS], uint32_t (&mv)[WORDS], const uint32_t (&eq)[WORDS], uint32_t top)
{
    static_assert(WORDS == 1 || WORDS == 2, "one dword for m <= 32, two for m <= 64");
    uint32_t xv[WORDS], ph[WORDS], mh[WORDS];
    uint32_t carry = 0;
    for (int w = 0; w < WORDS; ++w) {
        const uint32_t x = eq[w] & pv[w];
        const uint32_t s1 = x + pv[w];
        const uint32_t s = s1 + carry;
        carry = static_cast<uint32_t>(s1 < x) | static_cast<uint32_t>(s < s1);
        const uint32_t xh = (s ^ pv[w]) | eq[w];
        xv[w] = eq[w] | mv[w];
        ph[w] = mv[w] | ~(xh | pv[w]);
        mh[w] = pv[w] & xh;
    }
    const bool hi = WORDS == 2 && top >= 32;
    const uint32_t pt = hi ? ph[WORDS - 1] : ph[0], mt = hi ? mh[WORDS - 1] : mh[0];
    const int delta = static_cast<int>((pt >> (top & 31u)) & 1u) - static_cast<int>((mt >> (top & 31u)) & 1u);
    for (int w = WORDS - 1; w > 0; --w) {
        ph[w] = ph[w] << 1 | ph[w - 1] >> 31;
        mh[w] = mh[w] << 1 | mh[w - 1] >> 31;
    }
    ph[0] = ph[0] << 1 | 1u;  // the DISTANCE form: the one line that differs from edit_step
    mh[0] <<= 1;
    for (int w = 0; w < WORDS; ++w) {
        pv[w] = mh[w] | ~(xv[w] | ph[w]);
        mv[w] = ph[w] & xv[w];
    }
    return delta;
}

// D'[i][j] from column j's differences: j + the +1s - the -1s among rows 1 .. i (i <= 32 * WORDS)
template <int WORDS>
SG_HOST_DEVICE inline int edit_cell(const uint32_t (&pv)[WORDS], const uint32_t (&mv)[WORDS], uint32_t i, uint32_t j)
{
    int v = static_cast<int>(j);
    for (int w = 0; w < WORDS; ++w) {
        const uint32_t lo = 32u * w;
        const uint32_t low = i >= lo + 32 ? ~0u : i > lo ? (1u << (i - lo)) - 1u : 0u;
        v += __builtin_popcount(pv[w] & low) - __builtin_popcount(mv[w] & low);
    }
    return v;
}

// bit b (b < 32 * WORDS) of a mask, by select: the device keeps the words in registers
template <int WORDS>
SG_HOST_DEVICE inline uint32_t edit_bit(const uint32_t (&x)[WORDS], uint32_t b)
{
    const uint32_t w = (WORDS == 2 && b >= 32) ? x[WORDS - 1] : x[0];
    return (w >> (b & 31u)) & 1u;
}

// Operations of an alignment, two bits each (smartgpu.h): the pattern's edits.
enum : uint32_t { kOpEq = 0, kOpSub = 1, kOpIns = 2, kOpDel = 3 };
constexpr uint32_t kAlignMaxOps = 71;  // m + k <= SMARTGPU_PEDIT_MAXM + SMARTGPU_PMIS_MAX

// The alignment of the pattern to the J symbols that end at e, D'[m][J] = dist, into ops[3] (operation t in bits
// 2 * (t % 32) of word t / 32, the length L in the top byte of ops[2], every other bit 0); returns L.
// col(j, pv, mv, eq) gives column j (0 <= j <= J; column 0: edit_fresh) and, for j >= 1, the mask Eq of the symbol it consumed
// (T[e-j+1]) against the reversed pattern.  The walk goes from (m, J) to (0, 0) of the reversed matrix, which is text order:
// with R[i][jf] = ed(P[i..m), T[s+jf..e]) = D'[m-i][J-jf] it takes, at every cell, the first that applies of
//   1. the diagonal, when R[i+1][jf+1] + (accepted ? 0 : 1) == R[i][jf]:  '=' or 'X';
//   2. the pattern symbol alone, when R[i+1][jf] + 1 == R[i][jf]:          'D';
//   3. the text symbol alone:                                              'I'.
// Every step lowers i or j, so the loop ends after at most m + J steps whatever the columns hold; an operation beyond the
// 96th (none, when dist <= k) is dropped, not stored out of range.  The three words are built with selects: no indexed store.
template <int WORDS, typename Col>
SG_HOST_DEVICE __attribute__((always_inline)) inline uint32_t edit_traceback(uint32_t m, uint32_t J, int dist, Col&& col, uint64_t (&ops)[3])
{
    uint64_t o0 = 0, o1 = 0, o2 = 0;
    uint32_t i = m, j = J, t = 0;
    int cur = dist;
    while (i > 0 || j > 0) {
        uint32_t pv[WORDS], mv[WORDS], eq[WORDS], lpv[WORDS], lmv[WORDS], leq[WORDS];
        col(j, pv, mv, eq);
        col(j > 0 ? j - 1 : 0, lpv, lmv, leq);
        const uint32_t b = i > 0 ? i - 1 : 0;
        const int up = cur - static_cast<int>(edit_bit<WORDS>(pv, b)) + static_cast<int>(edit_bit<WORDS>(mv, b));  // D'[i-1][j]
        const int diag = edit_cell<WORDS>(lpv, lmv, b, j > 0 ? j - 1 : 0);                                        // D'[i-1][j-1]
        const uint32_t miss = edit_bit<WORDS>(eq, b) ^ 1u;
        uint32_t op;
        if (i > 0 && j > 0 && diag + static_cast<int>(miss) == cur) {
            op = miss ? kOpSub : kOpEq;
            --i; --j;
            cur = diag;
        } else if (i > 0 && (up + 1 == cur || j == 0)) {  // (j == 0: column 0 is D'[i][0] = i, the test holds by itself)
            op = kOpDel;
            --i;
            cur = up;
        } else {
            op = kOpIns;
            --j;
            --cur;
        }
        const uint64_t v = static_cast<uint64_t>(op) << (2u * (t & 31u));
        const uint32_t w = t >> 5;
        o0 |= w == 0 ? v : 0;
        o1 |= w == 1 ? v : 0;
        o2 |= w == 2 ? v : 0;
        ++t;
    }
    ops[0] = o0;
    ops[1] = o1;
    ops[2] = (o2 & 0x00ffffffffffffffull) | static_cast<uint64_t>(t & 0xffu) << 56;
    return t;
}

}  // namespace sg
