// k_palign.hip — packed texts: planes_edit_align, the start position, distance and alignment of edit-distance occurrences
// whose END positions the caller lists (smartgpu_palign_edit64): one short backward walk per occurrence with Myers'
// bit-vector recurrence in its DISTANCE form (edit_align.hpp)
// (one translation unit per kernel family: dev_common.hpp; the planes' layout: planes.hpp; the interface: palign.hpp)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "palign.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// planes_edit_align<PLANES, WORDS, OPS>: ONE LANE PER OCCURRENCE.  This kernel runs over a list of end positions, not over
// the text: a lane reads its e, loads the four dwords per plane that hold the symbols e - 96 - e % 32 .. e + 31 - e % 32
// (ordinary cached loads, they need not coalesce; m + k <= 71 symbols back from e lie inside them whatever e % 32 is; a dword
// index below 0 is clamped to 0 and never consumed, because a walk takes at most e - e_begin + 1 <= e + 1 columns; the up to
// 31 symbols above e in its dword are never consumed either) and walks e, e - 1, ... through edit_step_dist with the masks
// of the REVERSED pattern: after j columns the score is ed(P, T[e-j+1 .. e]).  The column starts fresh (score m: the empty
// substring), the lane keeps the minimum and the FIRST column J that reaches it: D(e) and the largest nearest start
// e - J + 1.  min(m + k, e - e_begin + 1) columns decide D(e) <= k exactly: a match within k has at most m + k symbols, so a
// minimum above k means D(e) > k and the entry becomes kAlignNone.
//
// OPS: every column's (Pv, Mv) goes to LDS as dwords [column][Pv words, Mv words][lane] — a lane's bank is its lane number
// whatever column it reads, so the divergent reads of the traceback are conflict-free — and edit_traceback walks them from
// (m, J) back to (0, 0), which emits the operations in text order.  The Eq mask of a column's symbol is not stored: it is
// selected again from the text dwords the lane still holds.
// LDS is dynamic only and at most 64 KB per workgroup, so the launch asks for no attribute: WORDS = 1 (m <= 32: 39 columns,
// 40 rows reserved) takes 40 x 2 x 64 lanes x 4 bytes = 20 KB per workgroup of 64 occurrences; WORDS = 2 at 64 lanes would need
// 72 KB, so that form runs 32 OCCURRENCES PER WORKGROUP (32 threads, half a wave): 72 x 4 x 32 x 4 = 36 KB.  Without OPS
// there is no LDS and every form runs 64 occurrences per workgroup.  No static LDS, no scratch: the text bits and the masks are chosen
// with mask arithmetic, the three ops words with selects of computed values, never with a run-time index.  All positions are
// 64-bit.
// ---------------------------------------------------------------------------
template <int WORDS, bool OPS>
struct AlignGeom {
    static constexpr uint32_t kLanes = (WORDS == 2 && OPS) ? 32 : 64;          // occurrences (threads) per workgroup
    static constexpr uint32_t kCols = WORDS == 2 ? 72 : 40;                     // columns of LDS: >= 32 * WORDS + SMARTGPU_PMIS_MAX
    static constexpr uint32_t kLdsBytes = OPS ? kCols * 2 * WORDS * kLanes * 4 : 0;
    static_assert(kCols >= 32 * WORDS + SMARTGPU_PMIS_MAX && kLdsBytes <= 65536, "every column of the longest walk, in 64 KB");
};

// A lane's four dwords of one plane as two scalars (never an array: nothing the compiler could index at run time), and the
// bit of window position wb (0 .. 127) by select and shift.
struct AlignWindow {
    uint64_t lo, hi;
};
static __device__ __forceinline__ uint32_t align_bit(const AlignWindow& t, uint32_t wb)
{
    const uint64_t up = 0ull - (uint64_t)(wb >> 6);  // all ones for the upper half (arithmetic, not a select of two loads)
    return (uint32_t)(((t.hi & up) | (t.lo & ~up)) >> (wb & 63u)) & 1u;
}

// The four masks as values in scalar registers (readfirstlane: they are wave-uniform kernel arguments).  Left as loads from
// the argument block, the selects below become ONE load at a per-lane address, and the compiler then copies peq to
// private memory to index it.
template <int WORDS>
struct AlignMasks {
    uint32_t c[4][WORDS];
    __device__ __forceinline__ explicit AlignMasks(const PlaneAlignArgs& a)
    {
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int w = 0; w < WORDS; ++w) c[v][w] = __builtin_amdgcn_readfirstlane(a.peq[v][w]);
    }
};

template <int PLANES, int WORDS>
static __device__ __forceinline__ void align_eq(const AlignMasks<WORDS>& q, uint32_t c0, uint32_t c1, uint32_t (&eq)[WORDS])
{
#pragma unroll
    for (int w = 0; w < WORDS; ++w) {
        const uint32_t s0 = 0u - c0, s1 = 0u - c1;  // c0, c1 are 0 or 1: all-ones masks
        const uint32_t e01 = q.c[0][w] ^ ((q.c[0][w] ^ q.c[1][w]) & s0);
        const uint32_t e23 = PLANES == 2 ? q.c[2][w] ^ ((q.c[2][w] ^ q.c[3][w]) & s0) : 0u;
        eq[w] = PLANES == 2 ? e01 ^ ((e01 ^ e23) & s1) : e01;
    }
}

template <int PLANES, int WORDS, bool OPS>
__global__ __launch_bounds__((AlignGeom<WORDS, OPS>::kLanes)) void planes_edit_align(PlaneAlignArgs a)
{
    using G = AlignGeom<WORDS, OPS>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // G::kLdsBytes
    uint32_t* cols = reinterpret_cast<uint32_t*>(smem);
    const uint32_t lane = threadIdx.x;
    const uint64_t idx = (uint64_t)blockIdx.x * G::kLanes + lane;
    if (idx >= a.count) return;  // (no barrier below: a lane's columns are its own)
    const uint64_t e = a.io[idx];
    if (e < a.e_begin || e >= a.e_end) {  // the host has refused such a list; never walk outside the range
        a.io[idx] = kAlignNone;
        if constexpr (OPS) a.ops[3 * idx] = a.ops[3 * idx + 1] = a.ops[3 * idx + 2] = 0;
        return;
    }
    const uint64_t E = e >> 5;
    AlignWindow t0, t1 = {0, 0};
    {
        const uint64_t d0 = E >= 3 ? E - 3 : 0, d1 = E >= 2 ? E - 2 : 0, d2 = E >= 1 ? E - 1 : 0;
        t0.lo = (uint64_t)a.p0[d0] | (uint64_t)a.p0[d1] << 32;
        t0.hi = (uint64_t)a.p0[d2] | (uint64_t)a.p0[E] << 32;
        if (PLANES == 2) {
            t1.lo = (uint64_t)a.p1[d0] | (uint64_t)a.p1[d1] << 32;
            t1.hi = (uint64_t)a.p1[d2] | (uint64_t)a.p1[E] << 32;
        }
    }
    const uint32_t mk = a.m + a.k, top = a.m - 1;
    const uint32_t ncols = e - a.e_begin + 1 < (uint64_t)mk ? (uint32_t)(e - a.e_begin + 1) : mk;  // <= G::kCols: m <= 32 * WORDS
    const uint32_t b0 = 96u + ((uint32_t)e & 31u);  // window bit of symbol e; column j consumed window bit b0 - (j - 1)

    const AlignMasks<WORDS> masks(a);
    uint32_t pv[WORDS], mv[WORDS];
    edit_fresh<WORDS>(pv, mv);
    int score = (int)a.m, best = (int)a.m;
    uint32_t J = 0;
    for (uint32_t j = 1; j <= ncols; ++j) {
        const uint32_t wb = b0 - (j - 1);
        const uint32_t c0 = align_bit(t0, wb), c1 = align_bit(t1, wb);
        uint32_t eq[WORDS];
        align_eq<PLANES, WORDS>(masks, c0, c1, eq);
        score += edit_step_dist<WORDS>(pv, mv, eq, top);
        if constexpr (OPS) {
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                cols[((j - 1) * 2 * WORDS + w) * G::kLanes + lane] = pv[w];
                cols[((j - 1) * 2 * WORDS + WORDS + w) * G::kLanes + lane] = mv[w];
            }
        }
        if (score < best) {
            best = score;
            J = j;
        }
    }
    const bool hit = best <= (int)a.k;
    a.io[idx] = hit ? (unsigned long long)(e + 1 - J) << kMisShift | (unsigned long long)best : kAlignNone;
    if constexpr (OPS) {
        uint64_t ops[3] = {0, 0, 0};
        if (hit) {
            auto col = [&](uint32_t j, uint32_t (&cpv)[WORDS], uint32_t (&cmv)[WORDS], uint32_t (&ceq)[WORDS]) __attribute__((always_inline)) {
                const uint32_t r = j ? j - 1 : 0;  // (column 0 reads row 0 and drops it: J >= 1 wherever it is asked for with i > 0)
                const uint32_t wb = b0 - r;
                const uint32_t c0 = align_bit(t0, wb), c1 = align_bit(t1, wb);
                align_eq<PLANES, WORDS>(masks, c0, c1, ceq);
#pragma unroll
                for (int w = 0; w < WORDS; ++w) {
                    const uint32_t p = cols[(r * 2 * WORDS + w) * G::kLanes + lane], q = cols[(r * 2 * WORDS + WORDS + w) * G::kLanes + lane];
                    cpv[w] = j ? p : ~0u;
                    cmv[w] = j ? q : 0u;
                }
            };
            edit_traceback<WORDS>(a.m, J, best, col, ops);
        }
        a.ops[3 * idx] = ops[0];
        a.ops[3 * idx + 1] = ops[1];
        a.ops[3 * idx + 2] = ops[2];
    }
}

static hipError_t launch_planes_edit_align(const PlaneAlignArgs& a, int planes, hipStream_t stream)
{
    if (a.m < 1 || a.m > kEditMaxM || a.k > SMARTGPU_PMIS_MAX || !a.io) return hipErrorInvalidValue;
    if (a.count == 0) return hipSuccess;
#define SG_ALIGN(p_, w_, o_)                                                                                                       \
    do {                                                                                                                           \
        using G = AlignGeom<w_, o_>;                                                                                               \
        const uint64_t grid = (a.count + G::kLanes - 1) / G::kLanes;                                                               \
        if (grid > 0x7fffffffull) return hipErrorInvalidValue;                                                                     \
        hipLaunchKernelGGL((planes_edit_align<p_, w_, o_>), dim3((uint32_t)grid), dim3(G::kLanes), G::kLdsBytes, stream, a);       \
    } while (0)
    const bool ops = a.ops != nullptr;
    if (planes == 2) {
        if (a.m <= 32) { if (ops) SG_ALIGN(2, 1, true); else SG_ALIGN(2, 1, false); }
        else           { if (ops) SG_ALIGN(2, 2, true); else SG_ALIGN(2, 2, false); }
    } else {
        if (a.m <= 32) { if (ops) SG_ALIGN(1, 1, true); else SG_ALIGN(1, 1, false); }
        else           { if (ops) SG_ALIGN(1, 2, true); else SG_ALIGN(1, 2, false); }
    }
#undef SG_ALIGN
    return hipGetLastError();
}

// match_calls.cpp reaches the launcher once this unit is part of the program (palign.hpp)
namespace {
struct RegisterPlanesAlign {
    RegisterPlanesAlign() { g_planes_edit_align = &launch_planes_edit_align; }
} g_register_planes_align;
}  // namespace

}  // namespace sg
