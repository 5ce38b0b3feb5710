// k_peditl.hip — packed texts: planes_editl_scan / planes_editl_find, occurrences within EDIT distance k of patterns up
// to 256 symbols, k up to 31, by Myers' bit-vector recurrence in blocks of 32 rows with Ukkonen's cut-off (edit_block.hpp)
// (one translation unit per kernel family: dev_common.hpp; the planes' layout: planes.hpp; the interface: peditl.hpp)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "peditl.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// planes_editl_scan<PLANES, WORDS> counts, planes_editl_find<PLANES, WORDS> lists the END positions e in [e_begin, e_end)
// with D(e) <= k, D as k_pedit.hip defines it: the last row of Sellers' DP on the range alone.  WORDS = 2, 4 or 8 dwords
// hold the column of a pattern of at most 32 WORDS symbols; the pattern is the four masks peq[code], 8 dwords each, kernel
// arguments; the symbol's code bits select one of them per active block.
//
// THE CUT-OFF.  Of a column's W = ceil(m / 32) blocks only the first B are stepped; the rule (grow before a symbol when
// the last active block's bottom value is <= k, shrink while it is >= k + the block's rows, report only with B == W) and
// the one score that is kept are edit_block.hpp's.  It is exact, not approximate:
//   * values along a DP path never decrease, so a cell <= k derives only from cells <= k, and those all lie in active
//     blocks: a block is left out only while every cell of it is > k, and it comes back, as a fresh upper bound, in the
//     column after the one in which the row above it reached k;
//   * everything that is computed is >= the true value;
//   * hence every computed value <= k is the true one, and the rest are truly > k.
// One grow per column is enough: a fresh block's bottom is >= 32 > k above the one before it (k <= 31).
// B is the WAVE's, not the lane's — a scalar, so that the unrolled blocks are skipped by scalar branches and pv / mv are
// indexed by constants only (no scratch): the wave grows when ANY of its lanes asks for it and shrinks when ALL agree.  A
// lane that carries more blocks than it needs still holds valid values, by the same argument.  With all_blocks set B is W
// from the first column on and never changes: the same answers, for the cross-check and the measurement.
//
// GEOMETRY.  A lane owns kEditlRun = 512 consecutive end positions, lane l of a wave the l-th run of 64, and walks them in
// pieces of 128 symbols, each loaded as it is reached (16 bytes per plane); all lanes of a wave consume the symbol at the
// same offset of their runs in the same step.  The fresh start of k_pedit.hip carries over unchanged: a lane starts at
// max(e_begin, first owned - (m + k)) with D[i] = i and counts only at owned positions; m + k <= 287 symbols lie in the
// three pieces before its run.  A lane whose start is clipped at e_begin begins later than its neighbours: it resets its
// column to the fresh one on B blocks (bot = min(32 B, m)) at its own first column, and takes no part in the votes before.
//
// The find collects the hits of 32 owned positions as a bit mask and their distances bit-sliced in five more dwords, and
// runs planes_find's output stage once per wave and 32 positions: prefix sum of the lanes' counts, ONE atomicAdd on the
// cursor, ordinary vector stores of (e << kEditlShift) | D(e) while slot < cap.  The entries reach the host in no order;
// it sorts them.  No static LDS, no scratch.
//
// Measured (1 Gi symbols of rand4, profiles/packed/RESULTS.md, "Edit distance: long patterns"): the scan takes 1.48-2.59 ms
// at k <= 7 for m = 64 .. 256 — one active block; the growth with m is the warm-up —, 4.86 ms at m = 256, k = 31; with
// all_blocks 2.07-9.66 ms, 3.6-3.7 x the cut-off form at m = 256, k <= 7.  Where every block is active anyway (m = 64,
// k >= 15) the votes and branches cost 7 %.  Other run lengths, a prefetch of the next piece and the occupancy: not tried.
// ---------------------------------------------------------------------------
constexpr int kEditlT = 256;
constexpr int kEditlWgs = 8;                     // workgroups per CU
constexpr int kEditlWarm = (int)(kEditlWarmPieces * kEditlPiece);
constexpr int kEditlPieces = (int)(kEditlWarmPieces + kEditlRun / kEditlPiece);
constexpr int kEditlPieceDw = (int)(kEditlPiece / 32);
static_assert(kEditlPieceDw == 4, "a piece is one 16-byte load per plane");
static_assert(kEditlMaxK < 32, "one grow per column: a fresh block's bottom is more than k above the block before it");

template <int PLANES, int WORDS, bool FIND>
static __device__ __forceinline__ void planes_editl_body(const PlaneEditlArgs& a, uint8_t* smem, unsigned long long* __restrict__ out,
                                                         unsigned long long cap)
{
    const uint64_t c_end = (a.e_end + kEditlRun - 1) / kEditlRun;
    const uint64_t stride = (uint64_t)gridDim.x * kEditlT;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t mk = a.m + a.k, W = (a.m + 31u) / 32u;
    const bool cut = a.all_blocks == 0u;
    const int x0 = kEditlWarm - (int)mk;  // the first column any lane walks, counted from kEditlWarm symbols before its run
    uint32_t hits = 0;
    // the trip count is the WAVE's (its first run decides): every lane stays for the votes and the shuffles
    for (uint64_t cw = a.e_begin / kEditlRun + (uint64_t)blockIdx.x * kEditlT + 64u * wave; cw < c_end; cw += stride) {
        const uint64_t c = cw + lane;
        const bool in = c < c_end;
        // the columns this lane walks: [first, last); those from kEditlWarm on are owned
        int first = 0, last = 0;
        {
            const uint64_t base = c * kEditlRun;
            const uint64_t own_lo = base > a.e_begin ? base : a.e_begin, own_hi = base + kEditlRun < a.e_end ? base + kEditlRun : a.e_end;
            if (in && own_lo < own_hi) {
                const uint64_t start = own_lo - a.e_begin > mk ? own_lo - mk : a.e_begin;
                first = kEditlWarm + (int)(long long)(start - base);
                last = kEditlWarm + (int)(own_hi - base);
            }
        }
        uint32_t pv[WORDS], mv[WORDS];
        int bot;
        uint32_t B = cut ? 1u : W;
        block_fresh<WORDS>(pv, mv, B, a.m, bot);
        for (int j = x0 / (int)kEditlPiece; j < kEditlPieces; ++j) {
            const int xlo = x0 > j * (int)kEditlPiece ? x0 : j * (int)kEditlPiece;
            if (!__any(first < (j + 1) * (int)kEditlPiece && last > xlo)) continue;  // (no lane of the wave walks this piece)
            uint4 va, vb = make_uint4(0u, 0u, 0u, 0u);
            {
                // dword of the piece in its plane; a piece before the text (run 0's warm-up) is not walked: any address will do
                const long long g = (long long)(c * (kEditlRun / 32)) + (long long)kEditlPieceDw * (j - (int)kEditlWarmPieces);
                const uint64_t dw = in && g > 0 ? (uint64_t)g : 0;
                if (j >= (int)kEditlWarmPieces) {
                    va = ld_stream16(reinterpret_cast<const uint8_t*>(a.p0 + dw));
                    if (PLANES == 2) vb = ld_stream16(reinterpret_cast<const uint8_t*>(a.p1 + dw));
                } else {  // the neighbour's run: cached
                    va = *reinterpret_cast<const uint4*>(a.p0 + dw);
                    if (PLANES == 2) vb = *reinterpret_cast<const uint4*>(a.p1 + dw);
                }
            }
            for (int d = 0; d < kEditlPieceDw; ++d) {
                const int xd = j * (int)kEditlPiece + 32 * d;
                const int blo = xlo > xd ? xlo - xd : 0;
                if (blo >= 32) continue;
                uint32_t w0 = (d == 0 ? va.x : d == 1 ? va.y : d == 2 ? va.z : va.w) >> blo;
                uint32_t w1 = PLANES == 2 ? (d == 0 ? vb.x : d == 1 ? vb.y : d == 2 ? vb.z : vb.w) >> blo : 0u;
                uint32_t M = 0, D[5] = {0u, 0u, 0u, 0u, 0u};
                for (int b = blo; b < 32; ++b) {
                    const int x = xd + b;
                    if (__any(x == first)) {  // (rare: the wave's first column, and starts clipped at e_begin, later than the wave's)
                        if (x == first) block_fresh<WORDS>(pv, mv, B, a.m, bot);
                    }
                    const bool act = (uint32_t)(x - first) < (uint32_t)(last - first);
                    if (cut && B < W && __any(act && block_wants_grow(bot, a.k))) block_grow<WORDS>(pv, mv, B, a.m, bot);
                    bot += block_step<WORDS>(pv, mv, [&](int w) {  // (the mask's dword: selected for the active blocks only)
                        const uint32_t e01 = (w0 & 1u) ? a.peq[1][w] : a.peq[0][w];
                        return PLANES == 2 ? ((w1 & 1u) ? ((w0 & 1u) ? a.peq[3][w] : a.peq[2][w]) : e01) : e01;
                    }, B, a.m);
                    if (cut)
                        while (B > 1u && __all(!act || block_may_shrink(bot, a.k, B, a.m))) block_shrink<WORDS>(pv, mv, B, a.m, bot);
                    const bool hit = act && j >= (int)kEditlWarmPieces && B == W && bot <= (int)a.k;
                    if constexpr (!FIND) {
                        hits += hit;
                    } else {
                        const uint32_t h = hit ? 1u << b : 0u;
                        M |= h;
#pragma unroll
                        for (int s = 0; s < 5; ++s) D[s] |= (bot >> s & 1) ? h : 0u;
                    }
                    w0 >>= 1;
                    w1 >>= 1;
                }
                if constexpr (FIND) {
                    if (!__any(M != 0u)) continue;
                    // planes_find's output stage: wave-wide exclusive prefix sum of the lanes' counts, one atomic, the lanes' stores
                    const uint32_t mine = __builtin_popcount(M);
                    unsigned long long slot = wave_reserve(mine, a.count, lane);
                    const uint64_t pos = c * kEditlRun + (uint64_t)(xd - kEditlWarm);  // (hits lie in owned pieces: xd >= kEditlWarm)
                    uint32_t r = M;
                    while (r) {
                        const uint32_t i = __builtin_ctz(r);
                        r &= r - 1;
                        const uint32_t dist = ((D[0] >> i) & 1u) | ((D[1] >> i) & 1u) << 1 | ((D[2] >> i) & 1u) << 2 | ((D[3] >> i) & 1u) << 3 |
                                              ((D[4] >> i) & 1u) << 4;
                        if (slot < cap) out[slot] = (pos + i) << kEditlShift | dist;
                        ++slot;
                    }
                }
            }
        }
    }
    if constexpr (!FIND) flush_hits(hits, a.count, smem, reinterpret_cast<const uint8_t*>(a.p0));
}

template <int PLANES, int WORDS>
__global__ __launch_bounds__(kEditlT, 8) void planes_editl_scan(PlaneEditlArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // 128 bytes: flush_hits
    planes_editl_body<PLANES, WORDS, false>(a, smem, nullptr, 0);
}

template <int PLANES, int WORDS>
__global__ __launch_bounds__(kEditlT, 8) void planes_editl_find(PlaneEditlArgs a, unsigned long long* __restrict__ out, unsigned long long cap)
{
    planes_editl_body<PLANES, WORDS, true>(a, nullptr, out, cap);
}

static bool editl_args_ok(const PlaneEditlArgs& a) { return a.m >= 1 && a.m <= kEditlMaxM && a.k <= kEditlMaxK; }

static uint32_t planes_editl_grid(const PlaneEditlArgs& a, int num_cus)
{
    const uint64_t runs = (a.e_end + kEditlRun - 1) / kEditlRun - a.e_begin / kEditlRun;
    return (uint32_t)std::min<uint64_t>((runs + kEditlT - 1) / kEditlT, (uint64_t)num_cus * kEditlWgs);
}

static hipError_t launch_planes_editl_scan(const PlaneEditlArgs& a, int planes, int num_cus, hipStream_t stream)
{
    if (!editl_args_ok(a)) return hipErrorInvalidValue;
    if (a.e_end <= a.e_begin) return hipSuccess;
    const uint32_t grid = planes_editl_grid(a, num_cus);
#define SG_EDITL_SCAN(p_, w_) hipLaunchKernelGGL((planes_editl_scan<p_, w_>), dim3(grid), dim3(kEditlT), 128, stream, a)
    if (planes == 2) {
        if (a.m <= 64) SG_EDITL_SCAN(2, 2); else if (a.m <= 128) SG_EDITL_SCAN(2, 4); else SG_EDITL_SCAN(2, 8);
    } else {
        if (a.m <= 64) SG_EDITL_SCAN(1, 2); else if (a.m <= 128) SG_EDITL_SCAN(1, 4); else SG_EDITL_SCAN(1, 8);
    }
#undef SG_EDITL_SCAN
    return hipGetLastError();
}

static hipError_t launch_planes_editl_find(const PlaneEditlArgs& a, unsigned long long* out, unsigned long long cap, int planes, int num_cus,
                                           hipStream_t stream)
{
    if (!editl_args_ok(a)) return hipErrorInvalidValue;
    if (a.e_end <= a.e_begin) return hipSuccess;
    const uint32_t grid = planes_editl_grid(a, num_cus);
#define SG_EDITL_FIND(p_, w_) hipLaunchKernelGGL((planes_editl_find<p_, w_>), dim3(grid), dim3(kEditlT), 0, stream, a, out, cap)
    if (planes == 2) {
        if (a.m <= 64) SG_EDITL_FIND(2, 2); else if (a.m <= 128) SG_EDITL_FIND(2, 4); else SG_EDITL_FIND(2, 8);
    } else {
        if (a.m <= 64) SG_EDITL_FIND(1, 2); else if (a.m <= 128) SG_EDITL_FIND(1, 4); else SG_EDITL_FIND(1, 8);
    }
#undef SG_EDITL_FIND
    return hipGetLastError();
}

// match_calls.cpp reaches the launchers once this unit is part of the program (peditl.hpp)
namespace {
struct RegisterPlanesEditl {
    RegisterPlanesEditl()
    {
        g_planes_editl_scan = &launch_planes_editl_scan;
        g_planes_editl_find = &launch_planes_editl_find;
    }
} g_register_planes_editl;
}  // namespace

}  // namespace sg
