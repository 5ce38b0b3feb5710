// k_pedit.hip — packed texts: planes_edit_scan / planes_edit_find, occurrences within EDIT distance k (unit-cost
// substitutions, insertions, deletions) by Myers' bit-vector recurrence in Hyyrö's search form (edit_step.hpp)
// (one translation unit per kernel family: dev_common.hpp; the planes' layout: planes.hpp; the interface: pedit.hpp)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "pedit.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// planes_edit_scan<PLANES, WORDS> counts, planes_edit_find<PLANES, WORDS> lists the END positions e in [e_begin, e_end)
// with D(e) <= k, where D(e) = min over e_begin <= s <= e + 1 of the edit distance between the pattern and the symbols
// [s, e]: the last row of Sellers' DP on the range alone, D[0][*] = 0, D[i][before e_begin] = i.
//
// The other plane kernels decide 32 start positions per instruction ACROSS the text; here a column depends on the one
// before it, so a lane WALKS the text, one symbol per step: the column's vertical differences are Pv / Mv, WORDS dwords each
// (WORDS = 1: m <= 32, WORDS = 2: m <= 64, the addition's carry going from dword to dword), the pattern is the four masks
// peq[code] — kernel arguments, wave-uniform —, the symbol's code bits select one of them (no memory lookup), edit_step
// gives the score's change.  A set pattern is another four masks: the kernels do not know the difference.
//
// A lane owns kEditRun = 128 consecutive end positions: four dwords per plane, one non-temporal 16-byte load, lane l of a
// wave the l-th run of 64 — planes_find's geometry.  It starts the recurrence FRESH (D[i] = i: Pv all ones, Mv zero, score m)
// at max(e_begin, first owned - (m + k)) and counts only at owned positions; the up to m + k <= 71 symbols before its run
// lie in the three dwords before it (a second, cached 16-byte load: the neighbour lane's run).
// The fresh start is exact, not approximate:
//   * a fresh column is never below the true one, because the true D[i][c] <= i (delete the first i pattern symbols), and
//     the recurrence is monotone in its left column: every value the lane computes is >= the true one;
//   * an alignment of cost <= k ending at e consumes at most m + k text symbols (m pattern symbols, at most k insertions), so
//     it starts at or after e - (m + k) + 1 >= the lane's first column: the lane's DP, which is the DP on the substring that
//     starts there, contains it — the value is also <= the true one;
//   * so every value <= k is the true value, and a value > k is truly > k;
//   * a start clipped at e_begin is not a warm-up at all: it IS the definition.
// The warm-up makes a lane walk (128 + m + k) / 128 symbols per owned one: 1.07 (m = 8, k = 1) to 1.55 (m = 64, k = 7).
// A longer run would lower that and spread a wave's loads over more cache lines; it was not tried.  Measured with this run
// (1 Gi symbols of rand4, profiles/packed/RESULTS.md, "Edit distance"): 0.90-1.06 ms with WORDS = 1, 1.49-1.81 ms with WORDS = 2.
//
// The find keeps the owned hits as a bit mask M and their distances bit-sliced in three more dwords per 32 positions, and
// runs planes_find's output stage once per wave and row: prefix sum of the lanes' counts, ONE atomicAdd on the cursor,
// ordinary vector stores of (e << kMisShift) | D(e) while slot < cap; entries beyond cap are counted and dropped.  What
// lies in `out` are therefore planes_mis_find's spans, ordered on the host by order_spans.  No LDS, no scratch.
// ---------------------------------------------------------------------------
constexpr int kEditT = 256;
constexpr int kEditWgs = 8;                     // workgroups per CU
constexpr uint32_t kEditDw = kEditRun / 32;     // owned dwords per lane and plane
constexpr uint32_t kEditWarmDw = 3;             // dwords before them that the warm-up may read
constexpr int kEditWarm = 32 * kEditWarmDw;
static_assert(kEditWarm >= (int)(kEditMaxM + SMARTGPU_PMIS_MAX), "the warm-up of the longest pattern at the largest k lies in the dwords a lane loads");
static_assert(kEditWarmDw < kEditDw, "the warm-up dwords come from ONE aligned 16-byte load before the run");
static_assert(kFrontPad >= 16 && kPlaneBackPad >= 16 + 4 * kEditDw, "that load and the last run's stay inside the allocation");

template <int PLANES, int WORDS, bool FIND>
static __device__ __forceinline__ void planes_edit_body(const PlaneEditArgs& a, uint8_t* smem, unsigned long long* __restrict__ out,
                                                        unsigned long long cap)
{
    constexpr int kWalkDw = kEditWarmDw + kEditDw;
    const uint64_t c_end = (a.e_end + kEditRun - 1) / kEditRun;
    const uint64_t stride = (uint64_t)gridDim.x * kEditT;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t mk = a.m + a.k, top = a.m - 1;
    uint32_t hits = 0;
    // the trip count is the WAVE's (its first run decides): every lane stays for the shuffles of the output stage
    for (uint64_t cw = a.e_begin / kEditRun + (uint64_t)blockIdx.x * kEditT + 64u * wave; cw < c_end; cw += stride) {
        const uint64_t c = cw + lane;
        const bool in = c < c_end;
        const uint64_t dw = in ? c * kEditDw : 0;
        uint32_t t0[kWalkDw], t1[kWalkDw];
        {
            const uint4 va = ld_stream16(reinterpret_cast<const uint8_t*>(a.p0 + dw));
            const uint4 ua = *reinterpret_cast<const uint4*>(a.p0 + (dw ? dw - kEditDw : 0));  // (run 0 of the text: not walked)
            t0[0] = ua.y; t0[1] = ua.z; t0[2] = ua.w; t0[3] = va.x; t0[4] = va.y; t0[5] = va.z; t0[6] = va.w;
            if (PLANES == 2) {
                const uint4 vb = ld_stream16(reinterpret_cast<const uint8_t*>(a.p1 + dw));
                const uint4 ub = *reinterpret_cast<const uint4*>(a.p1 + (dw ? dw - kEditDw : 0));
                t1[0] = ub.y; t1[1] = ub.z; t1[2] = ub.w; t1[3] = vb.x; t1[4] = vb.y; t1[5] = vb.z; t1[6] = vb.w;
            }
        }
        // the columns this lane walks, counted from kEditWarm symbols before its run: [first, last); those from kEditWarm on are owned
        int first = 0, last = 0;
        {
            const uint64_t base = c * kEditRun;
            const uint64_t own_lo = base > a.e_begin ? base : a.e_begin, own_hi = base + kEditRun < a.e_end ? base + kEditRun : a.e_end;
            if (in && own_lo < own_hi) {
                const uint64_t start = own_lo - a.e_begin > mk ? own_lo - mk : a.e_begin;
                first = kEditWarm + (int)(long long)(start - base);
                last = kEditWarm + (int)(own_hi - base);
            }
        }
        uint32_t pv[WORDS], mv[WORDS];
        edit_fresh<WORDS>(pv, mv);
        int score = (int)a.m;
        uint32_t M[kEditDw], D[3][kEditDw];
#pragma unroll
        for (uint32_t w = 0; w < kEditDw; ++w) M[w] = D[0][w] = D[1][w] = D[2][w] = 0u;
#pragma unroll
        for (int i = 0; i < kWalkDw; ++i) {
            const int lo = first > 32 * i ? first : 32 * i, hi = last < 32 * i + 32 ? last : 32 * i + 32;
            if (lo >= hi) continue;
            uint32_t w0 = t0[i] >> (lo - 32 * i), w1 = PLANES == 2 ? t1[i] >> (lo - 32 * i) : 0u;
            uint32_t bit = 1u << (lo - 32 * i);
            for (int p = lo; p < hi; ++p) {
                uint32_t eq[WORDS];
#pragma unroll
                for (int w = 0; w < WORDS; ++w) {
                    const uint32_t e01 = (w0 & 1u) ? a.peq[1][w] : a.peq[0][w];
                    eq[w] = PLANES == 2 ? ((w1 & 1u) ? ((w0 & 1u) ? a.peq[3][w] : a.peq[2][w]) : e01) : e01;
                }
                score += edit_step<WORDS>(pv, mv, eq, top);
                if (i >= (int)kEditWarmDw) {  // an owned position
                    const bool hit = score <= (int)a.k;
                    if constexpr (!FIND) {
                        hits += hit;
                    } else {
                        const uint32_t h = hit ? bit : 0u;
                        M[i - kEditWarmDw] |= h;
                        D[0][i - kEditWarmDw] |= (score & 1) ? h : 0u;
                        D[1][i - kEditWarmDw] |= (score & 2) ? h : 0u;
                        D[2][i - kEditWarmDw] |= (score & 4) ? h : 0u;
                    }
                }
                w0 >>= 1;
                w1 >>= 1;
                bit <<= 1;
            }
        }
        if constexpr (FIND) {
            const uint32_t live = M[0] | M[1] | M[2] | M[3];
            if (!__any(live != 0)) continue;
            // planes_find's output stage: wave-wide exclusive prefix sum of the lanes' counts, one atomic, the lanes' stores
            uint32_t mine = 0;
#pragma unroll
            for (uint32_t w = 0; w < kEditDw; ++w) mine += __builtin_popcount(M[w]);
            unsigned long long slot = wave_reserve(mine, a.count, lane);
            const uint64_t pos = c * kEditRun;
#pragma unroll
            for (uint32_t w = 0; w < kEditDw; ++w) {
                uint32_t r = M[w];
                while (r) {
                    const uint32_t i = __builtin_ctz(r);
                    r &= r - 1;
                    const uint32_t dist = ((D[0][w] >> i) & 1u) | ((D[1][w] >> i) & 1u) << 1 | ((D[2][w] >> i) & 1u) << 2;
                    if (slot < cap) out[slot] = (pos + 32 * w + i) << kMisShift | dist;
                    ++slot;
                }
            }
        }
    }
    if constexpr (!FIND) flush_hits(hits, a.count, smem, reinterpret_cast<const uint8_t*>(a.p0));
}

template <int PLANES, int WORDS>
__global__ __launch_bounds__(kEditT, 8) void planes_edit_scan(PlaneEditArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // 128 bytes: flush_hits
    planes_edit_body<PLANES, WORDS, false>(a, smem, nullptr, 0);
}

template <int PLANES, int WORDS>
__global__ __launch_bounds__(kEditT, 8) void planes_edit_find(PlaneEditArgs a, unsigned long long* __restrict__ out, unsigned long long cap)
{
    planes_edit_body<PLANES, WORDS, true>(a, nullptr, out, cap);
}

static bool edit_args_ok(const PlaneEditArgs& a) { return a.m >= 1 && a.m <= kEditMaxM && a.k <= SMARTGPU_PMIS_MAX; }

static uint32_t planes_edit_grid(const PlaneEditArgs& a, int num_cus)
{
    const uint64_t runs = (a.e_end + kEditRun - 1) / kEditRun - a.e_begin / kEditRun;
    return (uint32_t)std::min<uint64_t>((runs + kEditT - 1) / kEditT, (uint64_t)num_cus * kEditWgs);
}

static hipError_t launch_planes_edit_scan(const PlaneEditArgs& a, int planes, int num_cus, hipStream_t stream)
{
    if (!edit_args_ok(a)) return hipErrorInvalidValue;
    if (a.e_end <= a.e_begin) return hipSuccess;
    const uint32_t grid = planes_edit_grid(a, num_cus);
#define SG_EDIT_SCAN(p_, w_) hipLaunchKernelGGL((planes_edit_scan<p_, w_>), dim3(grid), dim3(kEditT), 128, stream, a)
    if (planes == 2) {
        if (a.m <= 32) SG_EDIT_SCAN(2, 1); else SG_EDIT_SCAN(2, 2);
    } else {
        if (a.m <= 32) SG_EDIT_SCAN(1, 1); else SG_EDIT_SCAN(1, 2);
    }
#undef SG_EDIT_SCAN
    return hipGetLastError();
}

static hipError_t launch_planes_edit_find(const PlaneEditArgs& a, unsigned long long* out, unsigned long long cap, int planes, int num_cus,
                                   hipStream_t stream)
{
    if (!edit_args_ok(a)) return hipErrorInvalidValue;
    if (a.e_end <= a.e_begin) return hipSuccess;
    const uint32_t grid = planes_edit_grid(a, num_cus);
#define SG_EDIT_FIND(p_, w_) hipLaunchKernelGGL((planes_edit_find<p_, w_>), dim3(grid), dim3(kEditT), 0, stream, a, out, cap)
    if (planes == 2) {
        if (a.m <= 32) SG_EDIT_FIND(2, 1); else SG_EDIT_FIND(2, 2);
    } else {
        if (a.m <= 32) SG_EDIT_FIND(1, 1); else SG_EDIT_FIND(1, 2);
    }
#undef SG_EDIT_FIND
    return hipGetLastError();
}

// match_calls.cpp reaches the launchers once this unit is part of the program (pedit.hpp)
namespace {
struct RegisterPlanesEdit {
    RegisterPlanesEdit()
    {
        g_planes_edit_scan = &launch_planes_edit_scan;
        g_planes_edit_find = &launch_planes_edit_find;
    }
} g_register_planes_edit;
}  // namespace

}  // namespace sg
