// k_tedit.hip — byte texts: text_edit_scan / text_edit_find, occurrences within EDIT distance k (unit-cost substitutions,
// insertions, deletions) by Myers' bit-vector recurrence in Hyyrö's search form (edit_step.hpp)
// (one translation unit per kernel family: dev_common.hpp; the interface: tedit.hpp; the run and the masks: tedit_host.hpp; the tile: text_tile.hpp)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "tedit.hpp"
#include "text_tile.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// text_edit_scan<WORDS> counts, text_edit_find<WORDS> lists the END positions e in [e_begin, e_end) with D(e) <= k, D(e) the
// last row of Sellers' DP on the range alone (D[0][*] = 0, D[i][before e_begin] = i): planes_edit_scan's question
// (k_pedit.hip) asked of a text of BYTES, whatever number of values it holds.  Two things differ from that kernel.
//
// THE MASKS.  A byte selects one of 256 masks "which pattern positions accept this value" (edit_peq_bytes /
// edit_peq_classes: the kernels do not know a class pattern from a byte pattern).  The table — 256 x WORDS dwords, 1 or
// 2 KiB — is copied from global memory to LDS once per workgroup, and a step reads peq[byte] with one ds_read_b32 / _b64.
// Lanes that read the same entry are a broadcast; distinct entries on one bank are a conflict, and how many there are
// depends on the text.
//
// THE TEXT.  The tile is text_tile.hpp's, shared with k_tmis.hip: a lane owns kTEditRun = 128 consecutive end positions, a
// workgroup's 256 lanes a TILE of 32 KiB, parked in LDS together with the run before it in rows of 132 bytes; that header
// holds the layout, the banks, the bounds and the BARRIERS rule of the tile loop.  The up to m + k <= 71 bytes before a
// lane's run, which it walks without counting, are the end of its neighbour's row; what is read outside [e_begin, e_end) is
// parked and never walked (edit_run_walk): a lane whose run lies outside the range gets an empty walk and still stores its
// chunks and arrives at the barriers.
//
// The recurrence, the fresh start at max(e_begin, first owned - (m + k)) and why it is EXACT: k_pedit.hip's header comment,
// word for word with "byte" for "symbol".  In short: a fresh column is never below the true one and the recurrence is
// monotone in its left column, so a lane's values are >= the true ones; an alignment of cost <= k ends at e and consumes at
// most m + k bytes, so it lies inside what the lane walked and its value is also <= the true one; hence every value <= k is
// true and a value > k is truly > k; a start clipped at e_begin is the definition itself.
//
// The find's output stage is planes_edit_body's: a hit mask and three bit-sliced distance dwords per 32 owned positions,
// a wave's slots from wave_reserve (ONE atomicAdd on the cursor), ordinary vector stores of (e << kMisShift) | D(e) while
// slot < cap.  Its `continue` is per WAVE and leads to the next trip's first barrier.  No scratch, no static LDS.
// ---------------------------------------------------------------------------
#ifndef SMARTGPU_TEDIT_ROW_PAD
#define SMARTGPU_TEDIT_ROW_PAD 4   // bytes behind a row's 128 (variant builds: 0 is the unpadded tile, tools/tedit_probe.py stride)
#endif
using Tile = TextTile<SMARTGPU_TEDIT_ROW_PAD>;
constexpr int kPadDw = Tile::kPadDw;  // dwords between a row's last byte and the next row's first
static_assert(kTEditRun >= kTEditMaxM + SMARTGPU_PMIS_MAX, "the warm-up of the longest pattern at the largest k lies in the neighbour's row");

template <int WORDS, bool FIND>
static __device__ __forceinline__ void text_edit_body(const TextEditArgs& a, uint8_t* smem, unsigned long long* __restrict__ out,
                                                      unsigned long long cap)
{
    constexpr int GROUPS = FIND ? kTEditRun / 32 : 1;  // the find keeps its hits per 32 positions; the count needs no such split
    constexpr int WIDTH = kTEditRun / GROUPS;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t mk = a.m + a.k, top = a.m - 1;
    uint32_t* const peq = reinterpret_cast<uint32_t*>(smem + kMasksOff);
    uint8_t* const tile = smem + text_tile_off(WORDS);
    // this lane's row, and the dwords it walks: dword j >= 0 of its run at row[j], dword j < 0 (the warm-up) at row[j - kPadDw]: the row before
    const uint32_t* const row = reinterpret_cast<const uint32_t*>(tile) + Tile::kRowDw * (tid + 1u);
    text_table_park<WORDS>(peq, a.peq, tid);

    const uint64_t c0 = a.e_begin / kTEditRun;
    const uint64_t ntiles = text_tile_count(a.e_begin, a.e_end);  // the grid's own count (text_tile.hpp, BARRIERS)
    uint32_t hits = 0;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        __syncthreads();  // every lane is done with the tile before
        Tile::park(a.text + c0 * kTEditRun + t * kTextTile - kTEditRun, tile, tid);
        __syncthreads();
        const uint64_t c = c0 + t * kTextT + tid;
        const EditWalk wk = edit_run_walk(c, a.e_begin, a.e_end, mk);
        uint32_t pv[WORDS], mv[WORDS];
        edit_fresh<WORDS>(pv, mv);
        int score = (int)a.m;
        const auto step = [&](uint32_t byte) {
            uint32_t eq[WORDS];
            if constexpr (WORDS == 1) {
                eq[0] = peq[byte];
            } else {
                const uint2 e = *reinterpret_cast<const uint2*>(peq + 2u * byte);
                eq[0] = e.x;
                eq[1] = e.y;
            }
            score += edit_step<WORDS>(pv, mv, eq, top);
        };
        if (wk.first < 0) {  // the warm-up: bytes [first, 0), not counted; only its first dword can be partial
            int j = wk.first >> 2;
            uint32_t w = row[j - kPadDw] >> (8 * (wk.first & 3));
            for (int b = wk.first & 3; b < 4; ++b) {
                step(w & 255u);
                w >>= 8;
            }
            for (++j; j < 0; ++j) {
                w = row[j - kPadDw];
                step(w & 255u);
                step((w >> 8) & 255u);
                step((w >> 16) & 255u);
                step(w >> 24);
            }
        }
        uint32_t M[GROUPS], D[3][GROUPS];
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            uint32_t mg = 0, d0 = 0, d1 = 0, d2 = 0;
            const auto record = [&](int p) {  // after the step of owned position p
                const bool hit = score <= (int)a.k;
                if constexpr (!FIND) {
                    hits += hit;
                } else {
                    const uint32_t h = hit ? 1u << (p & 31) : 0u;
                    mg |= h;
                    d0 |= (score & 1) ? h : 0u;
                    d1 |= (score & 2) ? h : 0u;
                    d2 |= (score & 4) ? h : 0u;
                }
            };
            const int lo = wk.own > WIDTH * g ? wk.own : WIDTH * g, hi = wk.last < WIDTH * (g + 1) ? wk.last : WIDTH * (g + 1);
            for (int p = lo; p < hi;) {
                if ((p & 3) == 0 && p + 4 <= hi) {  // a whole dword: every trip but those at the edges of the range
                    const uint32_t w = row[p >> 2];
                    step(w & 255u);
                    record(p);
                    step((w >> 8) & 255u);
                    record(p + 1);
                    step((w >> 16) & 255u);
                    record(p + 2);
                    step(w >> 24);
                    record(p + 3);
                    p += 4;
                } else {
                    step((row[p >> 2] >> (8 * (p & 3))) & 255u);
                    record(p);
                    ++p;
                }
            }
            M[g] = mg;
            D[0][g] = d0;
            D[1][g] = d1;
            D[2][g] = d2;
        }
        if constexpr (FIND) {
            uint32_t live = 0;
#pragma unroll
            for (int g = 0; g < GROUPS; ++g) live |= M[g];
            if (!__any(live != 0)) continue;  // (to the next trip's barrier: see BARRIERS)
            // planes_find's output stage: wave-wide exclusive prefix sum of the lanes' counts, one atomic, the lanes' stores
            uint32_t mine = 0;
#pragma unroll
            for (int g = 0; g < GROUPS; ++g) mine += __builtin_popcount(M[g]);
            unsigned long long slot = wave_reserve(mine, a.count, lane);
            const uint64_t pos = c * kTEditRun;
#pragma unroll
            for (int g = 0; g < GROUPS; ++g) {
                uint32_t r = M[g];
                while (r) {
                    const uint32_t i = __builtin_ctz(r);
                    r &= r - 1;
                    const uint32_t dist = ((D[0][g] >> i) & 1u) | ((D[1][g] >> i) & 1u) << 1 | ((D[2][g] >> i) & 1u) << 2;
                    if (slot < cap) out[slot] = (pos + 32 * g + i) << kMisShift | dist;
                    ++slot;
                }
            }
        }
    }
    if constexpr (!FIND) flush_hits(hits, a.count, smem, a.text);
}

template <int WORDS>
__global__ __launch_bounds__(kTextT, kTextWgs) void text_edit_scan(TextEditArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // Tile::lds_bytes(WORDS)
    text_edit_body<WORDS, false>(a, smem, nullptr, 0);
}

template <int WORDS>
__global__ __launch_bounds__(kTextT, kTextWgs) void text_edit_find(TextEditArgs a, unsigned long long* __restrict__ out, unsigned long long cap)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // Tile::lds_bytes(WORDS)
    text_edit_body<WORDS, true>(a, smem, out, cap);
}

static bool tedit_args_ok(const TextEditArgs& a) { return a.m >= 1 && a.m <= kTEditMaxM && a.k <= SMARTGPU_PMIS_MAX && a.text && a.peq; }

static hipError_t launch_text_edit_scan(const TextEditArgs& a, int num_cus, hipStream_t stream)
{
    if (!tedit_args_ok(a)) return hipErrorInvalidValue;
    if (a.e_end <= a.e_begin) return hipSuccess;
    const uint32_t grid = text_tile_grid(a.e_begin, a.e_end, num_cus);
    if (a.m <= 32)
        hipLaunchKernelGGL((text_edit_scan<1>), dim3(grid), dim3(kTextT), Tile::lds_bytes(1), stream, a);
    else
        hipLaunchKernelGGL((text_edit_scan<2>), dim3(grid), dim3(kTextT), Tile::lds_bytes(2), stream, a);
    return hipGetLastError();
}

static hipError_t launch_text_edit_find(const TextEditArgs& a, unsigned long long* out, unsigned long long cap, int num_cus, hipStream_t stream)
{
    if (!tedit_args_ok(a)) return hipErrorInvalidValue;
    if (a.e_end <= a.e_begin) return hipSuccess;
    const uint32_t grid = text_tile_grid(a.e_begin, a.e_end, num_cus);
    if (a.m <= 32)
        hipLaunchKernelGGL((text_edit_find<1>), dim3(grid), dim3(kTextT), Tile::lds_bytes(1), stream, a, out, cap);
    else
        hipLaunchKernelGGL((text_edit_find<2>), dim3(grid), dim3(kTextT), Tile::lds_bytes(2), stream, a, out, cap);
    return hipGetLastError();
}

// match_calls.cpp reaches the launchers once this unit is part of the program (tedit.hpp)
namespace {
struct RegisterTextEdit {
    RegisterTextEdit()
    {
        g_text_edit_scan = &launch_text_edit_scan;
        g_text_edit_find = &launch_text_edit_find;
    }
} g_register_text_edit;
}  // namespace

}  // namespace sg
