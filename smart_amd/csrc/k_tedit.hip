// k_tedit.hip — byte texts: text_edit_scan / text_edit_find, occurrences within EDIT distance k (unit-cost substitutions,
// insertions, deletions) by Myers' bit-vector recurrence in Hyyrö's search form (edit_step.hpp)
// (one translation unit per kernel family: dev_common.hpp; the interface: tedit.hpp; the geometry and the masks: tedit_host.hpp)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "tedit.hpp"

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
// THE TEXT.  A lane owns kTEditRun = 128 consecutive end positions, lane l of a wave the l-th run of 64 (a wave:
// kFindSpan bytes, so the find's entries are the spans order_spans orders), the four waves of a workgroup four
// consecutive spans: a TILE of 32 KiB.  128 bytes per lane is a cache line per lane, so the tile comes into LDS with
// coalesced 16-byte loads (ld_stream16: 1 KiB per wave and instruction) together with the run before it — 257 runs —,
// and every lane then walks its run out of LDS, one dword read per four steps.  The up to m + k <= 71 bytes before a
// lane's run, which it walks without counting, are the end of its neighbour's row.
//   * LDS layout: [128 bytes: flush_hits][256 x WORDS dwords: peq][257 rows of kRowBytes = 132 bytes: the tile].
//     Run r of the tile (r = 0: the one before it) is row r: 128 bytes of text and 4 never written.
//   * Banks.  ds_read_b32 serves a wave in two groups of 32 lanes, bank = dword address mod 32.  Unpadded, lane l's t-th
//     dword is dword 32 l + t: ONE bank for the whole group, a 32-way conflict on every read.  With rows of 33 dwords it
//     is dword 33 l + t, bank (l + t) mod 32: the 32 lanes of a group on 32 distinct banks, in the warm-up too (the
//     neighbour's row: dword 33 l + t - 1).
//   * The tile's stores: chunk q (16 bytes) goes to row q / 8, chunk c = q % 8 of it, as four dword stores; dword i of it
//     is on bank (r + 4 c + i) mod 32, and the 32 lanes of a group hold four consecutive rows and all eight chunks of
//     each: r + 4 c takes 32 distinct values, so the stores are conflict-free as well.
//   * Bounds: none are checked.  The tile begins at most 128 bytes below text byte 0 (kFrontPad lies there) and ends less
//     than kTEditTile bytes behind e_end <= n (kBackPad lies there); what is read outside [e_begin, e_end) is parked and
//     never walked (edit_run_walk).  Both are asserted below.
//
// The recurrence, the fresh start at max(e_begin, first owned - (m + k)) and why it is EXACT: k_pedit.hip's header comment,
// word for word with "byte" for "symbol".  In short: a fresh column is never below the true one and the recurrence is
// monotone in its left column, so a lane's values are >= the true ones; an alignment of cost <= k ends at e and consumes at
// most m + k bytes, so it lies inside what the lane walked and its value is also <= the true one; hence every value <= k is
// true and a value > k is truly > k; a start clipped at e_begin is the definition itself.
//
// BARRIERS.  The tile loop holds two __syncthreads() per trip (before the tile is overwritten, after it is written).  Its
// trip count is tiles blockIdx.x, blockIdx.x + gridDim.x, ... below ntiles, and ntiles is computed from e_begin and e_end
// alone: a function of blockIdx, gridDim and the kernel arguments, the same for all 256 lanes of a workgroup.  Nothing
// between the barriers leaves the loop or skips a trip: a lane whose run lies outside the range gets an empty walk from
// edit_run_walk and still stores its chunks and arrives; the find's output stage `continue`s per WAVE, but only to the
// next trip's first barrier, which every wave reaches.  flush_hits' own two barriers come after the loop, where all
// lanes arrive.  (planes_edit_body's loop runs on the WAVE's own count; it holds no barrier.  Here that would hang.)
//
// The find's output stage is planes_edit_body's: a hit mask and three bit-sliced distance dwords per 32 owned positions,
// a wave-wide prefix sum, ONE atomicAdd on the cursor by lane 0, ordinary vector stores of (e << kMisShift) | D(e) while
// slot < cap.  No scratch, no static LDS.
// ---------------------------------------------------------------------------
constexpr int kTEditT = 256;
constexpr int kTEditWgs = 4;                                   // workgroups per CU: 160 KiB of LDS / 35.3 KiB
constexpr uint32_t kTEditTile = kTEditT * kTEditRun;           // bytes of text a workgroup owns per trip
#ifndef SMARTGPU_TEDIT_ROW_PAD
#define SMARTGPU_TEDIT_ROW_PAD 4   // bytes behind a row's 128 (variant builds: 0 is the unpadded tile, tools/tedit_probe.py stride)
#endif
constexpr uint32_t kRowBytes = kTEditRun + SMARTGPU_TEDIT_ROW_PAD, kRowDw = kRowBytes / 4;
constexpr int kPadDw = SMARTGPU_TEDIT_ROW_PAD / 4;           // dwords between a row's last byte and the next row's first
constexpr uint32_t kTileRows = kTEditT + 1;                    // the run before the tile: the first lane's warm-up
constexpr uint32_t kTileChunks = kTileRows * (kTEditRun / 16); // 16-byte chunks parked per trip
constexpr uint32_t kPeqOff = 128;                              // behind flush_hits' 128 bytes
static_assert(kTEditRun >= kTEditMaxM + SMARTGPU_PMIS_MAX, "the warm-up of the longest pattern at the largest k lies in the neighbour's row");
static_assert(SMARTGPU_TEDIT_ROW_PAD % 4 == 0 && (SMARTGPU_TEDIT_ROW_PAD != 4 || kRowDw % 32 == 1), "lanes a row apart sit on neighbouring banks");
static_assert(kFrontPad >= kTEditRun && kFrontPad % 16 == 0, "the run before the first tile lies in the front pad");
static_assert(kBackPad >= kTEditTile, "the last tile ends in the back pad");
static_assert(kTileChunks > 8u * kTEditT && kTileChunks <= 9u * kTEditT, "a tile is parked in nine rounds, the ninth partial");

__host__ __device__ constexpr uint32_t tedit_tile_off(int words) { return kPeqOff + 1024u * words; }
__host__ __device__ constexpr uint32_t tedit_lds_bytes(int words) { return tedit_tile_off(words) + kTileRows * kRowBytes; }
static_assert(kTEditWgs * tedit_lds_bytes(2) <= 160u * 1024u, "four workgroups' LDS on a CU");

template <int WORDS, bool FIND>
static __device__ __forceinline__ void text_edit_body(const TextEditArgs& a, uint8_t* smem, unsigned long long* __restrict__ out,
                                                      unsigned long long cap)
{
    constexpr int GROUPS = FIND ? kTEditRun / 32 : 1;  // the find keeps its hits per 32 positions; the count needs no such split
    constexpr int WIDTH = kTEditRun / GROUPS;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t mk = a.m + a.k, top = a.m - 1;
    uint32_t* const peq = reinterpret_cast<uint32_t*>(smem + kPeqOff);
    uint8_t* const tile = smem + tedit_tile_off(WORDS);
    // this lane's row, and the dwords it walks: dword j >= 0 of its run at row[j], dword j < 0 (the warm-up) at row[j - kPadDw]: the row before
    const uint32_t* const row = reinterpret_cast<const uint32_t*>(tile) + kRowDw * (tid + 1u);
#pragma unroll
    for (int w = 0; w < WORDS; ++w) peq[tid + kTEditT * w] = a.peq[tid + kTEditT * w];  // (read after the loop's barriers)

    const uint64_t c0 = a.e_begin / kTEditRun;
    const uint64_t ntiles = (a.e_end - c0 * kTEditRun + kTEditTile - 1) / kTEditTile;  // the same for every lane of the grid
    uint32_t hits = 0;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        __syncthreads();  // every lane is done with the tile before
        {
            const uint8_t* src = a.text + c0 * kTEditRun + t * kTEditTile - kTEditRun;
            uint4 v[9];
            v[8] = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) v[i] = ld_stream16(src + 16u * (tid + kTEditT * i));
            if (tid < kTileChunks - 8u * kTEditT) v[8] = ld_stream16(src + 16u * (tid + kTEditT * 8u));
#pragma unroll
            for (uint32_t i = 0; i < 9; ++i) {
                const uint32_t q = tid + kTEditT * i;
                if (i < 8 || q < kTileChunks) {
                    uint32_t* d = reinterpret_cast<uint32_t*>(tile + (q >> 3) * kRowBytes + (q & 7u) * 16u);
                    d[0] = v[i].x; d[1] = v[i].y; d[2] = v[i].z; d[3] = v[i].w;
                }
            }
        }
        __syncthreads();
        const uint64_t c = c0 + t * kTEditT + tid;
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
            uint32_t incl = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d, 64);
                if (lane >= (uint32_t)d) incl += up;
            }
            const uint32_t total = __shfl(incl, 63, 64);
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(a.count, (unsigned long long)total);
            base = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) << 32) |
                   __builtin_amdgcn_readfirstlane((uint32_t)base);
            unsigned long long slot = base + (incl - mine);
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
__global__ __launch_bounds__(kTEditT, kTEditWgs) void text_edit_scan(TextEditArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // tedit_lds_bytes(WORDS)
    text_edit_body<WORDS, false>(a, smem, nullptr, 0);
}

template <int WORDS>
__global__ __launch_bounds__(kTEditT, kTEditWgs) void text_edit_find(TextEditArgs a, unsigned long long* __restrict__ out, unsigned long long cap)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // tedit_lds_bytes(WORDS)
    text_edit_body<WORDS, true>(a, smem, out, cap);
}

static bool tedit_args_ok(const TextEditArgs& a) { return a.m >= 1 && a.m <= kTEditMaxM && a.k <= SMARTGPU_PMIS_MAX && a.text && a.peq; }

static uint32_t text_edit_grid(const TextEditArgs& a, int num_cus)
{
    const uint64_t tiles = (a.e_end - a.e_begin / kTEditRun * kTEditRun + kTEditTile - 1) / kTEditTile;
    return (uint32_t)std::min<uint64_t>(tiles, (uint64_t)num_cus * kTEditWgs);
}

static hipError_t launch_text_edit_scan(const TextEditArgs& a, int num_cus, hipStream_t stream)
{
    if (!tedit_args_ok(a)) return hipErrorInvalidValue;
    if (a.e_end <= a.e_begin) return hipSuccess;
    const uint32_t grid = text_edit_grid(a, num_cus);
    if (a.m <= 32)
        hipLaunchKernelGGL((text_edit_scan<1>), dim3(grid), dim3(kTEditT), tedit_lds_bytes(1), stream, a);
    else
        hipLaunchKernelGGL((text_edit_scan<2>), dim3(grid), dim3(kTEditT), tedit_lds_bytes(2), stream, a);
    return hipGetLastError();
}

static hipError_t launch_text_edit_find(const TextEditArgs& a, unsigned long long* out, unsigned long long cap, int num_cus, hipStream_t stream)
{
    if (!tedit_args_ok(a)) return hipErrorInvalidValue;
    if (a.e_end <= a.e_begin) return hipSuccess;
    const uint32_t grid = text_edit_grid(a, num_cus);
    if (a.m <= 32)
        hipLaunchKernelGGL((text_edit_find<1>), dim3(grid), dim3(kTEditT), tedit_lds_bytes(1), stream, a, out, cap);
    else
        hipLaunchKernelGGL((text_edit_find<2>), dim3(grid), dim3(kTEditT), tedit_lds_bytes(2), stream, a, out, cap);
    return hipGetLastError();
}

// api.cpp reaches the launchers once this unit is part of the program (tedit.hpp)
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
