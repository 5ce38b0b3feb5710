// k_tmis.hip — byte texts: text_mis_scan / text_mis_find, occurrences with at most k MISMATCHES (substitutions only: the
// Hamming distance of a window of m bytes) by a bit-sliced counter that moves with the text (tmis_host.hpp)
// (one translation unit per kernel family: dev_common.hpp; the interface: tmis.hpp; the masks and the recurrence: tmis_host.hpp; the tile: text_tile.hpp)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "tmis.hpp"
#include "text_tile.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// text_mis_scan<WORDS, BITS> counts, text_mis_find<WORDS, BITS> lists the windows of m bytes that lie in [e_begin, e_end)
// and hold at most k bytes their pattern position does not accept: planes_mis_scan's question (k_planes.hip) asked of a
// text of BYTES.  WORDS = 1 / 2 for m <= 32 / 64, BITS = 1 / 2 / 3 counter planes for k <= 1 / 3 / 7.
//
// THE GEOMETRY is text_edit_scan's, and both units take it from text_tile.hpp: a lane owns kTEditRun = 128 consecutive END
// positions e = s + m - 1, a workgroup's 256 lanes a TILE of 32 KiB, parked in LDS together with the run before it in rows
// of 132 bytes; that header holds the layout, the banks, the bounds and the BARRIERS rule of the tile loop.  The
// m - 1 <= 63 bytes before a lane's run, the part of its first windows that lies in the neighbour's run, are the end of the
// neighbour's row; they are walked without counting.  What is read outside [e_begin, e_end) is parked, at most walked, and
// never part of an answer that is kept (THE WALK).
//
// THE WALK.  edit_run_walk(c, e_begin, e_end, m - 1) says which bytes decide a lane's owned ends: it may start fresh
// (mis_fresh) m - 1 bytes before its first owned end, or at e_begin when that is nearer.  A Hamming window needs exactly its
// own m bytes, so every owned end whose window begins at or behind that start is decided exactly, and walking MORE bytes
// before it changes nothing for them.  The kernels use that: every lane of a workgroup starts at the same dword,
// mis_walk_start(m) bytes before its run, and walks the whole run, so the loop counter is the workgroup's (a scalar), every
// trip is a whole dword, and the step's code stands in the kernel ONCE — twelve instantiations make a large code object.
// What e_begin and e_end clip is decided where an answer is kept: per 32 positions a lane keeps the ends
// [mis_keep_from, last) (mis_group_mask) — the owned ends whose window begins at or behind edit_run_walk's `first`, which is
// the contract: no window begins before e_begin.  A lane at the edge of the range walks bytes it keeps nothing of; a wave
// with no owned end skips the walk.
//
// BARRIERS (text_tile.hpp).  A lane whose run lies outside the range keeps no answer and still stores its chunks and
// arrives; the two `continue`s — a wave with no owned end, the find's wave with no hit — are per WAVE, stand behind the
// trip's second barrier and lead only to the next trip's first barrier, which every wave reaches.
//
// The find's output stage is text_edit_find's: per 32 owned positions a hit mask and the counter planes' top bits, a wave's
// slots from wave_reserve (ONE atomicAdd on the cursor), ordinary vector stores of (e << kMisShift) | distance while
// slot < cap (tmis.hpp: the host turns e into s).  No scratch, no static LDS.
// ---------------------------------------------------------------------------
using Tile = TextTile<4>;  // (k_tedit.hip's variant build without the pad is not this unit's)
constexpr int kPadDw = Tile::kPadDw;  // dwords between a row's last byte and the next row's first
static_assert(Tile::kRowDw % 32 == 1, "lanes a row apart sit on neighbouring banks");

template <int WORDS, int BITS, bool FIND>
static __device__ __forceinline__ void text_mis_body(const TextMisArgs& a, uint8_t* smem, unsigned long long* __restrict__ out,
                                                     unsigned long long cap)
{
    constexpr int GROUPS = kTEditRun / 32;  // answers are kept per 32 positions: the find's four hit masks
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t top = a.m - 1, tb = top & 31u, bias = (1u << BITS) - 1u - a.k;
    uint32_t* const neq = reinterpret_cast<uint32_t*>(smem + kMasksOff);
    uint8_t* const tile = smem + text_tile_off(WORDS);
    // this lane's row, and the dwords it walks: dword j >= 0 of its run at row[j], dword j < 0 (the warm-up) at row[j - kPadDw]: the row before
    const uint32_t* const row = reinterpret_cast<const uint32_t*>(tile) + Tile::kRowDw * (tid + 1u);
    text_table_park<WORDS>(neq, a.neq, tid);

    const uint64_t c0 = a.e_begin / kTEditRun;
    const uint64_t ntiles = text_tile_count(a.e_begin, a.e_end);  // the grid's own count (text_tile.hpp, BARRIERS)
    uint32_t hits = 0;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        __syncthreads();  // every lane is done with the tile before
        Tile::park(a.text + c0 * kTEditRun + t * kTextTile - kTEditRun, tile, tid);
        __syncthreads();
        const uint64_t c = c0 + t * kTextT + tid;
        const EditWalk wk = edit_run_walk(c, a.e_begin, a.e_end, top);
        if (!__any(wk.last > wk.own)) continue;  // a wave outside the range (to the next trip's barrier: see BARRIERS)
        const int lo = mis_keep_from(wk, a.m), hi = wk.last;
        MisState<WORDS, BITS> st;
        mis_fresh(st);
        // the current 32 positions: over budget, and the counter planes' top bits; the find's four groups, oldest first
        uint32_t over = 0, d0 = 0, d1 = 0, d2 = 0;
        uint32_t M[GROUPS], D[3][GROUPS];
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) M[g] = D[0][g] = D[1][g] = D[2][g] = 0;
        const auto step = [&](uint32_t byte, uint32_t at) {  // one byte, and what it says of the window that ends on it
            uint32_t nq[WORDS];
            if constexpr (WORDS == 1) {
                nq[0] = neq[byte];
            } else {
                const uint2 e = *reinterpret_cast<const uint2*>(neq + 2u * byte);
                nq[0] = e.x;
                nq[1] = e.y;
            }
            mis_step<WORDS, BITS>(st, nq, bias);
            over |= ((st.ov[WORDS - 1] >> tb) & 1u) << at;
            if constexpr (FIND) {
                d0 |= ((st.c[0][WORDS - 1] >> tb) & 1u) << at;
                if constexpr (BITS > 1) d1 |= ((st.c[1][WORDS - 1] >> tb) & 1u) << at;
                if constexpr (BITS > 2) d2 |= ((st.c[2][WORDS - 1] >> tb) & 1u) << at;
            }
        };
        // dword j of the run, j < 0 in the row before; the counter is the workgroup's (mis_walk_start), one copy of the step's code
        const int jstart = mis_walk_start(a.m) / 4;
        uint32_t next = row[jstart < 0 ? jstart - kPadDw : jstart];
#pragma unroll 1
        for (int j = jstart; j < (int)(kTEditRun / 4); ++j) {
            const uint32_t w = next;
            next = row[j + 1 < 0 ? j + 1 - kPadDw : j + 1];  // (behind the run: the row's four bytes that are never written, never used)
            if ((j & 7) == 0) over = d0 = d1 = d2 = 0;       // a new group; what the warm-up recorded is dropped here
            const uint32_t at = (4u * (uint32_t)j) & 31u;
            step(w & 255u, at);
            step((w >> 8) & 255u, at + 1);
            step((w >> 16) & 255u, at + 2);
            step(w >> 24, at + 3);
            if ((j & 7) == 7 && j >= 0) {
                const uint32_t mg = ~over & mis_group_mask(lo, hi, j >> 3);
                if constexpr (!FIND) {
                    hits += __builtin_popcount(mg);
                } else {
#pragma unroll
                    for (int g = 0; g + 1 < GROUPS; ++g) {
                        M[g] = M[g + 1];
                        D[0][g] = D[0][g + 1];
                        D[1][g] = D[1][g + 1];
                        D[2][g] = D[2][g + 1];
                    }
                    M[GROUPS - 1] = mg;
                    D[0][GROUPS - 1] = d0;
                    D[1][GROUPS - 1] = d1;
                    D[2][GROUPS - 1] = d2;
                }
            }
        }
        if constexpr (FIND) {
            uint32_t live = 0;
#pragma unroll
            for (int g = 0; g < GROUPS; ++g) live |= M[g];
            if (!__any(live != 0)) continue;  // (to the next trip's barrier: see BARRIERS)
            // text_edit_find's output stage: wave-wide exclusive prefix sum of the lanes' counts, one atomic, the lanes' stores
            uint32_t mine = 0;
#pragma unroll
            for (int g = 0; g < GROUPS; ++g) mine += __builtin_popcount(M[g]);
            unsigned long long slot = wave_reserve(mine, a.count, lane);
            uint64_t pos = c * kTEditRun;
#pragma unroll 1
            for (int g = 0; g < GROUPS; ++g, pos += 32) {  // one copy of the stores' code: the groups move down to M[0]
                uint32_t r = M[0];
                while (r) {
                    const uint32_t i = __builtin_ctz(r);
                    r &= r - 1;
                    // a hit's biased count has not overflowed: it is at least bias
                    const uint32_t dist = (((D[0][0] >> i) & 1u) | ((D[1][0] >> i) & 1u) << 1 | ((D[2][0] >> i) & 1u) << 2) - bias;
                    if (slot < cap) out[slot] = (pos + i) << kMisShift | dist;
                    ++slot;
                }
#pragma unroll
                for (int h = 0; h + 1 < GROUPS; ++h) {
                    M[h] = M[h + 1];
                    D[0][h] = D[0][h + 1];
                    D[1][h] = D[1][h + 1];
                    D[2][h] = D[2][h + 1];
                }
            }
        }
    }
    if constexpr (!FIND) flush_hits(hits, a.count, smem, a.text);
}

template <int WORDS, int BITS>
__global__ __launch_bounds__(kTextT, kTextWgs) void text_mis_scan(TextMisArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // Tile::lds_bytes(WORDS)
    text_mis_body<WORDS, BITS, false>(a, smem, nullptr, 0);
}

template <int WORDS, int BITS>
__global__ __launch_bounds__(kTextT, kTextWgs) void text_mis_find(TextMisArgs a, unsigned long long* __restrict__ out, unsigned long long cap)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // Tile::lds_bytes(WORDS)
    text_mis_body<WORDS, BITS, true>(a, smem, out, cap);
}

static bool tmis_args_ok(const TextMisArgs& a) { return a.m >= 1 && a.m <= kTMisMaxM && a.k <= SMARTGPU_PMIS_MAX && a.text && a.neq; }

template <int WORDS, int BITS>
static void launch_scan_as(const TextMisArgs& a, uint32_t grid, hipStream_t stream)
{
    hipLaunchKernelGGL((text_mis_scan<WORDS, BITS>), dim3(grid), dim3(kTextT), Tile::lds_bytes(WORDS), stream, a);
}

template <int WORDS, int BITS>
static void launch_find_as(const TextMisArgs& a, unsigned long long* out, unsigned long long cap, uint32_t grid, hipStream_t stream)
{
    hipLaunchKernelGGL((text_mis_find<WORDS, BITS>), dim3(grid), dim3(kTextT), Tile::lds_bytes(WORDS), stream, a, out, cap);
}

static hipError_t launch_text_mis_scan(const TextMisArgs& a, int num_cus, hipStream_t stream)
{
    if (!tmis_args_ok(a)) return hipErrorInvalidValue;
    if (a.e_end <= a.e_begin) return hipSuccess;
    const uint32_t grid = text_tile_grid(a.e_begin, a.e_end, num_cus);
    switch (mis_words(a.m) * 10 + mis_bits(a.k)) {
    case 11: launch_scan_as<1, 1>(a, grid, stream); break;
    case 12: launch_scan_as<1, 2>(a, grid, stream); break;
    case 13: launch_scan_as<1, 3>(a, grid, stream); break;
    case 21: launch_scan_as<2, 1>(a, grid, stream); break;
    case 22: launch_scan_as<2, 2>(a, grid, stream); break;
    default: launch_scan_as<2, 3>(a, grid, stream); break;
    }
    return hipGetLastError();
}

static hipError_t launch_text_mis_find(const TextMisArgs& a, unsigned long long* out, unsigned long long cap, int num_cus, hipStream_t stream)
{
    if (!tmis_args_ok(a)) return hipErrorInvalidValue;
    if (a.e_end <= a.e_begin) return hipSuccess;
    const uint32_t grid = text_tile_grid(a.e_begin, a.e_end, num_cus);
    switch (mis_words(a.m) * 10 + mis_bits(a.k)) {
    case 11: launch_find_as<1, 1>(a, out, cap, grid, stream); break;
    case 12: launch_find_as<1, 2>(a, out, cap, grid, stream); break;
    case 13: launch_find_as<1, 3>(a, out, cap, grid, stream); break;
    case 21: launch_find_as<2, 1>(a, out, cap, grid, stream); break;
    case 22: launch_find_as<2, 2>(a, out, cap, grid, stream); break;
    default: launch_find_as<2, 3>(a, out, cap, grid, stream); break;
    }
    return hipGetLastError();
}

// match_calls.cpp reaches the launchers once this unit is part of the program (tmis.hpp)
namespace {
struct RegisterTextMis {
    RegisterTextMis()
    {
        g_text_mis_scan = &launch_text_mis_scan;
        g_text_mis_find = &launch_text_mis_find;
    }
} g_register_text_mis;
}  // namespace

}  // namespace sg
