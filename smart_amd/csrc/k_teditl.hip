// k_teditl.hip — byte texts: text_editl_scan / text_editl_find, occurrences within EDIT distance k of patterns up to 256
// bytes, k up to 31, by Myers' bit-vector recurrence in blocks of 32 rows with Ukkonen's cut-off (edit_block.hpp)
// (one translation unit per kernel family: dev_common.hpp; the interface: teditl.hpp; the geometry and the masks: teditl_host.hpp)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "teditl.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// text_editl_scan<WORDS> counts, text_editl_find<WORDS> lists the END positions e in [e_begin, e_end) with D(e) <= k, D as
// k_tedit.hip defines it: the last row of Sellers' DP on the range alone.  WORDS = 2, 4 or 8 dwords hold the column of a
// pattern of at most 32 WORDS bytes.  Two halves that exist elsewhere meet here.
//
// THE RECURRENCE is k_peditl.hip's, unchanged: the blocks, the cut-off rule and the one kept score of edit_block.hpp, and how
// a wave runs them — B, the number of active blocks, is the WAVE's, a scalar, so that the unrolled blocks are skipped by
// scalar branches and pv / mv are indexed by constants only (no scratch); the wave grows when ANY of its lanes asks for it
// and shrinks when ALL agree; one grow per column; a hit is reported only with B == W.  That header comment says why the
// answers are exact and why a lane may carry more blocks than it needs.  With all_blocks set B is W throughout.
//
// THE FEEDING is k_tedit.hip's: a byte selects one of 256 masks in LDS (editl_peq_bytes / editl_peq_classes: the kernels do
// not know a class pattern from a byte pattern), here WORD-MAJOR — dword w of byte v at peq[256 w + v], one ds_read_b32 per
// ACTIVE block, on bank v mod 32 whatever w is; and the text is parked in LDS by coalesced loads, in rows of 132 bytes that
// keep the lanes of a group of 32 on distinct banks (text_tile.hpp's row).
//
// GEOMETRY.  A lane owns kTEditlRun = 512 consecutive end positions (a run of 128 would walk up to 3.2 bytes per owned one
// at m + k = 287; this one 1.56), the 256 lanes of a workgroup a SUPER-TILE of 128 KiB; workgroup t takes the super-tiles t,
// t + gridDim.x, ... below editl_tile_count.  A super-tile is walked in TRIPS: in trip j every lane's PIECE j — the 128
// bytes at base + 512 lane + 128 j — is parked in the lane's own row: eight consecutive lanes load one 128-byte line
// (ld_stream16), chunk q goes to row q / 8, chunk q % 8 of it, as four dword stores (TextTile::park's pattern: dword i on
// bank (r + 4 c + i) mod 32, conflict-free); then every lane walks its row, four steps per dword read.  Pieces 0 .. 3 are
// owned; pieces j0 .. -1, j0 = -ceil((m + k) / 128) >= -3, are the warm-up — the neighbour's last pieces, addressed by the
// same formula with a negative j, so no extra row is needed.  The column (pv, mv, bot; B) stays in registers across a
// super-tile's trips.  It is fresh (block_fresh) at each super-tile's first trip, and again at a lane's own `first`
// (editl_run_walk): for all lanes but those of the range's first two runs that is the byte m + k before the run, the first
// byte any lane walks; a lane whose start is clipped at e_begin begins later than its neighbours, on the B blocks the wave
// has by then, and takes no part in the votes before.  Why the fresh start is EXACT: k_pedit.hip's header comment.
//
// BARRIERS (text_tile.hpp has the rule).  Two __syncthreads() per trip: before the rows are overwritten, after they are
// written.  A workgroup's trips are editl_tile_count's super-tiles of its blockIdx, times (4 - j0): functions of blockIdx,
// gridDim and the kernel arguments only, and the same count sizes the grid.  A wave that has nothing to walk in a trip still
// parks its chunks and arrives at both barriers; the walk, its skip (per WAVE) and the find's output stage all stand
// behind the trip's second barrier and lead to the next trip's first one.  flush_hits' two barriers come after the loops.
//
// VOTES.  All 64 lanes of a wave take every step of a trip's walk, so that __any / __all of the grow and the shrink and the
// shuffles of wave_reserve see whole waves.  A lane outside the range, before its `first` or behind its `last` steps on
// whatever its row holds and votes neutrally — false for the grow, true for the shrink —, is never a hit, and is fresh
// again before any value of it counts.
//
// BOUNDS: none are checked.  The first warm-up piece of the text's first run begins 384 bytes below text byte 0 (kFrontPad
// lies there), the last super-tile ends less than 128 KiB behind e_end <= n (kBackPad lies there); teditl.hpp asserts
// both.  What is read outside [e_begin, e_end) is parked and never part of an answer: act is false there.
//
// The find's output stage is planes_editl_body's: a hit mask and five bit-sliced distance dwords per 32 owned positions, a
// wave's slots from wave_reserve (ONE atomicAdd on the cursor), ordinary vector stores of (e << kTEditlShift) | D(e) while
// slot < cap.  The entries reach the host in no order; it sorts them.  No static LDS, no scratch.
//
// Measured (1 GiB of rand128, English and rand4, profiles/tedit/RESULTS.md, "Long patterns"): the scan takes 1.59-1.68 ms at
// m = 64, 1.77-1.99 ms at m = 65, 100, 2.73-2.89 ms at m = 150, 3.15-3.42 ms at m = 256 for k <= 7, up to 5.19 ms at m = 256,
// k = 31; with all_blocks 1.94-7.96 ms, 2.26-2.45 x the cut-off form at m = 256, k <= 7 and 0.85-0.87 x where every block is
// active anyway (m = 64, k = 31).  1.12-1.16 x text_edit_scan at m = 64, k <= 7; 1.08-1.29 x planes_editl_scan on the same rand4
// bytes packed at k <= 7 (the warm-up pieces are parked whole for every lane).  The step from m = 100 to m = 150 (1.45 x)
// coincides with WORDS = 8 running 3 workgroups per CU instead of 4.  Other run and piece lengths, a prefetch of the next
// piece and the occupancy: not tried.
// ---------------------------------------------------------------------------
static_assert(kTEditlMaxK < 32, "one grow per column: a fresh block's bottom is more than k above the block before it");

// Trip j of the super-tile whose first run begins at src0: every lane's piece j into its row.  Chunk q = tid + 256 i of the
// 2048 lies at src0 + 512 (q / 8) + 128 j + 16 (q % 8); all loads are issued before the stores.
static __device__ __forceinline__ void teditl_park(const uint8_t* src0, int j, uint8_t* rows, uint32_t tid)
{
    const uint8_t* const src = src0 + (long long)j * (long long)kTEditlPiece;
    uint4 v[8];
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t q = tid + (uint32_t)kTEditlT * i;
        v[i] = ld_stream16(src + (size_t)(q >> 3) * kTEditlRun + (q & 7u) * 16u);
    }
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t q = tid + (uint32_t)kTEditlT * i;
        uint32_t* d = reinterpret_cast<uint32_t*>(rows + (q >> 3) * kTEditlRowBytes + (q & 7u) * 16u);
        d[0] = v[i].x; d[1] = v[i].y; d[2] = v[i].z; d[3] = v[i].w;
    }
}

template <int WORDS, bool FIND>
static __device__ __forceinline__ void text_editl_body(const TextEditlArgs& a, uint8_t* smem, unsigned long long* __restrict__ out,
                                                       unsigned long long cap)
{
    constexpr int GROUPS = FIND ? (int)kTEditlPiece / 32 : 1;  // the find keeps its hits per 32 positions; the count needs no such split
    constexpr int GROUP_DW = (int)kTEditlPiece / 4 / GROUPS;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t mk = a.m + a.k, W = (a.m + 31u) / 32u;
    const bool cut = a.all_blocks == 0u;
    uint32_t* const peq = reinterpret_cast<uint32_t*>(smem + kTEditlMasksOff);
    uint8_t* const rows = smem + teditl_rows_off(WORDS);
    const uint32_t* const row = reinterpret_cast<const uint32_t*>(rows) + kTEditlRowDw * tid;  // this lane's piece
#pragma unroll
    for (int w = 0; w < WORDS; ++w) peq[tid + kTEditlT * w] = a.peq[tid + kTEditlT * w];  // (read behind the first trip's barriers)

    const uint64_t c0 = a.e_begin / kTEditlRun;
    const uint64_t ntiles = editl_tile_count(a.e_begin, a.e_end);  // the grid's own count (BARRIERS)
    const int j0 = editl_first_piece(mk);                          // the first trip of every super-tile
    const int x0 = -(int)mk;                                       // the first byte any lane walks, relative to its run
    uint32_t hits = 0;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t c = c0 + t * kTEditlLanes + tid;
        const EditlWalk wk = editl_run_walk(c, a.e_begin, a.e_end, mk);
        const int first = wk.first, last = wk.last;
        const uint8_t* const src0 = a.text + (c0 + t * kTEditlLanes) * kTEditlRun;
        uint32_t pv[WORDS], mv[WORDS];
        int bot;
        uint32_t B = cut ? 1u : W;
        block_fresh<WORDS>(pv, mv, B, a.m, bot);
        for (int j = j0; j < (int)kTEditlPieces; ++j) {
            __syncthreads();  // every lane is done with the piece before
            teditl_park(src0, j, rows, tid);
            __syncthreads();
            const int xj = j * (int)kTEditlPiece;
            const int xlo = x0 > xj ? x0 : xj;
            if (!__any(first < xj + (int)kTEditlPiece && last > xlo)) continue;  // (per WAVE, to the next trip's first barrier)
            const bool owned = j >= 0;
            const int dlo = (xlo - xj) >> 2;  // the first dword of the piece that holds a walked byte: 0 but in trip j0
#pragma unroll 1
            for (int g = 0; g < GROUPS; ++g) {
                uint32_t M = 0, D[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll 1
                for (int d = GROUP_DW * g > dlo ? GROUP_DW * g : dlo; d < GROUP_DW * (g + 1); ++d) {
                    uint32_t w = row[d];
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int x = xj + 4 * d + b;
                        if (__any(x == first)) {  // (rare: the wave's first column, and starts clipped at e_begin, later than the wave's)
                            if (x == first) block_fresh<WORDS>(pv, mv, B, a.m, bot);
                        }
                        const bool act = (uint32_t)(x - first) < (uint32_t)(last - first);
                        if (cut && B < W && __any(act && block_wants_grow(bot, a.k))) block_grow<WORDS>(pv, mv, B, a.m, bot);
                        const uint32_t* const eq = peq + (w & 255u);
                        bot += block_step<WORDS>(pv, mv, [&](int blk) { return eq[256 * blk]; }, B, a.m);  // (the active blocks' dwords only)
                        if (cut)
                            while (B > 1u && __all(!act || block_may_shrink(bot, a.k, B, a.m))) block_shrink<WORDS>(pv, mv, B, a.m, bot);
                        const bool hit = act && owned && B == W && bot <= (int)a.k;
                        if constexpr (!FIND) {
                            hits += hit;
                        } else {
                            const uint32_t h = hit ? 1u << ((4 * d + b) & 31) : 0u;
                            M |= h;
#pragma unroll
                            for (int s = 0; s < 5; ++s) D[s] |= (bot >> s & 1) ? h : 0u;
                        }
                        w >>= 8;
                    }
                }
                if constexpr (FIND) {
                    if (!__any(M != 0u)) continue;  // (per wave; no barrier stands inside the walk)
                    // planes_find's output stage: wave-wide exclusive prefix sum of the lanes' counts, one atomic, the lanes' stores
                    const uint32_t mine = __builtin_popcount(M);
                    unsigned long long slot = wave_reserve(mine, a.count, lane);
                    const uint64_t pos = c * kTEditlRun + (uint64_t)(xj + 32 * g);  // (hits lie in owned pieces: xj >= 0)
                    uint32_t r = M;
                    while (r) {
                        const uint32_t i = __builtin_ctz(r);
                        r &= r - 1;
                        const uint32_t dist = ((D[0] >> i) & 1u) | ((D[1] >> i) & 1u) << 1 | ((D[2] >> i) & 1u) << 2 | ((D[3] >> i) & 1u) << 3 |
                                              ((D[4] >> i) & 1u) << 4;
                        if (slot < cap) out[slot] = (pos + i) << kTEditlShift | dist;
                        ++slot;
                    }
                }
            }
        }
    }
    if constexpr (!FIND) flush_hits(hits, a.count, smem, a.text);
}

template <int WORDS>
__global__ __launch_bounds__(kTEditlT, teditl_wgs(WORDS)) void text_editl_scan(TextEditlArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // teditl_lds_bytes(WORDS)
    text_editl_body<WORDS, false>(a, smem, nullptr, 0);
}

template <int WORDS>
__global__ __launch_bounds__(kTEditlT, teditl_wgs(WORDS)) void text_editl_find(TextEditlArgs a, unsigned long long* __restrict__ out, unsigned long long cap)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // teditl_lds_bytes(WORDS)
    text_editl_body<WORDS, true>(a, smem, out, cap);
}

static bool teditl_args_ok(const TextEditlArgs& a) { return a.m >= 1 && a.m <= kTEditlMaxM && a.k <= kTEditlMaxK && a.text && a.peq; }

static int teditl_words(uint32_t m) { return m <= 64 ? 2 : m <= 128 ? 4 : 8; }

// One workgroup per super-tile, at most what the LDS lets a CU hold: editl_tile_count is the kernels' trip count too.
static uint32_t teditl_grid(const TextEditlArgs& a, int words, int num_cus)
{
    return (uint32_t)std::min<uint64_t>(editl_tile_count(a.e_begin, a.e_end), (uint64_t)num_cus * teditl_wgs(words));
}

static hipError_t launch_text_editl_scan(const TextEditlArgs& a, int num_cus, hipStream_t stream)
{
    if (!teditl_args_ok(a)) return hipErrorInvalidValue;
    if (a.e_end <= a.e_begin) return hipSuccess;
    const int words = teditl_words(a.m);
    const uint32_t grid = teditl_grid(a, words, num_cus);
#define SG_TEDITL_SCAN(w_) hipLaunchKernelGGL((text_editl_scan<w_>), dim3(grid), dim3(kTEditlT), teditl_lds_bytes(w_), stream, a)
    if (words == 2) SG_TEDITL_SCAN(2); else if (words == 4) SG_TEDITL_SCAN(4); else SG_TEDITL_SCAN(8);
#undef SG_TEDITL_SCAN
    return hipGetLastError();
}

static hipError_t launch_text_editl_find(const TextEditlArgs& a, unsigned long long* out, unsigned long long cap, int num_cus, hipStream_t stream)
{
    if (!teditl_args_ok(a)) return hipErrorInvalidValue;
    if (a.e_end <= a.e_begin) return hipSuccess;
    const int words = teditl_words(a.m);
    const uint32_t grid = teditl_grid(a, words, num_cus);
#define SG_TEDITL_FIND(w_) hipLaunchKernelGGL((text_editl_find<w_>), dim3(grid), dim3(kTEditlT), teditl_lds_bytes(w_), stream, a, out, cap)
    if (words == 2) SG_TEDITL_FIND(2); else if (words == 4) SG_TEDITL_FIND(4); else SG_TEDITL_FIND(8);
#undef SG_TEDITL_FIND
    return hipGetLastError();
}

// match_calls.cpp reaches the launchers once this unit is part of the program (teditl.hpp)
namespace {
struct RegisterTextEditl {
    RegisterTextEditl()
    {
        g_text_editl_scan = &launch_text_editl_scan;
        g_text_editl_find = &launch_text_editl_find;
    }
} g_register_text_editl;
}  // namespace

}  // namespace sg
