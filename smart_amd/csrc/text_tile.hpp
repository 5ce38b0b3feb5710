// text_tile.hpp — byte texts: the tile of text_edit_scan / _find (k_tedit.hip) and text_mis_scan / _find (k_tmis.hip), once:
// its constants, its LDS layout, how many tiles a range has (the kernels' trip count AND the host's grid), the staging of a
// tile and of the 256 masks.  Device code, __forceinline__; the two units keep what is theirs: the walk, the step, what
// they record, their stores.
#pragma once
#include "dev_common.hpp"
#include "tedit_host.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// THE GEOMETRY.  A lane owns kTEditRun = 128 consecutive END positions, lane l of a wave the l-th run of 64 (a wave:
// kFindSpan bytes, so the finds' entries are the spans order_spans orders), the four waves of a workgroup four consecutive
// spans: a TILE of 32 KiB.  128 bytes per lane is a cache line per lane, so the tile comes into LDS with coalesced 16-byte
// loads (ld_stream16: 1 KiB per wave and instruction) together with the run before it — 257 runs —, and every lane then
// walks its run out of LDS, one dword read per four steps.  The bytes before a lane's run that its first windows need
// (at most kTEditRun: each unit asserts its own) are the end of its neighbour's row.
//   * LDS layout: [128 bytes: flush_hits][256 x WORDS dwords: the masks][257 rows of kRowBytes = 132 bytes: the tile].
//     Run r of the tile (r = 0: the one before it) is row r: 128 bytes of text and PAD = 4 never written.
//   * Banks.  ds_read_b32 serves a wave in two groups of 32 lanes, bank = dword address mod 32.  Unpadded, lane l's t-th
//     dword is dword 32 l + t: ONE bank for the whole group, a 32-way conflict on every read.  With rows of 33 dwords it
//     is dword 33 l + t, bank (l + t) mod 32: the 32 lanes of a group on 32 distinct banks, in the warm-up too (the
//     neighbour's row: dword 33 l + t - 1).  The mask lookups are a broadcast or a conflict as the text decides.
//   * The tile's stores: chunk q (16 bytes) goes to row q / 8, chunk c = q % 8 of it, as four dword stores; dword i of it
//     is on bank (r + 4 c + i) mod 32, and the 32 lanes of a group hold four consecutive rows and all eight chunks of
//     each: r + 4 c takes 32 distinct values, so the stores are conflict-free as well.
//   * Bounds: none are checked.  The tile begins at most 128 bytes below text byte 0 (kFrontPad lies there) and ends less
//     than kTextTile bytes behind e_end <= n (kBackPad lies there); what is read outside [e_begin, e_end) is parked and
//     never part of an answer (each unit's walk says why).  Both are asserted below.
//
// BARRIERS.  A kernel's tile loop holds two __syncthreads() per trip (before the tile is overwritten, after it is written).
// Its trips are the tiles blockIdx.x, blockIdx.x + gridDim.x, ... below text_tile_count(e_begin, e_end): a function of
// blockIdx, gridDim and the kernel arguments, the same for all 256 lanes of a workgroup — and the SAME function sizes the
// grid (text_tile_grid), so no workgroup is launched without a trip or left with one nobody takes.  Nothing between the
// barriers may leave the loop or skip a trip: a lane whose run lies outside the range still stores its chunks and arrives;
// a `continue` is per WAVE, stands behind the trip's second barrier and leads only to the next trip's first barrier, which
// every wave reaches.  flush_hits' own two barriers come after the loop, where all lanes arrive.  (planes_edit_body's loop
// runs on the WAVE's own count; it holds no barrier.  Here that would hang.)
// ---------------------------------------------------------------------------
constexpr int kTextT = 256;                                     // lanes of a workgroup
constexpr int kTextWgs = 4;                                     // workgroups per CU: 160 KiB of LDS / 35.3 KiB
constexpr uint32_t kTextTile = kTextT * kTEditRun;              // bytes of text a workgroup owns per trip
constexpr uint32_t kTileRows = kTextT + 1;                      // the run before the tile: the first lane's warm-up
constexpr uint32_t kTileChunks = kTileRows * (kTEditRun / 16);  // 16-byte chunks parked per trip
constexpr uint32_t kMasksOff = 128;                             // the masks: behind flush_hits' 128 bytes
static_assert(kFrontPad >= kTEditRun && kFrontPad % 16 == 0, "the run before the first tile lies in the front pad");
static_assert(kBackPad >= kTextTile, "the last tile ends in the back pad");
static_assert(kTileChunks > 8u * kTextT && kTileChunks <= 9u * kTextT, "a tile is parked in nine rounds, the ninth partial");

__host__ __device__ constexpr uint32_t text_tile_off(int words) { return kMasksOff + 1024u * words; }

// The tiles of [e_begin, e_end): the first begins at the run that holds e_begin.  The same for every lane of the grid.
SG_HOST_DEVICE inline uint64_t text_tile_count(uint64_t e_begin, uint64_t e_end)
{
    return (e_end - e_begin / kTEditRun * kTEditRun + kTextTile - 1) / kTextTile;
}

inline uint32_t text_tile_grid(uint64_t e_begin, uint64_t e_end, int num_cus)
{
    return (uint32_t)std::min<uint64_t>(text_tile_count(e_begin, e_end), (uint64_t)num_cus * kTextWgs);
}

// The rows, PAD bytes behind each row's 128 (4: the product; 0: the unpadded tile of k_tedit's variant build).
template <uint32_t PAD>
struct TextTile {
    static constexpr uint32_t kRowBytes = kTEditRun + PAD, kRowDw = kRowBytes / 4;
    static constexpr int kPadDw = PAD / 4;  // dwords between a row's last byte and the next row's first
    static_assert(PAD % 4 == 0 && (PAD != 4 || kRowDw % 32 == 1), "lanes a row apart sit on neighbouring banks");
    static_assert(kTextWgs * (text_tile_off(2) + kTileRows * kRowBytes) <= 160u * 1024u, "four workgroups' LDS on a CU");

    static __host__ __device__ constexpr uint32_t lds_bytes(int words) { return text_tile_off(words) + kTileRows * kRowBytes; }

    // Park the tile whose row 0 begins at src (the run BEFORE the workgroup's 256): all loads are issued before the stores.
    static __device__ __forceinline__ void park(const uint8_t* src, uint8_t* tile, uint32_t tid)
    {
        uint4 v[9];
        v[8] = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) v[i] = ld_stream16(src + 16u * (tid + kTextT * i));
        if (tid < kTileChunks - 8u * kTextT) v[8] = ld_stream16(src + 16u * (tid + kTextT * 8u));
#pragma unroll
        for (uint32_t i = 0; i < 9; ++i) {
            const uint32_t q = tid + kTextT * i;
            if (i < 8 || q < kTileChunks) {
                uint32_t* d = reinterpret_cast<uint32_t*>(tile + (q >> 3) * kRowBytes + (q & 7u) * 16u);
                d[0] = v[i].x; d[1] = v[i].y; d[2] = v[i].z; d[3] = v[i].w;
            }
        }
    }
};

// The 256 masks of WORDS dwords from global memory to LDS, one entry per lane and word (read after the loop's barriers).
template <int WORDS>
static __device__ __forceinline__ void text_table_park(uint32_t* lds, const uint32_t* table, uint32_t tid)
{
#pragma unroll
    for (int w = 0; w < WORDS; ++w) lds[tid + kTextT * w] = table[tid + kTextT * w];
}

}  // namespace sg
