// k_horm.hip — hor_multi_scan: Horspool (and Tuned BM) on hor_scan's LDS tiles for up to eight patterns of one length
// in ONE pass over the text (a translation unit of its own: dev_common.hpp says why)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "multi.hpp"

namespace sg {

// Patterns walked together in one loop (1, 2 or 4): a lane's walk is a chain of dependent LDS reads — text byte, table
// entry, add — and the chains of different patterns over the same staged tile are independent of each other.  One after
// another is the default until a sweep says otherwise (profiles/coalesce/RESULTS.md; a macro, as tools/build_variant.sh
// builds variants for an A/B).
#ifndef SMARTGPU_HORM_IL
#define SMARTGPU_HORM_IL 1
#endif

// ---------------------------------------------------------------------------
// hor_scan<.., VAR 0> (k_hor.hip) with the tile staged ONCE for np <= NP patterns: a streaming scan at m = 32 spends
// its time fetching the tile, not walking it (two LDS reads per window, two to three windows per 64-byte lane segment),
// so searches of one text that are queued together (api.cpp) share the fetch and HBM bytes per pattern fall by np.
// Same tiles on absolute offsets indexed by window end, same back halo, same prefetch one tile ahead, same swizzle,
// same range clamps.
// LDS: u64 blob[8] | u64 count[8] | u64 hits[8] | np x (u16 tab[256] | pattern tail P[m-1-H..m-1]) | text [tile0-H16, tile0+TB)
// The arrays of MultiArgs are indexed with compile-time constants only, once, in the prologue that copies the pointers
// to LDS (a run-time index into the arguments makes the compiler select between addresses and load through flat_load);
// the loop over the patterns is a run-time loop — the kernel is as long as hor_scan whatever NP is — and takes a
// pattern's pointer from LDS as a number, made wave-uniform and cast to GLOBAL memory.  NP, the most patterns a pass can
// take, is therefore instantiated once, at kMultiMax: a kernel per group size would be the same code again, and the
// product library has a size to keep (tests/test_abi.py holds it below 0.7 of the A/B build).
// Counts: an occurrence is rare for a streaming pattern (the only kind that gets here), so a lane adds what it found in
// a tile to its pattern's LDS counter, and at the end the workgroup adds every non-zero counter straight to that
// pattern's result slot.  Not through the staging slots of flush_hits: those assume ONE flush per grid, and here a grid
// flushes np sums.
// ---------------------------------------------------------------------------
constexpr uint32_t kHormHead = 3 * 8 * kMultiMax;  // the three u64 arrays in front of the tables
static_assert(kHormHead % 64 == 0, "the tables and the tile stay 16-byte aligned");

// a wave-uniform pointer into global memory from the number an LDS slot holds
__device__ __forceinline__ const uint8_t* horm_global(const unsigned long long* slot)
{
    const unsigned long long v = *slot;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    typedef const __attribute__((address_space(1))) uint8_t* global_u8;
    return (const uint8_t*)reinterpret_cast<global_u8>(((unsigned long long)hi << 32) | lo);
}

template <int THREADS, int L, bool LONG, int NP>  // LONG: m-1 > back halo, windows are completed in HBM
__global__ __launch_bounds__(THREADS) void hor_multi_scan(MultiArgs a, uint64_t tile_first, uint32_t ntiles)
{
    constexpr int TB = THREADS * L;
    constexpr int IL = SMARTGPU_HORM_IL < NP ? SMARTGPU_HORM_IL : NP;
    static_assert(NP <= kMultiMax && (IL == 1 || IL == 2 || IL == 4) && NP % IL == 0, "groups of IL patterns");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t m = a.m, H = a.halo, H16 = round16(H), np = a.np;
    const uint32_t slot = 512 + round16(H + 1);  // one pattern's tab + ptail; ptail[H-k] == P[m-1-k]
    unsigned long long* blobs = reinterpret_cast<unsigned long long*>(smem);
    unsigned long long* counts = blobs + kMultiMax;
    unsigned long long* sums = counts + kMultiMax;
    uint8_t* tabs = smem + kHormHead;
    uint8_t* txt = tabs + np * slot;  // txt[H16 + x] == T[tile0 + x]

    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            blobs[i] = (uint32_t)i < np ? (unsigned long long)a.blob[i] : 0ull;
            counts[i] = (uint32_t)i < np ? (unsigned long long)a.count[i] : 0ull;
            sums[i] = 0;
        }
    }
    __syncthreads();
    for (uint32_t i = 0; i < np; ++i) {
        const uint8_t* blob = horm_global(blobs + i);
        uint16_t* tab = reinterpret_cast<uint16_t*>(tabs + i * slot);
        uint8_t* ptail = tabs + i * slot + 512;
        for (uint32_t j = threadIdx.x; j < 256; j += THREADS) tab[j] = reinterpret_cast<const uint16_t*>(blob + kTableOff)[j];
        for (uint32_t j = threadIdx.x; j <= H; j += THREADS) ptail[j] = blob[m - 1 - H + j];
    }

    const uint64_t e_begin = a.s_begin + m - 1, e_end = a.s_end + m - 1;
    const uint64_t t_end = tile_first + ntiles;
    static_assert(TB == THREADS * 64, "prefetch registers are written out for L = 64");
    uint4 p0, p1, p2, p3, ph;  // prefetch registers: 4 tile rows + one halo chunk
    const bool halo_lane = threadIdx.x * 16u < H16;
    auto issue = [&](uint64_t tile0) {
        const uint8_t* src = a.text + tile0 + threadIdx.x * 16u;
        p0 = ld_stream16(src);
        p1 = ld_stream16(src + THREADS * 16);
        p2 = ld_stream16(src + THREADS * 32);
        p3 = ld_stream16(src + THREADS * 48);
        if (halo_lane) ph = ld_stream16(src - H16);
    };
    uint64_t t = tile_first + blockIdx.x;
    issue(t * TB);
    for (; t < t_end; t += gridDim.x) {
        const uint64_t tile0 = t * TB;
        __syncthreads();  // previous tile fully consumed (and tables visible)
        {
            const uint32_t i0 = H16 + threadIdx.x * 16u;
            tile_park(txt, i0, p0);
            tile_park(txt, i0 + THREADS * 16, p1);
            tile_park(txt, i0 + THREADS * 32, p2);
            tile_park(txt, i0 + THREADS * 48, p3);
            if (halo_lane) tile_park(txt, threadIdx.x * 16u, ph);
        }
        __syncthreads();
        if (t + gridDim.x < t_end) issue((t + gridDim.x) * TB);
        const uint64_t seg = tile0 + (uint64_t)threadIdx.x * L;
        const uint64_t lo = seg > e_begin ? seg : e_begin;
        const uint64_t hi = seg + L < e_end ? seg + L : e_end;
        // the lane's window ends of this tile, [e0, ehi) in tile coordinates; none: e0 == ehi
        const uint32_t e0 = lo < hi ? (uint32_t)(lo - tile0) + H16 : 0u;
        const uint32_t ehi = lo < hi ? (uint32_t)(hi - tile0) + H16 : 0u;
        // the staged tile, walked once per pattern — IL patterns at a time
        for (uint32_t g = 0; g < np; g += IL) {
            uint32_t e[IL], hits[IL];
            bool parked[IL];  // first candidate of this tile awaiting wave_verify
            const uint8_t* parked_at[IL];
#pragma unroll
            for (int j = 0; j < IL; ++j) {
                e[j] = g + j < np ? e0 : ehi;
                hits[j] = 0;
                parked[j] = false;
                parked_at[j] = a.text;
            }
            for (;;) {
                bool more = false;
#pragma unroll
                for (int j = 0; j < IL; ++j) more |= e[j] < ehi;
                if (!more) break;
                uint32_t ent[IL];
#pragma unroll
                for (int j = 0; j < IL; ++j) {  // (a pattern that has reached the end of the segment re-reads its last byte)
                    const uint32_t at = IL == 1 ? e[j] : min(e[j], ehi - 1u);
                    ent[j] = reinterpret_cast<const uint16_t*>(tabs + (g + j) * slot)[txt[tile_at(at)]];
                }
#pragma unroll
                for (int j = 0; j < IL; ++j) {
                    if ((IL == 1 || e[j] < ehi) && (ent[j] & 0x8000u) != 0) {
                        const uint8_t* ptail = tabs + (g + j) * slot + 512;
                        uint32_t k = 1;  // bytes matched so far, right to left
                        while (k <= H && ptail[H - k] == txt[tile_at(e[j] - k)]) ++k;
                        bool ok = k == H + 1;
                        if (LONG && ok) {  // the rest of the window is not in LDS
                            const uint8_t* rest = a.text + tile0 + (e[j] - H16) - (m - 1);
                            if (!parked[j]) {
                                parked[j] = true;
                                parked_at[j] = rest;
                                ok = false;  // counted by wave_verify below
                            } else {
                                ok = global_equal(rest, horm_global(blobs + g + j), m - 1 - H);
                            }
                        }
                        hits[j] += ok;
                    }
                    e[j] += ent[j] & 0x7FFFu;
                }
            }
#pragma unroll
            for (int j = 0; j < IL; ++j) {
                if (LONG && g + j < np) hits[j] += wave_verify(parked[j], parked_at[j], horm_global(blobs + g + j), m - 1 - H);
                if (hits[j] != 0) atomicAdd(sums + g + j, (unsigned long long)hits[j]);
            }
        }
    }

    // the workgroup's np sums, each straight to its pattern's result slot
    __syncthreads();
    if (threadIdx.x < np && sums[threadIdx.x] != 0) {
        typedef __attribute__((address_space(1))) unsigned long long* global_u64;
        atomicAdd((unsigned long long*)reinterpret_cast<global_u64>(counts[threadIdx.x]), sums[threadIdx.x]);
    }
}

// ---------------------------------------------------------------------------
// launcher: the grid and the tile's LDS as launch_hor's streaming branch, plus the tables of np patterns
// ---------------------------------------------------------------------------
hipError_t launch_hor_multi(const MultiArgs& a, int num_cus, hipStream_t stream)
{
    if (a.np < 1 || a.np > (uint32_t)kMultiMax || a.m < 1 || a.halo > kHaloMax || a.halo > a.m - 1) return hipErrorInvalidValue;
    const uint32_t m = a.m, H = a.halo;
    const TileRange tr = tiles_for(a.s_begin + m - 1, a.s_end + m - 1, (uint64_t)kHorT * kHorL);
    if (tr.count == 0) return hipSuccess;
    const size_t lds = kHormHead + (size_t)a.np * (512 + r16(H + 1)) + ((r16(H) + (size_t)kHorT * kHorL + 16 + 63) & ~(size_t)63);  // whole 64-byte blocks: tile_at() permutes inside them
    // workgroups per CU as a solo launch of one of these patterns (tile_wgs: they are all sparse); smartgpu_tune(4, .) applies
    ScanArgs one = {};
    one.m = m;
    one.sparse = 1;
    const int wgs_per_cu = g_tune[4] ? g_tune[4] : tile_wgs(one);
    uint32_t grid = (uint32_t)num_cus * (uint32_t)wgs_per_cu;
    if (grid > tr.count) grid = tr.count;
    if (m - 1 > H) hipLaunchKernelGGL((hor_multi_scan<kHorT, kHorL, true, kMultiMax>), dim3(grid), dim3(kHorT), lds, stream, a, tr.first, tr.count);
    else hipLaunchKernelGGL((hor_multi_scan<kHorT, kHorL, false, kMultiMax>), dim3(grid), dim3(kHorT), lds, stream, a, tr.first, tr.count);
    return hipGetLastError();
}

// api.cpp queues launches only once this unit is part of the program
namespace {
struct RegisterHorMulti {
    RegisterHorMulti() { g_hor_multi = &launch_hor_multi; }
} g_register_hor_multi;
}  // namespace

}  // namespace sg
