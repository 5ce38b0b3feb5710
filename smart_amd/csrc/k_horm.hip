// k_horm.hip — hor_multi_scan: Horspool (and Tuned BM) on hor_scan's LDS tiles for up to eight patterns of one length
// in ONE pass over the text (a translation unit of its own: dev_common.hpp says why)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "multi.hpp"

namespace sg {

// Loop states per lane (1, 2 or 4 "chains"): a lane walks ALL its patterns in one loop over (pattern, window end) — see
// the kernel — and a chain is one such walk over a contiguous share of the pass's patterns.  The chains of a lane are
// independent chains of dependent LDS reads (text byte, table entry, add) stepped in one loop body: more of them shorten
// the dependent chain and issue a few more steps (a share that ends early idles).  The default is the measured one
// (profiles/coalesce/RESULTS.md); a macro, as tools/build_variant.sh builds the variants for an A/B.
#ifndef SMARTGPU_HORM_CHAINS
#define SMARTGPU_HORM_CHAINS 1
#endif

// ---------------------------------------------------------------------------
// hor_scan<.., VAR 0> (k_hor.hip) with the tile staged ONCE for np <= NP patterns: searches of one text that are queued
// together (api.cpp) share the fetch and HBM bytes per pattern fall by np.  Same tiles on absolute offsets indexed by
// window end, same back halo, same prefetch one tile ahead, same swizzle, same range clamps.
// LDS: u64 blob[8] | u64 count[8] | u64 hits[8] | np x (u16 tab[256] | pattern tail P[m-1-H..m-1]) | text [tile0-H16, tile0+TB)
// The walk: eight walks of a staged tile cost more than its fetch, so a pass is bound by the walk, and a wave's walk
// lasts as long as its slowest lane's.  A lane therefore holds (pattern g, window end e, table offset) and, when a shift
// takes e past its 64-byte segment, moves on to the next pattern IN THE SAME ITERATION; the loop ends when every lane has
// been through all patterns.  The wave waits for the lane with the longest SUM over the patterns (as hor_flat and bm_scan
// wait for the longest sum over a lane's state), not for the sum over the patterns of the slowest lane of each.
// The arrays of MultiArgs are indexed with compile-time constants only, once, in the prologue that copies the pointers
// to LDS (a run-time index into the arguments makes the compiler select between addresses and load through flat_load);
// a pattern's pointer is read from LDS as a number and cast to GLOBAL memory.  The kernel is as long as hor_scan
// whatever NP is, so NP, the most patterns a pass can take, is instantiated once, at kMultiMax, and completion in
// memory (m - 1 > H) is a run-time branch of that one kernel, taken by rare candidates only: the product library has a
// size to keep (tests/test_abi.py holds it below 0.7 of the A/B build).
// Counts: an occurrence is rare for a streaming pattern (the only kind that gets here), so a lane adds each one straight
// to its pattern's LDS counter, and at the end the workgroup adds every non-zero counter to that pattern's result slot.
// Not through the staging slots of flush_hits: those assume ONE flush per grid, and here a grid flushes np sums.
// ---------------------------------------------------------------------------
constexpr uint32_t kHormHead = 3 * 8 * kMultiMax;  // the three u64 arrays in front of the tables
static_assert(kHormHead % 64 == 0, "the tables and the tile stay 16-byte aligned");

// a pointer into global memory from the number an LDS slot holds (per lane: lanes may ask for different patterns)
__device__ __forceinline__ const uint8_t* horm_global(unsigned long long v)
{
    typedef const __attribute__((address_space(1))) uint8_t* global_u8;
    return (const uint8_t*)reinterpret_cast<global_u8>(v);
}

// a 64-bit value of the first active lane / of lane `src`, wave-uniform.  The halves go through uint32_t: the builtins
// return int, and an int OR-ed into 64 bits is sign-extended — a pointer whose low word has bit 31 set would come out
// with its high word all ones.
__device__ __forceinline__ unsigned long long horm_first(unsigned long long v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long horm_lane(unsigned long long v, int src)
{
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, src), hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

// wave_verify (dev_common.hpp) with the pattern as well as the text pointer taken from the parked lane: the candidates
// a wave has parked may belong to different patterns.  Returns 1 in the lane whose candidate verified, 0 elsewhere.
__device__ __forceinline__ uint32_t horm_wave_verify(bool has, const uint8_t* tptr, const uint8_t* pptr, uint32_t len)
{
    unsigned long long todo = __ballot(has);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t mine = 0;
    while (todo) {
        const int src = __builtin_ctzll(todo);  // wave-uniform
        todo &= todo - 1;
        const uint8_t* t = horm_global(horm_lane((unsigned long long)tptr, src));
        const uint8_t* p = horm_global(horm_lane((unsigned long long)pptr, src));
        bool diff = false;
        for (uint32_t off = lane * 16u; off < len; off += 1024u)
            diff |= differ16(t + off, p + off, len - off < 16 ? len - off : 16u);
        if (!__any(diff) && lane == (uint32_t)src) mine = 1;
    }
    return mine;
}

template <int THREADS, int L, int NP>
__global__ __launch_bounds__(THREADS) void hor_multi_scan(MultiArgs a, uint64_t tile_first, uint32_t ntiles)
{
    constexpr int TB = THREADS * L;
    constexpr int C = SMARTGPU_HORM_CHAINS;
    static_assert(NP <= kMultiMax && (C == 1 || C == 2 || C == 4), "one, two or four chains");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t m = a.m, H = a.halo, H16 = round16(H), np = a.np;
    const bool in_memory = m - 1 > H;  // windows are completed in HBM
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
        const uint8_t* blob = horm_global(horm_first(blobs[i]));
        uint16_t* tab = reinterpret_cast<uint16_t*>(tabs + i * slot);
        uint8_t* ptail = tabs + i * slot + 512;
        for (uint32_t j = threadIdx.x; j < 256; j += THREADS) tab[j] = reinterpret_cast<const uint16_t*>(blob + kTableOff)[j];
        for (uint32_t j = threadIdx.x; j <= H; j += THREADS) ptail[j] = blob[m - 1 - H + j];
    }
    // chain c walks the patterns [c * share, (c + 1) * share) below np: none for a chain past the last pattern
    const uint32_t share = (np + C - 1) / C;

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
        // the lane's window ends of this tile, [e0, ehi) in tile coordinates; none: the lane starts finished
        const bool any = lo < hi;
        const uint32_t e0 = any ? (uint32_t)(lo - tile0) + H16 : H16;
        const uint32_t ehi = any ? (uint32_t)(hi - tile0) + H16 : H16;
        // the staged tile, walked for all patterns in one loop: per chain the pattern g (up to gend), its window end e
        // and the offset of its table
        uint32_t g[C], gend[C], e[C], tb[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            gend[c] = min((c + 1) * share, np);
            g[c] = any ? min(c * share, np) : gend[c];
            e[c] = e0;
            tb[c] = g[c] * slot;
        }
        bool parked = false;  // first candidate of this tile awaiting the wave-wide compare, and its pattern
        uint32_t parked_g = 0;
        const uint8_t* parked_at = a.text;
        for (;;) {
            bool more = false;
#pragma unroll
            for (int c = 0; c < C; ++c) more |= g[c] < gend[c];
            if (!more) break;
            uint32_t ent[C];
#pragma unroll
            for (int c = 0; c < C; ++c)  // (a finished chain reads some byte of the tile and some entry behind its last table)
                ent[c] = reinterpret_cast<const uint16_t*>(tabs + tb[c])[txt[tile_at(e[c])]];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (C > 1 && g[c] >= gend[c]) continue;
                if ((ent[c] & 0x8000u) != 0) {
                    const uint8_t* ptail = tabs + tb[c] + 512;
                    uint32_t k = 1;  // bytes matched so far, right to left
                    while (k <= H && ptail[H - k] == txt[tile_at(e[c] - k)]) ++k;
                    bool ok = k == H + 1;
                    if (in_memory && ok) {  // the rest of the window is not in LDS
                        const uint8_t* rest = a.text + tile0 + (e[c] - H16) - (m - 1);
                        if (!parked) {
                            parked = true;
                            parked_at = rest;
                            parked_g = g[c];
                            ok = false;  // counted after the loop
                        } else {
                            ok = global_equal(rest, horm_global(blobs[g[c]]), m - 1 - H);
                        }
                    }
                    if (ok) atomicAdd(sums + g[c], 1ull);
                }
                e[c] += ent[c] & 0x7FFFu;
                if (e[c] >= ehi) {  // on to the next pattern, no iteration spent
                    g[c] += 1;
                    e[c] = e0;
                    tb[c] += slot;
                }
            }
        }
        if (in_memory && horm_wave_verify(parked, parked_at, horm_global(blobs[parked_g]), m - 1 - H)) atomicAdd(sums + parked_g, 1ull);
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
    hipLaunchKernelGGL((hor_multi_scan<kHorT, kHorL, kMultiMax>), dim3(grid), dim3(kHorT), lds, stream, a, tr.first, tr.count);
    return hipGetLastError();
}

// api.cpp queues launches only once this unit is part of the program
namespace {
struct RegisterHorMulti {
    RegisterHorMulti() { g_hor_multi = &launch_hor_multi; }
} g_register_hor_multi;
}  // namespace

}  // namespace sg
