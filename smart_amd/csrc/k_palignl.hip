// k_palignl.hip — packed texts, LONG patterns: planes_editl_align, the start position, distance and alignment of edit-distance
// occurrences (m <= 256, k <= 31) whose END positions the caller lists (smartgpu_palign_editl64): one WAVE per occurrence, one
// LANE per diagonal of the band |i - j| <= k of edit_align.hpp's reversed matrix (alignl_band.hpp)
// (one translation unit per kernel family: dev_common.hpp; the planes' layout: planes.hpp; the interface: palignl.hpp; the cell
// rule and the packing: alignl_band.hpp)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "palignl.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// planes_editl_align<PLANES, OPS>: text_editl_align (k_talignl.hip) on bit planes.  The decomposition, the wavefront, the
// decisions, the key reduction and the walk are that kernel's, and everything a lane decides by itself is alignl_band.hpp's;
// what differs is how a cell learns `miss`.
//
// GEOMETRY.  256 threads, four waves; a wave strides over the list (entry = workgroup * 4 + wave, then + 4 * grid), the grid
// is bounded by what the CUs hold.
//   BARRIER.  The masks of the reversed pattern — four codes x eight dwords, kernel arguments — go to LDS once per workgroup
//   (a lane's (i, code) differ from its neighbours', so the read is indexed per lane; thread t < 32 picks mask dword t by
//   selects of the 32 argument values, never by an index into the argument block); ONE __syncthreads() stands between that
//   copy and the loop and nothing returns before it.  Inside the loop there is no workgroup barrier: the waves' trip counts
//   differ.  A wave's window and decisions are its own regions, ordered by wavefront-scope fences (wave_sync below).
//
// THE WINDOW.  The symbols the band consumes, e - (m + k) + 1 .. e, lie in the kPAlignlWinDw = 10 ALIGNED dwords of each plane
// that end with plane dword e >> 5.  The wave loads them coalesced, lane l < 10 dword l of plane 0, lane 10 + l that of plane
// 1, into its LDS region; column j's code is taken from there by shift.  For e < 32 * 9 the window reaches up to 36 bytes
// below dword 0 of a plane — the front pad below plane 0, plane 0's back pad below plane 1: legal to read and never consumed,
// because the band has at most e - e_begin + 1 <= e + 1 columns.  Nothing above dword e >> 5 is read.  All positions are
// 64-bit.
//
// THE WAVEFRONT, DECISIONS AND TRACEBACK: as k_talignl.hip says them.  `miss` is one LDS read of the masks with the code from
// the window.  No register array under a run-time index, no scratch.
//
// LDS, static, per workgroup: [32 dwords: the masks][4 x 10 x PLANES dwords: the windows][4 x 17 x 64 dwords: the decisions,
// OPS only]: 0.3 to 17.4 KiB, so the launch asks for no attribute.
// ---------------------------------------------------------------------------
constexpr uint32_t kPAlignlT = 256, kPAlignlWaves = kPAlignlT / kAlignlLanes;
template <int PLANES, bool OPS>
struct PlaneAlignlGeom {
    static constexpr uint32_t kPeqDw = 4 * kEditlWords;
    static constexpr uint32_t kWinWave = kPAlignlWinDw * PLANES;
    static constexpr uint32_t kWinDw = kPAlignlWaves * kWinWave;
    static constexpr uint32_t kDecWave = kAlignlDecDw * kAlignlLanes;
    static constexpr uint32_t kDecDw = OPS ? kPAlignlWaves * kDecWave : 0;
    static constexpr uint32_t kLdsBytes = 4 * (kPeqDw + kWinDw + kDecDw);
    static constexpr int kWgsPerCu = (int)(160u * 1024u / kLdsBytes) < 8 ? (int)(160u * 1024u / kLdsBytes) : 8;  // 8 x 4 waves: a CU's 32 at <= 128 VGPRs
    static_assert(PLANES == 1 || PLANES == 2, "one or two planes: three-plane texts are refused by the host");
    static_assert(kPeqDw == 32, "thread t < 32 stages mask dword t");
    static_assert(kLdsBytes <= 65536 && kWgsPerCu == 8, "within 64 KB with no launch attribute; eight workgroups per CU");
    // the window of a small e begins 4 * 9 bytes below dword 0 of its plane: below plane 0 lies the front pad, below plane 1
    // plane 0's back pad (planes.hpp: plane b at b * plane_stride(n), whose tail is kPlaneBackPad zero bytes)
    static_assert(4 * (kPAlignlWinDw - 1) <= kFrontPad && 4 * (kPAlignlWinDw - 1) <= kPlaneBackPad, "the window of a small e lies inside the allocation");
};

// a wave's LDS traffic stays in program order for the compiler too; no workgroup barrier (the waves' trips differ)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int PLANES, bool OPS>
__global__ __launch_bounds__(kPAlignlT) void planes_editl_align(PlaneAlignlArgs a)
{
    using G = PlaneAlignlGeom<PLANES, OPS>;
    __shared__ uint32_t peq[G::kPeqDw];
    __shared__ uint32_t wins[G::kWinDw];
    __shared__ uint32_t decs[OPS ? G::kDecDw : 1];
    {
        uint32_t mine = 0;  // mask dword threadIdx.x, chosen among the 32 argument values
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c)
#pragma unroll
            for (uint32_t w = 0; w < kEditlWords; ++w) mine = threadIdx.x == c * kEditlWords + w ? a.peq[c][w] : mine;
        if (threadIdx.x < G::kPeqDw) peq[threadIdx.x] = mine;
    }
    __syncthreads();  // the masks are whole; nothing has returned before it, and no workgroup barrier follows

    const uint32_t lane = threadIdx.x & (kAlignlLanes - 1u);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / kAlignlLanes);
    uint32_t* const win = wins + wave * G::kWinWave;
    uint32_t* const dec = decs + (OPS ? wave * G::kDecWave : 0u);
    const int d = alignl_diag(lane);
    const bool live = alignl_live(d, a.k);
    const bool up_ok = live && alignl_live(d + 1, a.k), left_ok = live && alignl_live(d - 1, a.k);
    const uint32_t m = a.m, mk = a.m + a.k;
    const uint64_t stride = (uint64_t)gridDim.x * kPAlignlWaves;
    // the lane's share of the window load: lanes 0 .. 9 plane 0, lanes 10 .. 19 plane 1
    const bool loads = lane < G::kWinWave;
    const uint32_t* const plane = PLANES == 2 && lane >= kPAlignlWinDw ? a.p1 : a.p0;
    const uint32_t wdw = PLANES == 2 && lane >= kPAlignlWinDw ? lane - kPAlignlWinDw : lane;

    for (uint64_t idx = (uint64_t)blockIdx.x * kPAlignlWaves + wave; idx < a.count; idx += stride) {
        const unsigned long long ev = a.io[idx];  // one address for the wave
        // (readfirstlane returns an int: each half goes through uint32_t, or a low half >= 2^31 would sign-extend over the high one)
        const uint64_t e = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(ev >> 32)) << 32 | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)ev);
        if (e < a.e_begin || e >= a.e_end) {  // the host has refused such a list; never walk outside the range
            if (lane == 0) a.io[idx] = kPlaneAlignlNone;
            if constexpr (OPS)
                if (lane < kAlignlOpsWords) a.ops[kAlignlOpsWords * idx + lane] = 0;
            continue;
        }
        wave_sync();  // the previous occurrence's reads of the window and the decisions are done
        if (loads) win[lane] = plane[palignl_window_first(e) + (long long)wdw];
        wave_sync();

        const uint32_t ncols = talign_columns(e, a.e_begin, mk);
        uint32_t val = (uint32_t)kAlignlBig, acc = 0, key = kAlignlKeyNone;
        for (uint32_t step = 0; step <= m + ncols; ++step) {
            // every lane, every step: lane l + 1's and lane l - 1's latest values (0 from beyond the wave: never used)
            const uint32_t upv = __builtin_amdgcn_update_dpp(0u, val, 0x130, 0xF, 0xF, true);    // wave_shl:1
            const uint32_t leftv = __builtin_amdgcn_update_dpp(0u, val, 0x138, 0xF, 0xF, true);  // wave_shr:1
            uint32_t i, j;
            if (live && alignl_step_cell(step, d, m, ncols, &i, &j)) {
                uint32_t nv;
                if (i == 0) {
                    nv = j;
                } else if (j == 0) {
                    nv = i;
                } else {
                    const uint32_t wb = palignl_window_bit(e, j);
                    uint32_t code = (win[wb >> 5] >> (wb & 31u)) & 1u;
                    if constexpr (PLANES == 2) code |= ((win[kPAlignlWinDw + (wb >> 5)] >> (wb & 31u)) & 1u) << 1;
                    const uint32_t miss = alignl_miss(i, peq[palignl_peq_index(i, code)]);
                    const AlignlCell c = alignl_cell((int)val, up_ok ? (int)upv : kAlignlBig, left_ok ? (int)leftv : kAlignlBig, miss);
                    nv = (uint32_t)c.value;
                    if constexpr (OPS) {
                        acc |= c.op << alignl_dec_shift(i);
                        if (alignl_dec_flush(i, j, m, ncols)) {
                            dec[alignl_dec_dword(i) * kAlignlLanes + lane] = acc;
                            acc = 0;
                        }
                    }
                }
                val = nv;
                if (i == m) key = alignl_key((int)nv, j);
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)key, s);
            key = other < key ? other : key;
        }
        key = (uint32_t)__builtin_amdgcn_readfirstlane(key);
        const uint32_t dist = alignl_key_dist(key), J = alignl_key_j(key);
        const bool hit = dist <= a.k;
        if (lane == 0) a.io[idx] = hit ? (unsigned long long)(e + 1 - J) << kPAlignlShift | (unsigned long long)dist : kPlaneAlignlNone;
        if constexpr (OPS) {
            unsigned long long word = 0;
            if (hit) {
                wave_sync();  // the lanes' decisions are in LDS
                uint32_t i = m, j = J, t = 0;
                while (i > 0 || j > 0) {
                    uint32_t dec2 = 0;
                    if (i > 0 && j > 0)  // one address for the wave: a broadcast
                        dec2 = (uint32_t)__builtin_amdgcn_readfirstlane(dec[alignl_dec_dword(i) * kAlignlLanes + alignl_dec_lane(i, j)]) >> alignl_dec_shift(i) & 3u;
                    const uint32_t op = alignl_walk_step(&i, &j, dec2);
                    word |= lane == alignl_op_word(t) ? alignl_op_bits(t, op) : 0ull;
                    ++t;
                }
                if (lane == kAlignlOpsWords - 1) word = t;
            }
            if (lane < kAlignlOpsWords) a.ops[kAlignlOpsWords * idx + lane] = word;
        }
    }
}

static hipError_t launch_planes_editl_align(const PlaneAlignlArgs& a, int planes, int num_cus, hipStream_t stream)
{
    if (a.m < 1 || a.m > kAlignlMaxM || a.k > kAlignlMaxK || !a.io || !a.p0 || !a.p1 || planes < 1 || planes > 2 || num_cus < 1) return hipErrorInvalidValue;
    if (a.count == 0) return hipSuccess;
    const uint64_t wgs = (a.count + kPAlignlWaves - 1) / kPAlignlWaves;
#define SG_PALIGNL(p_, o_)                                                                                                         \
    do {                                                                                                                           \
        using G = PlaneAlignlGeom<p_, o_>;                                                                                         \
        const uint32_t grid = (uint32_t)std::min<uint64_t>(wgs, (uint64_t)num_cus * G::kWgsPerCu);                                 \
        hipLaunchKernelGGL((planes_editl_align<p_, o_>), dim3(grid), dim3(kPAlignlT), 0, stream, a);                               \
    } while (0)
    const bool ops = a.ops != nullptr;
    if (planes == 2) { if (ops) SG_PALIGNL(2, true); else SG_PALIGNL(2, false); }
    else             { if (ops) SG_PALIGNL(1, true); else SG_PALIGNL(1, false); }
#undef SG_PALIGNL
    return hipGetLastError();
}

// align_calls.cpp reaches the launcher once this unit is part of the program (palignl.hpp)
namespace {
struct RegisterPlanesAlignl {
    RegisterPlanesAlignl() { g_planes_editl_align = &launch_planes_editl_align; }
} g_register_planes_alignl;
}  // namespace

}  // namespace sg
