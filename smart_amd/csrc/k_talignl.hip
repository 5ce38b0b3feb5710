// k_talignl.hip — byte texts, LONG patterns: text_editl_align, the start position, distance and alignment of edit-distance
// occurrences (m <= 256, k <= 31) whose END positions the caller lists (smartgpu_align_editl64): one WAVE per occurrence, one
// LANE per diagonal of the band |i - j| <= k of edit_align.hpp's reversed matrix (alignl_band.hpp)
// (one translation unit per kernel family: dev_common.hpp; the interface: talignl.hpp; the cell rule and the packing: alignl_band.hpp)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "talignl.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// text_editl_align<WORDS, OPS>.  text_edit_align (k_talign.hip) keeps every column's (Pv, Mv) in LDS for the traceback: at
// m = 256, k = 31 that is 18 KiB per occurrence and a lane per occurrence cannot afford it.  An alignment of cost <= k never
// leaves the 2 k + 1 <= 63 diagonals around the main one, so here a wave takes ONE occurrence, lane l owns the diagonal
// d = j - i = l - 32 (live when |d| <= k), and the wave sweeps the anti-diagonals a = i + j = 0 .. m + ncols: at step a the
// lanes with a = d (mod 2) compute their cell from their own previous value (the diagonal neighbour, step a - 2) and the
// latest values of lanes l + 1 (up) and l - 1 (left), which computed at step a - 1.  alignl_band.hpp says why the band is
// exact for everything <= k, and why the operation recorded when a cell is computed is the one edit_traceback would choose.
//
// GEOMETRY.  256 threads, four waves; a wave strides over the list (entry = workgroup * 4 + wave, then + 4 * grid), the grid
// is bounded by what the CUs hold.  WORDS (2, 4, 8: m <= 64, 128, 256) only sizes the mask table.
//   BARRIER.  The workgroup copies the table — 256 x WORDS dwords, word-major (teditl_host.hpp) — from the arena to LDS once;
//   ONE __syncthreads() stands between that copy and the loop and nothing returns before it.  Inside the loop there is no
//   workgroup barrier: the waves' trip counts differ.  A wave's window and decisions are its own regions, ordered by
//   wavefront-scope fences (wave_sync below): LDS operations of one wave complete in order, the fence keeps the compiler
//   from moving them.
//
// THE WINDOW.  The bytes the band consumes, e - (m + k) + 1 .. e, lie in the kAlignlWinDw = 73 ALIGNED dwords that end with
// text dword e >> 2 (talign_host.hpp's geometry with m + k <= 287).  The wave loads them coalesced, lane l dwords l and
// 64 + l, into its LDS region; column j's byte is taken from there by shift.  For e < 4 * 72 the window reaches into the
// kFrontPad zero bytes below text byte 0: legal to read and never consumed, because the band has at most e - e_begin + 1
// <= e + 1 columns.  Nothing above dword e >> 2 is read: its last byte is at most n + 2, inside kBackPad.  All positions
// are 64-bit.
//
// THE WAVEFRONT.  Neighbours come by DPP wave shifts, one VALU operation each (wave_shl:1: lane l takes lane l + 1's value,
// as k_packed.hip uses it; wave_shr:1 the other way), executed by ALL lanes at the top of every step, outside any divergent
// branch: a shift reads nothing from a lane that is switched off.  A neighbour that is dead (|d +- 1| > k, or beyond the
// wave) counts as kAlignlBig, and so does one that has not started, whose value still is the initial kAlignlBig.  `miss`
// is one LDS read of the table with the byte from the window.  A lane's value at row m is D'[m][m + d]; one wave reduction
// of alignl_key gives the minimum and, among equal minima, the smallest j = J: start = e + 1 - J, or the sentinel when the
// minimum exceeds k.  The trip count m + ncols + 1 and every branch around the shifts are wave-uniform (e travels through
// readfirstlane).
//
// DECISIONS AND TRACEBACK (OPS).  An interior cell's two bits go into a register, sixteen rows per dword, stored to the
// wave's LDS as [row / 16][lane] (17 dwords per lane) when alignl_dec_flush says so.  The walk from (m, J) to (0, 0) is
// wave-uniform and serial: row 0 is 'I', column 0 is 'D', otherwise one broadcast LDS read; lane t / 32 (lanes 0 .. 8) ORs
// operation t into its own word, lane 9 keeps L, and the ten words leave with one coalesced store.  Every step lowers i or
// j, so the walk ends after at most m + J steps whatever the decisions hold; an operation beyond the 288th (none, when
// dist <= k) lands in a lane whose word is not stored or is overwritten by L.  No register array under a run-time index,
// no scratch.  Without OPS the same kernel skips the decision stores and the walk.
//
// LDS, static, per workgroup: [256 x WORDS dwords: the table][4 x 73 dwords: the windows][4 x 17 x 64 dwords: the decisions,
// OPS only]: 2 + 1.1 + 17 KiB to 8 + 1.1 + 17 KiB, within 64 KB, so the launch asks for no attribute.
// ---------------------------------------------------------------------------
constexpr uint32_t kTAlignlT = 256, kTAlignlWaves = kTAlignlT / kAlignlLanes;
template <int WORDS, bool OPS>
struct TextAlignlGeom {
    static constexpr uint32_t kPeqDw = 256 * WORDS;
    static constexpr uint32_t kWinDw = kTAlignlWaves * kAlignlWinDw;
    static constexpr uint32_t kDecWave = kAlignlDecDw * kAlignlLanes;
    static constexpr uint32_t kDecDw = OPS ? kTAlignlWaves * kDecWave : 0;
    static constexpr uint32_t kLdsBytes = 4 * (kPeqDw + kWinDw + kDecDw);
    static constexpr int kWgsPerCu = (int)(160u * 1024u / kLdsBytes) < 8 ? (int)(160u * 1024u / kLdsBytes) : 8;  // 8 x 4 waves: a CU's 32 at <= 128 VGPRs
    static_assert(WORDS == 2 || WORDS == 4 || WORDS == 8, "the table of teditl_host.hpp");
    static_assert(kLdsBytes <= 65536 && kWgsPerCu >= 5, "within 64 KB with no launch attribute; five workgroups or more per CU");
    static_assert(4 * (kAlignlWinDw - 1) <= kFrontPad, "the window of a small e lies in the front pad");
    static_assert(kBackPad >= 4, "the dword of the last byte ends in the back pad");
};

// a wave's LDS traffic stays in program order for the compiler too; no workgroup barrier (the waves' trips differ)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int WORDS, bool OPS>
__global__ __launch_bounds__(kTAlignlT) void text_editl_align(TextAlignlArgs a)
{
    using G = TextAlignlGeom<WORDS, OPS>;
    __shared__ uint32_t peq[G::kPeqDw];
    __shared__ uint32_t wins[G::kWinDw];
    __shared__ uint32_t decs[OPS ? G::kDecDw : 1];
    for (uint32_t i = threadIdx.x; i < G::kPeqDw; i += kTAlignlT) peq[i] = a.peq[i];
    __syncthreads();  // the table is whole; nothing has returned before it, and no workgroup barrier follows

    const uint32_t lane = threadIdx.x & (kAlignlLanes - 1u);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / kAlignlLanes);
    uint32_t* const win = wins + wave * kAlignlWinDw;
    uint32_t* const dec = decs + (OPS ? wave * G::kDecWave : 0u);
    const int d = alignl_diag(lane);
    const bool live = alignl_live(d, a.k);
    const bool up_ok = live && alignl_live(d + 1, a.k), left_ok = live && alignl_live(d - 1, a.k);
    const uint32_t m = a.m, mk = a.m + a.k;
    const uint64_t stride = (uint64_t)gridDim.x * kTAlignlWaves;

    for (uint64_t idx = (uint64_t)blockIdx.x * kTAlignlWaves + wave; idx < a.count; idx += stride) {
        const unsigned long long ev = a.io[idx];  // one address for the wave
        // (readfirstlane returns an int: each half goes through uint32_t, or a low half >= 2^31 would sign-extend over the high one)
        const uint64_t e = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(ev >> 32)) << 32 | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)ev);
        if (e < a.e_begin || e >= a.e_end) {  // the host has refused such a list; never walk outside the range
            if (lane == 0) a.io[idx] = kTextAlignlNone;
            if constexpr (OPS)
                if (lane < kAlignlOpsWords) a.ops[kAlignlOpsWords * idx + lane] = 0;
            continue;
        }
        wave_sync();  // the previous occurrence's reads of the window and the decisions are done
        {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(a.text) + talign_window_first(e, kAlignlWinDw);
            win[lane] = src[lane];
            if (lane < kAlignlWinDw - kAlignlLanes) win[kAlignlLanes + lane] = src[kAlignlLanes + lane];
        }
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
                    const uint32_t wb = talign_window_byte(e, j, kAlignlWinDw);
                    const uint32_t byte = (win[wb >> 2] >> (8u * (wb & 3u))) & 255u;
                    const uint32_t miss = alignl_miss(i, peq[alignl_peq_index(i, byte)]);
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
        if (lane == 0) a.io[idx] = hit ? (unsigned long long)(e + 1 - J) << kTAlignlShift | (unsigned long long)dist : kTextAlignlNone;
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

static hipError_t launch_text_editl_align(const TextAlignlArgs& a, int num_cus, hipStream_t stream)
{
    if (a.m < 1 || a.m > kAlignlMaxM || a.k > kAlignlMaxK || !a.io || !a.text || !a.peq || num_cus < 1) return hipErrorInvalidValue;
    if (a.count == 0) return hipSuccess;
    const uint64_t wgs = (a.count + kTAlignlWaves - 1) / kTAlignlWaves;
#define SG_TALIGNL(w_, o_)                                                                                                         \
    do {                                                                                                                           \
        using G = TextAlignlGeom<w_, o_>;                                                                                          \
        const uint32_t grid = (uint32_t)std::min<uint64_t>(wgs, (uint64_t)num_cus * G::kWgsPerCu);                                 \
        hipLaunchKernelGGL((text_editl_align<w_, o_>), dim3(grid), dim3(kTAlignlT), 0, stream, a);                                 \
    } while (0)
    const bool ops = a.ops != nullptr;
    switch (talignl_words(a.m)) {
    case 2: if (ops) SG_TALIGNL(2, true); else SG_TALIGNL(2, false); break;
    case 4: if (ops) SG_TALIGNL(4, true); else SG_TALIGNL(4, false); break;
    default: if (ops) SG_TALIGNL(8, true); else SG_TALIGNL(8, false); break;
    }
#undef SG_TALIGNL
    return hipGetLastError();
}

// alignl_calls.cpp reaches the launcher once this unit is part of the program (talignl.hpp)
namespace {
struct RegisterTextAlignl {
    RegisterTextAlignl() { g_text_editl_align = &launch_text_editl_align; }
} g_register_text_alignl;
}  // namespace

}  // namespace sg
