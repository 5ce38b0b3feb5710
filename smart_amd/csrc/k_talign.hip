// k_talign.hip — byte texts: text_edit_align, the start position, distance and alignment of edit-distance occurrences whose
// END positions the caller lists (smartgpu_align_edit64): one short backward walk per occurrence with Myers' bit-vector
// recurrence in its DISTANCE form (edit_align.hpp)
// (one translation unit per kernel family: dev_common.hpp; the interface: talign.hpp; the reversal and the window: talign_host.hpp)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "talign.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// text_edit_align<WORDS, OPS>: ONE LANE PER OCCURRENCE, planes_edit_align's walk (k_palign.hip) on a text of BYTES.  A lane
// reads its e, starts fresh (score m: the empty substring) and steps e, e - 1, ... through edit_step_dist with the masks of
// the REVERSED pattern for min(m + k, e - e_begin + 1) columns; it keeps the minimum and the FIRST column J that reaches it:
// D(e) and the largest nearest start e - J + 1.  That many columns decide D(e) <= k exactly (a match within k has at most
// m + k bytes), so a minimum above k makes the entry kTextAlignNone.  With OPS edit_traceback walks the stored columns from
// (m, J) back to (0, 0), which emits the operations in text order.  Two things differ from the planes kernel.
//
// THE MASKS.  A byte selects one of 256 masks (edit_peq_table of the reversed pattern: the kernel does not know a class
// pattern from a byte pattern).  As in k_tedit.hip the table — 256 x WORDS dwords, 1 or 2 KiB — is copied from the arena
// to LDS by the whole workgroup, and a step reads peq[byte] with one ds_read_b32 / _b64; lanes on the same entry are a
// broadcast.  (Reading the arena per step would need no barrier, but puts a dependent global load into every one of up to
// 71 serial steps of a lane; the LDS copy costs the workgroup 4 to 16 loads per lane once.)
//   BARRIER.  The copy needs ONE __syncthreads() between the table's stores and the first step.  Every lane of the
//   workgroup reaches it: a lane with idx >= count, or with an end outside the range, is predicated off (`live`), takes
//   part in the copy, arrives, and only then leaves.  Nothing before the barrier returns.
//
// THE WINDOW.  The bytes a walk consumes, e - (m + k) + 1 .. e, lie in the kDw = talign_window_dwords(WORDS) ALIGNED dwords
// that end with text dword e >> 2 (11 for one mask dword, 19 for two: talign_host.hpp).  The lane loads them with ordinary
// cached loads (they need not coalesce) into LDS as [dword][lane] and takes column j's byte from there by shift; the
// traceback selects a column's Eq again the same way, it is not stored.  For e < 4 (kDw - 1) the window reaches into the
// kFrontPad zero bytes below text byte 0: legal to read and never consumed, because a walk takes at most e - e_begin + 1
// <= e + 1 columns.  Nothing above dword e >> 2 is read: its last byte is at most n + 2, inside kBackPad.
//
// LDS, static, per workgroup: [256 x WORDS dwords: peq][kDw x kLanes dwords: the window][kCols x 2 WORDS x kLanes dwords:
// every column's (Pv, Mv), OPS only].  The window and the columns are [row][lane]: a lane's bank is its lane number whatever
// row it reads, so the divergent reads of the walk and the traceback are conflict-free.  WORDS = 1: 1 + 2.75 + 20 KiB for 64
// occurrences.  WORDS = 2 with OPS at 64 lanes would need 72 KiB of columns, so that form runs 32 OCCURRENCES PER WORKGROUP
// (half a wave): 2 + 2.375 + 36 KiB.  Without OPS: the table and the window, 64 occurrences.  All within 64 KB, so the launch
// asks for no attribute.  No scratch: the masks and the three ops words are selects of computed values, never an array under
// a run-time index.  All positions are 64-bit.
// ---------------------------------------------------------------------------
template <int WORDS, bool OPS>
struct TextAlignGeom {
    static constexpr uint32_t kLanes = (WORDS == 2 && OPS) ? 32 : 64;          // occurrences (threads) per workgroup
    static constexpr uint32_t kCols = WORDS == 2 ? 72 : 40;                     // columns of LDS: >= 32 * WORDS + SMARTGPU_PMIS_MAX
    static constexpr uint32_t kDw = talign_window_dwords(WORDS);                // dwords of a lane's window
    static constexpr uint32_t kPeqDw = 256 * WORDS;
    static constexpr uint32_t kWinDw = kDw * kLanes;
    static constexpr uint32_t kColDw = OPS ? kCols * 2 * WORDS * kLanes : 0;
    static constexpr uint32_t kLdsBytes = 4 * (kPeqDw + kWinDw + kColDw);
    static_assert(kCols >= 32 * WORDS + SMARTGPU_PMIS_MAX, "every column of the longest walk");
    static_assert(4 * (kDw - 1) + 1 >= 32 * WORDS + SMARTGPU_PMIS_MAX && 4 * (kDw - 2) + 1 < 32 * WORDS + SMARTGPU_PMIS_MAX,
                  "the window holds the longest walk at e % 4 == 0, and not a dword more");
    static_assert(kDw == (WORDS == 2 ? 19 : 11), "19 dwords ending at dword e >> 2 for two mask dwords, 11 for one");
    static_assert(kPeqDw * 4 <= 2048 && kWinDw * 4 <= 4864 && kColDw * 4 <= 36864 && kLdsBytes <= 65536,
                  "at most 2 KiB of table, 4.75 KiB of window and 36 KiB of columns: within 64 KB with no launch attribute");
    static_assert(4 * (talign_window_dwords(2) - 1) <= kFrontPad, "the window of a small e lies in the front pad");
    static_assert(kBackPad >= 4, "the dword of the last byte ends in the back pad");
};

template <int WORDS, bool OPS>
__global__ __launch_bounds__((TextAlignGeom<WORDS, OPS>::kLanes)) void text_edit_align(TextAlignArgs a)
{
    using G = TextAlignGeom<WORDS, OPS>;
    __shared__ __attribute__((aligned(16))) uint32_t peq[G::kPeqDw];
    __shared__ uint32_t win[G::kWinDw];
    __shared__ uint32_t cols[OPS ? G::kColDw : 1];
    const uint32_t lane = threadIdx.x;
    const uint64_t idx = (uint64_t)blockIdx.x * G::kLanes + lane;
    for (uint32_t i = lane; i < G::kPeqDw; i += G::kLanes) peq[i] = a.peq[i];

    bool live = idx < a.count;  // (no return before the barrier: see BARRIER)
    uint64_t e = 0;
    if (live) {
        e = a.io[idx];
        if (e < a.e_begin || e >= a.e_end) {  // the host has refused such a list; never walk outside the range
            a.io[idx] = kTextAlignNone;
            if constexpr (OPS) a.ops[3 * idx] = a.ops[3 * idx + 1] = a.ops[3 * idx + 2] = 0;
            live = false;
        }
    }
    if (live) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.text) + talign_window_first(e, G::kDw);
#pragma unroll
        for (uint32_t w = 0; w < G::kDw; ++w) win[w * G::kLanes + lane] = src[w];
    }
    __syncthreads();  // the table is whole; (a lane's window and columns are its own)
    if (!live) return;

    const uint32_t mk = a.m + a.k, top = a.m - 1;
    const uint32_t ncols = talign_columns(e, a.e_begin, mk);  // <= G::kCols: m <= 32 * WORDS
    const auto eq_of = [&](uint32_t j, uint32_t (&eq)[WORDS]) __attribute__((always_inline)) {  // column j >= 1: the masks of byte e - (j - 1)
        const uint32_t wb = talign_window_byte(e, j, G::kDw);
        const uint32_t byte = (win[(wb >> 2) * G::kLanes + lane] >> (8u * (wb & 3u))) & 255u;
        if constexpr (WORDS == 1) {
            eq[0] = peq[byte];
        } else {
            const uint2 v = *reinterpret_cast<const uint2*>(peq + 2u * byte);
            eq[0] = v.x;
            eq[1] = v.y;
        }
    };

    uint32_t pv[WORDS], mv[WORDS];
    edit_fresh<WORDS>(pv, mv);
    int score = (int)a.m, best = (int)a.m;
    uint32_t J = 0;
    for (uint32_t j = 1; j <= ncols; ++j) {
        uint32_t eq[WORDS];
        eq_of(j, eq);
        score += edit_step_dist<WORDS>(pv, mv, eq, top);
        if constexpr (OPS) {
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                cols[((j - 1) * 2 * WORDS + w) * G::kLanes + lane] = pv[w];
                cols[((j - 1) * 2 * WORDS + WORDS + w) * G::kLanes + lane] = mv[w];
            }
        }
        if (score < best) {
            best = score;
            J = j;
        }
    }
    const bool hit = best <= (int)a.k;
    a.io[idx] = hit ? (unsigned long long)(e + 1 - J) << kMisShift | (unsigned long long)best : kTextAlignNone;
    if constexpr (OPS) {
        uint64_t ops[3] = {0, 0, 0};
        if (hit) {
            auto col = [&](uint32_t j, uint32_t (&cpv)[WORDS], uint32_t (&cmv)[WORDS], uint32_t (&ceq)[WORDS]) __attribute__((always_inline)) {
                const uint32_t r = j ? j - 1 : 0;  // (column 0 reads row 0 and drops it: J >= 1 wherever it is asked for with i > 0)
                eq_of(r + 1, ceq);
#pragma unroll
                for (int w = 0; w < WORDS; ++w) {
                    const uint32_t p = cols[(r * 2 * WORDS + w) * G::kLanes + lane], q = cols[(r * 2 * WORDS + WORDS + w) * G::kLanes + lane];
                    cpv[w] = j ? p : ~0u;
                    cmv[w] = j ? q : 0u;
                }
            };
            edit_traceback<WORDS>(a.m, J, best, col, ops);
        }
        a.ops[3 * idx] = ops[0];
        a.ops[3 * idx + 1] = ops[1];
        a.ops[3 * idx + 2] = ops[2];
    }
}

static hipError_t launch_text_edit_align(const TextAlignArgs& a, hipStream_t stream)
{
    if (a.m < 1 || a.m > kTEditMaxM || a.k > SMARTGPU_PMIS_MAX || !a.io || !a.text || !a.peq) return hipErrorInvalidValue;
    if (a.count == 0) return hipSuccess;
#define SG_TALIGN(w_, o_)                                                                                                          \
    do {                                                                                                                           \
        using G = TextAlignGeom<w_, o_>;                                                                                           \
        const uint64_t grid = (a.count + G::kLanes - 1) / G::kLanes;                                                               \
        if (grid > 0x7fffffffull) return hipErrorInvalidValue;                                                                     \
        hipLaunchKernelGGL((text_edit_align<w_, o_>), dim3((uint32_t)grid), dim3(G::kLanes), 0, stream, a);                        \
    } while (0)
    const bool ops = a.ops != nullptr;
    if (a.m <= 32) { if (ops) SG_TALIGN(1, true); else SG_TALIGN(1, false); }
    else           { if (ops) SG_TALIGN(2, true); else SG_TALIGN(2, false); }
#undef SG_TALIGN
    return hipGetLastError();
}

// match_calls.cpp reaches the launcher once this unit is part of the program (talign.hpp)
namespace {
struct RegisterTextAlign {
    RegisterTextAlign() { g_text_edit_align = &launch_text_edit_align; }
} g_register_text_align;
}  // namespace

}  // namespace sg
