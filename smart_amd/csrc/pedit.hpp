// pedit.hpp — packed texts: occurrences within EDIT distance k (substitutions, insertions, deletions), the launch
// interface of planes_edit_scan / planes_edit_find (k_pedit.hip).  Host-only types, as planes.hpp, whose layout of the
// planes, pads and find entries this header takes over.
#pragma once
#include "planes.hpp"
#include "pedit_host.hpp"

namespace sg {

static_assert(kEditMaxM == SMARTGPU_PEDIT_MAXM, "the masks of pedit_host.hpp hold the longest pattern");

// What planes_edit_scan and planes_edit_find receive (by value).  They count / list END positions: e in [e_begin, e_end)
// with D(e) <= k, D the edit distance of the pattern to the nearest substring [s, e] with s >= e_begin (smartgpu.h).
struct PlaneEditArgs {
    const uint32_t* p0;         // as PlaneArgs
    const uint32_t* p1;
    uint64_t e_begin, e_end;    // the range of the text: nothing before e_begin is read into a distance
    uint32_t m;                 // pattern length, 1 .. kEditMaxM; the kernels with WORDS = 1 take m <= 32
    uint32_t k;                 // <= SMARTGPU_PMIS_MAX
    uint32_t peq[4][kEditWords];  // edit_peq_pattern / edit_peq_sets (one plane: peq[0], peq[1]; WORDS = 1: peq[c][0])
    unsigned long long* count;  // device result slot (pre-zeroed)
};

// End positions a lane owns and walks one after the other: planes_find's chunk, so that a wave's 64 lanes cover
// kFindSpan consecutive positions and the find's entries are planes_mis_find's spans (order_spans with kMisShift).
// A lane walks up to m + k <= kEditMaxM + SMARTGPU_PMIS_MAX symbols before its run without counting (the warm-up).
constexpr uint32_t kEditRun = 128;
static_assert(kFindSpan == 64 * kEditRun, "a span: one wave's lanes, one run each");

// Grid: a workgroup of 256 lanes per 256 runs, at most 8 per CU.  The find's entries are (e << kMisShift) | D(e).
// The launchers of k_pedit.hip are reached through pointers that the unit's own static initialiser sets (as multi.hpp's
// g_hor_multi): match_calls.cpp holds them — null: the edit calls answer SMARTGPU_ERR_HIP, they never fall back to anything — so a
// program that includes match_calls.cpp without k_pedit.hip still links.
extern hipError_t (*g_planes_edit_scan)(const PlaneEditArgs& a, int planes, int num_cus, hipStream_t stream);
extern hipError_t (*g_planes_edit_find)(const PlaneEditArgs& a, unsigned long long* out, unsigned long long cap, int planes, int num_cus,
                                        hipStream_t stream);

}  // namespace sg
