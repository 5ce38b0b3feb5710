// tedit.hpp — byte texts: occurrences within EDIT distance k, the launch interface of text_edit_scan / text_edit_find
// (k_tedit.hip).  Host-only types.  The find's entries and spans are pedit.hpp's: (e << kMisShift) | D(e), one span per
// wave, ordered by order_spans.
#pragma once
#include "planes.hpp"
#include "tedit_host.hpp"

namespace sg {

static_assert(kTEditMaxM == SMARTGPU_EDIT_MAXM, "the masks of tedit_host.hpp hold the longest pattern");
static_assert(kFindSpan == 64 * kTEditRun, "a span: one wave's lanes, one run each");

// What text_edit_scan and text_edit_find receive (by value).  They count / list END positions: e in [e_begin, e_end) with
// D(e) <= k, D the edit distance of the pattern to the nearest substring [s, e] with s >= e_begin (smartgpu.h).
struct TextEditArgs {
    const uint8_t* text;        // text byte 0 (kFrontPad zero bytes below it, kBackPad behind byte n: kernels.hpp)
    const uint32_t* peq;        // device: 256 masks of WORDS dwords (edit_peq_table), 16-byte aligned
    uint64_t e_begin, e_end;    // the range of the text: nothing before e_begin is read into a distance
    uint32_t m;                 // pattern length, 1 .. kTEditMaxM; the kernels with WORDS = 1 take m <= 32
    uint32_t k;                 // <= SMARTGPU_PMIS_MAX
    unsigned long long* count;  // device result slot (pre-zeroed)
};

// The launchers of k_tedit.hip are reached through pointers that the unit's own static initialiser sets (as pedit.hpp's):
// match_calls.cpp holds them — null: the calls answer SMARTGPU_ERR_HIP, they never fall back to anything.
extern hipError_t (*g_text_edit_scan)(const TextEditArgs& a, int num_cus, hipStream_t stream);
extern hipError_t (*g_text_edit_find)(const TextEditArgs& a, unsigned long long* out, unsigned long long cap, int num_cus, hipStream_t stream);

}  // namespace sg
