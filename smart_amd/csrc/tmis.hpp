// tmis.hpp — byte texts: occurrences with at most k MISMATCHES (the Hamming distance of a window of m bytes), the launch
// interface of text_mis_scan / text_mis_find (k_tmis.hip).  Host-only types.  The lanes own END positions e = s + m - 1, in
// tedit.hpp's geometry; the find's entries are (e << kMisShift) | distance, one span of kFindSpan ends per wave, ordered by
// order_spans over the ends — the host turns an end into its start, e - (m - 1), when it unpacks the distances (a span of
// STARTS would begin m - 1 below a span boundary and order_spans would see it in two pieces).
#pragma once
#include "planes.hpp"
#include "tmis_host.hpp"

namespace sg {

static_assert(kTMisMaxM == SMARTGPU_MIS_MAXM, "the masks of tmis_host.hpp hold the longest pattern");
static_assert(kFindSpan == 64 * kTEditRun, "a span: one wave's lanes, one run each");

// What text_mis_scan and text_mis_find receive (by value).  They count / list the windows [e - m + 1, e] with
// e_begin + m - 1 <= e < e_end and at most k positions whose mask does not accept the window's byte.
struct TextMisArgs {
    const uint8_t* text;        // text byte 0 (kFrontPad zero bytes below it, kBackPad behind byte n: kernels.hpp)
    const uint32_t* neq;        // device: 256 masks of WORDS dwords (mis_neq_*, edit_peq_table), 16-byte aligned
    uint64_t e_begin, e_end;    // the range of the text: no window begins before e_begin or ends at or behind e_end
    uint32_t m;                 // pattern length, 1 .. kTMisMaxM; the kernels with WORDS = 1 take m <= 32
    uint32_t k;                 // <= SMARTGPU_PMIS_MAX; the kernels with BITS = 1 / 2 take k <= 1 / 3
    unsigned long long* count;  // device result slot (pre-zeroed)
};

// The launchers of k_tmis.hip are reached through pointers that the unit's own static initialiser sets (as tedit.hpp's):
// match_calls.cpp holds them — null: the calls answer SMARTGPU_ERR_HIP, they never fall back to anything.
extern hipError_t (*g_text_mis_scan)(const TextMisArgs& a, int num_cus, hipStream_t stream);
extern hipError_t (*g_text_mis_find)(const TextMisArgs& a, unsigned long long* out, unsigned long long cap, int num_cus, hipStream_t stream);

}  // namespace sg
