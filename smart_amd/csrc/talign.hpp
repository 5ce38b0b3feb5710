// talign.hpp — byte texts: start positions and alignments of edit-distance occurrences, the launch interface of
// text_edit_align (k_talign.hip).  Host-only types, as tedit.hpp, whose masks and limits this header takes over; the
// recurrence, the traceback and the packing of the operations are edit_align.hpp's, as for the packed texts (palign.hpp).
#pragma once
#include "tedit.hpp"
#include "talign_host.hpp"
#include "edit_align.hpp"

namespace sg {

static_assert(kTAlignMaxK == SMARTGPU_PMIS_MAX, "the window of talign_host.hpp holds the longest walk");
static_assert(kAlignMaxOps == kTEditMaxM + SMARTGPU_PMIS_MAX, "the longest walk: m + k columns");

// What text_edit_align receives (by value).  One lane per entry of io: it reads the END position e = io[i] (relative to
// text byte 0, e_begin <= e < e_end: the host has checked every one, the kernel checks again), walks
// min(m + k, e - e_begin + 1) bytes backward and overwrites io[i] with (s << kMisShift) | D(e) — the find's entry with the
// start in place of the end — or with all ones when D(e) > k.  ops (null: no traceback; the kernels with OPS = false never
// read it) receives three words per entry, all zero when D(e) > k.
struct TextAlignArgs {
    const uint8_t* text;        // text byte 0 (kFrontPad zero bytes below it, kBackPad behind byte n: kernels.hpp), 4-byte aligned
    const uint32_t* peq;        // device: 256 masks of WORDS dwords (edit_peq_table) of the REVERSED pattern
    uint64_t e_begin, e_end;    // the range of the text: no match starts before e_begin
    uint32_t m;                 // pattern length, 1 .. kTEditMaxM; the kernels with WORDS = 1 take m <= 32
    uint32_t k;                 // <= SMARTGPU_PMIS_MAX
    unsigned long long* io;     // device, count entries
    unsigned long long* ops;    // device, 3 * count words, or null
    uint64_t count;
};
constexpr unsigned long long kTextAlignNone = ~0ull;  // io[i] of an end that is no occurrence

// Reached through a pointer that the unit's own static initialiser sets, as g_text_edit_find (tedit.hpp): null — the
// align calls answer SMARTGPU_ERR_HIP.
extern hipError_t (*g_text_edit_align)(const TextAlignArgs& a, hipStream_t stream);

}  // namespace sg
