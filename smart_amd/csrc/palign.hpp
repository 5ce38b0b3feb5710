// palign.hpp — packed texts: start positions and alignments of edit-distance occurrences, the launch interface of
// planes_edit_align (k_palign.hip).  Host-only types, as pedit.hpp, whose masks and limits this header takes over.
#pragma once
#include "pedit.hpp"
#include "edit_align.hpp"

namespace sg {

static_assert(kAlignMaxOps == kEditMaxM + SMARTGPU_PMIS_MAX, "the longest walk: m + k columns");

// What planes_edit_align receives (by value).  One lane per entry of io: it reads the END position e = io[i] (relative to
// symbol 0, e_begin <= e < e_end: the host has checked every one), walks min(m + k, e - e_begin + 1) symbols backward and
// overwrites io[i] with (s << kMisShift) | D(e) — the find's entry with the start in place of the end — or with all ones
// when D(e) > k.  ops (null: no traceback; the kernels with OPS = false never read it) receives three words per entry, all
// zero when D(e) > k.
struct PlaneAlignArgs {
    const uint32_t* p0;         // as PlaneArgs
    const uint32_t* p1;
    uint64_t e_begin, e_end;    // the range of the text: no match starts before e_begin
    uint32_t m;                 // pattern length, 1 .. kEditMaxM; the kernels with WORDS = 1 take m <= 32
    uint32_t k;                 // <= SMARTGPU_PMIS_MAX
    uint32_t peq[4][kEditWords];  // edit_peq_pattern / edit_peq_sets of the REVERSED pattern
    unsigned long long* io;     // device, count entries
    unsigned long long* ops;    // device, 3 * count words, or null
    uint64_t count;
};
constexpr unsigned long long kAlignNone = ~0ull;  // io[i] of an end that is no occurrence

// Reached through a pointer that the unit's own static initialiser sets, as g_planes_edit_find (pedit.hpp): null — the
// align calls answer SMARTGPU_ERR_HIP.
extern hipError_t (*g_planes_edit_align)(const PlaneAlignArgs& a, int planes, hipStream_t stream);

}  // namespace sg
