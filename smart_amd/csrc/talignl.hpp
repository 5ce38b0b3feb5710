// talignl.hpp — byte texts, LONG patterns: start positions and alignments of edit-distance occurrences (m <= 256, k <= 31),
// the launch interface of text_editl_align (k_talignl.hip).  Host-only types, as talign.hpp, beside which this family stands:
// talign.hpp's kernel walks one LANE per occurrence with bit-vector columns kept in LDS, this one one WAVE per occurrence with
// a lane per diagonal of the band (alignl_band.hpp).  The masks and their table are teditl_host.hpp's, of the REVERSED pattern.
#pragma once
#include "planes.hpp"
#include "teditl_host.hpp"
#include "alignl_band.hpp"

namespace sg {

static_assert(kAlignlMaxM == kTEditlMaxM && kAlignlMaxK == kTEditlMaxK, "the band holds the long family's bounds");
static_assert(kAlignlMaxM == SMARTGPU_EDITL_MAXM && kAlignlMaxK == SMARTGPU_EDITL_MAXK && kAlignlOpsWords == SMARTGPU_ALIGNL_OPS_WORDS,
              "the header's bounds");

// What text_editl_align receives (by value).  One wave per entry of io: it reads the END position e = io[i] (relative to
// text byte 0, e_begin <= e < e_end: the host has checked every one, the kernel checks again), computes the band over
// min(m + k, e - e_begin + 1) columns and overwrites io[i] with (s << kTAlignlShift) | D(e) — the long find's entry with the
// start in place of the end — or with all ones when D(e) > k.  ops (null: no decisions, no traceback; the kernels with
// OPS = false never read it) receives kAlignlOpsWords words per entry, all zero when D(e) > k.
struct TextAlignlArgs {
    const uint8_t* text;        // text byte 0 (kFrontPad zero bytes below it, kBackPad behind byte n: kernels.hpp), 4-byte aligned
    const uint32_t* peq;        // device: 256 masks of the REVERSED pattern, word-major (editl_peq_table), WORDS * 256 dwords
    uint64_t e_begin, e_end;    // the range of the text: no match starts before e_begin
    uint32_t m;                 // pattern length, 1 .. kAlignlMaxM; the kernels with WORDS dwords take m <= 32 * WORDS
    uint32_t k;                 // <= kAlignlMaxK
    unsigned long long* io;     // device, count entries
    unsigned long long* ops;    // device, kAlignlOpsWords * count words, or null
    uint64_t count;
};
constexpr uint32_t kTAlignlShift = 5;                   // the long find's (teditl.hpp: kTEditlShift)
constexpr unsigned long long kTextAlignlNone = ~0ull;  // io[i] of an end that is no occurrence
static_assert(kAlignlMaxK < (1u << kTAlignlShift), "a distance fits below the position");

// dwords per byte value of the table a pattern of m bytes is staged with: the kernels' WORDS
constexpr uint32_t talignl_words(uint32_t m) { return m <= 64 ? 2u : m <= 128 ? 4u : 8u; }

// Reached through a pointer that the unit's own static initialiser sets, as g_text_edit_align (talign.hpp); alignl_calls.cpp
// holds it — null: the calls answer SMARTGPU_ERR_HIP, they never fall back to anything.
extern hipError_t (*g_text_editl_align)(const TextAlignlArgs& a, int num_cus, hipStream_t stream);

}  // namespace sg
