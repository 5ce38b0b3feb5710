// palignl.hpp — packed texts, LONG patterns: start positions and alignments of edit-distance occurrences (m <= 256, k <= 31),
// the launch interface of planes_editl_align (k_palignl.hip).  Host-only types, as palign.hpp, beside which this family stands:
// palign.hpp's kernel walks one LANE per occurrence with bit-vector columns kept in LDS, this one one WAVE per occurrence with
// a lane per diagonal of the band (alignl_band.hpp) — the decomposition of text_editl_align (talignl.hpp), fed from bit planes
// instead of bytes.  The masks are peditl_host.hpp's, of the REVERSED pattern: four of eight dwords, kernel arguments.
#pragma once
#include "planes.hpp"
#include "peditl_host.hpp"
#include "alignl_band.hpp"

namespace sg {

static_assert(kAlignlMaxM == kEditlMaxM && kAlignlMaxK == kEditlMaxK, "the band holds the long packed family's bounds");
static_assert(kAlignlMaxM == SMARTGPU_PEDITL_MAXM && kAlignlMaxK == SMARTGPU_PEDITL_MAXK && kAlignlOpsWords == SMARTGPU_ALIGNL_OPS_WORDS,
              "the header's bounds");

// What planes_editl_align receives (by value).  One wave per entry of io: it reads the END position e = io[i] (relative to
// symbol 0, e_begin <= e < e_end: the host has checked every one, the kernel checks again), computes the band over
// min(m + k, e - e_begin + 1) columns and overwrites io[i] with (s << kPAlignlShift) | D(e) — the long find's entry with the
// start in place of the end — or with all ones when D(e) > k.  ops (null: no decisions, no traceback; the kernels with
// OPS = false never read it) receives kAlignlOpsWords words per entry, all zero when D(e) > k.
struct PlaneAlignlArgs {
    const uint32_t* p0;         // as PlaneArgs
    const uint32_t* p1;
    uint64_t e_begin, e_end;    // the range of the text: no match starts before e_begin
    uint32_t m;                 // pattern length, 1 .. kAlignlMaxM
    uint32_t k;                 // <= kAlignlMaxK
    uint32_t peq[4][kEditlWords];  // editl_peq_pattern / editl_peq_sets of the REVERSED pattern (one plane: peq[0], peq[1])
    unsigned long long* io;     // device, count entries
    unsigned long long* ops;    // device, kAlignlOpsWords * count words, or null
    uint64_t count;
};
constexpr uint32_t kPAlignlShift = 5;                    // the long find's (peditl.hpp: kEditlShift)
constexpr unsigned long long kPlaneAlignlNone = ~0ull;  // io[i] of an end that is no occurrence
static_assert(kAlignlMaxK < (1u << kPAlignlShift), "a distance fits below the position");

// THE WINDOW.  A band from e consumes the symbols e, e - 1, ..., at most m + k <= 287 of them.  The wave holds the ALIGNED
// dwords of each plane that cover them: kPAlignlWinDw = 10, the last of them plane dword e >> 5.  With e % 32 == 0 symbol e is
// alone in the last dword and the other 286 lie in the nine before it.
constexpr uint32_t kPAlignlWinDw = 1u + (kAlignlMaxOps - 1u + 31u) / 32u;
static_assert(kPAlignlWinDw == 10 && 32 * (kPAlignlWinDw - 1) + 1 >= kAlignlMaxOps && 32 * (kPAlignlWinDw - 2) + 1 < kAlignlMaxOps,
              "the window holds the longest walk at e % 32 == 0, and not a dword more");
static_assert(2 * kPAlignlWinDw <= kAlignlLanes, "a wave loads the windows of both planes with one load per lane");

// The plane dword (index relative to dword 0 of the plane) that window dword 0 holds: negative for e < 32 * 9, where the
// window reaches up to 36 bytes below the plane; a band never consumes those (it has at most e - e_begin + 1 <= e + 1 columns).
SG_HOST_DEVICE inline long long palignl_window_first(uint64_t e)
{
    return static_cast<long long>(e >> 5) - static_cast<long long>(kPAlignlWinDw - 1u);
}

// Column j >= 1 of the band consumes symbol e - (j - 1): bit wb & 31 of window dword wb >> 5, wb as returned here — the
// symbol's own bit (e - j + 1) & 31 of plane dword (e - j + 1) >> 5.  j - 1 <= 286 < 32 * 9 + 1, so wb >= 0 whatever e % 32 is.
SG_HOST_DEVICE inline uint32_t palignl_window_bit(uint64_t e, uint32_t j)
{
    return 32u * (kPAlignlWinDw - 1u) + (static_cast<uint32_t>(e) & 31u) - (j - 1u);
}

// miss of cell (i, j), i >= 1, whose column's symbol has the code `code`: the dword of the four masks to hand to alignl_miss
SG_HOST_DEVICE inline uint32_t palignl_peq_index(uint32_t i, uint32_t code) { return code * kEditlWords + ((i - 1u) >> 5); }

// Reached through a pointer that the unit's own static initialiser sets, as g_planes_edit_align (palign.hpp); align_calls.cpp
// holds it — null: the calls answer SMARTGPU_ERR_HIP, they never fall back to anything.
extern hipError_t (*g_planes_editl_align)(const PlaneAlignlArgs& a, int planes, int num_cus, hipStream_t stream);

}  // namespace sg

// The host path of smartgpu_palign_editl64 / smartgpu_palign_sets_editl64 (palignl_calls.cpp): align_run of the family PAlignl,
// defined in align_calls.cpp beside the other families.  C++ linkage, hidden: no part of the ABI.
template <typename Text>
struct Question;  // call_host.hpp
__attribute__((visibility("hidden"))) int palignl_run(const Question<smartgpu_ptext>& q, const uint64_t* ends, uint64_t count, uint64_t* starts,
                                                      uint8_t* distances, uint64_t* ops);
