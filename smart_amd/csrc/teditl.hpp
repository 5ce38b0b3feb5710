// teditl.hpp — byte texts: occurrences within EDIT distance k of patterns up to 256 bytes, k up to 31: the launch interface
// of text_editl_scan / text_editl_find (k_teditl.hip).  Host-only types, as tedit.hpp, beside which this family stands:
// tedit.hpp's kernels keep the whole column in one or two dwords, these keep it in blocks (edit_block.hpp), as peditl.hpp's.
#pragma once
#include "planes.hpp"
#include "teditl_host.hpp"

namespace sg {

static_assert(kTEditlMaxM == SMARTGPU_EDITL_MAXM && kTEditlMaxK == SMARTGPU_EDITL_MAXK, "the masks of teditl_host.hpp hold the longest pattern");

// What text_editl_scan and text_editl_find receive (by value): TextEditArgs with the wider table and the switch.
struct TextEditlArgs {
    const uint8_t* text;        // text byte 0 (kFrontPad zero bytes below it, kBackPad behind byte n: kernels.hpp)
    const uint32_t* peq;        // device: 256 masks, word-major (editl_peq_table), WORDS * 256 dwords, 16-byte aligned
    uint64_t e_begin, e_end;    // the range of the text: nothing before e_begin is read into a distance
    uint32_t m;                 // pattern length, 1 .. kTEditlMaxM; the kernels with WORDS dwords take m <= 32 * WORDS
    uint32_t k;                 // <= kTEditlMaxK
    uint32_t all_blocks;        // non-zero: every block of every column, no cut-off (SMARTGPU_EDITL_ALL_BLOCKS)
    unsigned long long* count;  // device result slot (pre-zeroed)
};

// The workgroup and its LDS: [128 bytes: flush_hits][WORDS KiB: the masks, word-major][256 rows of 132 bytes: one piece per
// lane].  A row is text_tile.hpp's: 128 bytes of text and 4 never written, so that lanes a row apart sit on neighbouring
// banks.  All of it is dynamic LDS.
constexpr int kTEditlT = (int)kTEditlLanes;                        // lanes of a workgroup
constexpr uint32_t kTEditlRowBytes = kTEditlPiece + 4, kTEditlRowDw = kTEditlRowBytes / 4;
constexpr uint32_t kTEditlMasksOff = 128;                          // the masks: behind flush_hits' 128 bytes
constexpr uint32_t kTEditlPieces = kTEditlRun / kTEditlPiece;      // owned pieces of a run
constexpr uint32_t kTEditlWarmPieces = (kTEditlMaxM + kTEditlMaxK + kTEditlPiece - 1) / kTEditlPiece;  // at most, before a run
constexpr uint32_t kTEditlLdsCu = 160u * 1024u;                    // LDS of a CU
__host__ __device__ constexpr uint32_t teditl_rows_off(int words) { return kTEditlMasksOff + 1024u * words; }
__host__ __device__ constexpr uint32_t teditl_lds_bytes(int words) { return teditl_rows_off(words) + kTEditlLanes * kTEditlRowBytes; }
// workgroups per CU: what fits in the LDS — the kernels' __launch_bounds__ and the grid's cap
__host__ __device__ constexpr int teditl_wgs(int words) { return (int)(kTEditlLdsCu / teditl_lds_bytes(words)); }
static_assert(kTEditlT == 256 && kTEditlPiece == 128 && kTEditlRun % kTEditlPiece == 0, "a piece is eight 16-byte chunks, a run whole pieces, a lane parks eight chunks per trip");
static_assert(kTEditlRowDw % 32 == 1, "lanes a row apart sit on neighbouring banks");
static_assert(kTEditlRun > kTEditlMaxM + kTEditlMaxK, "only the lanes of a range's first two runs start clipped");
static_assert(teditl_lds_bytes(2) == 35968 && teditl_lds_bytes(4) == 38016 && teditl_lds_bytes(8) == 42112, "the LDS of a workgroup");
static_assert(teditl_wgs(2) == 4 && teditl_wgs(4) == 4 && teditl_wgs(8) == 3, "workgroups per CU");
// the loads: the first warm-up piece of a text's first run begins kTEditlWarmPieces pieces below text byte 0, and the last
// super-tile ends less than one super-tile behind e_end <= n; what is read outside [e_begin, e_end) is parked, never walked
static_assert(kTEditlWarmPieces * kTEditlPiece == 384, "three pieces before a run");
static_assert(kFrontPad >= 384 && kBackPad >= 256 * 512, "the pads hold what the first and the last super-tile read");
static_assert(kFrontPad >= kTEditlWarmPieces * kTEditlPiece && kBackPad >= kTEditlSuper && kFrontPad % 16 == 0, "the same, by name");

// The find's entries are (e << kEditlShift) | D(e) in no particular order, as peditl.hpp's: the host sorts them.
constexpr uint32_t kTEditlShift = 5;
static_assert(kTEditlMaxK < (1u << kTEditlShift), "a distance fits below the position");

// The launchers of k_teditl.hip are reached through pointers that the unit's own static initialiser sets (as tedit.hpp's):
// match_calls.cpp holds them — null: the calls answer SMARTGPU_ERR_HIP, they never fall back to anything.
extern hipError_t (*g_text_editl_scan)(const TextEditlArgs& a, int num_cus, hipStream_t stream);
extern hipError_t (*g_text_editl_find)(const TextEditlArgs& a, unsigned long long* out, unsigned long long cap, int num_cus, hipStream_t stream);

}  // namespace sg
