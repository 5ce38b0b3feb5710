// peditl.hpp — packed texts: occurrences within EDIT distance k of patterns up to 256 symbols, k up to 31: the launch
// interface of planes_editl_scan / planes_editl_find (k_peditl.hip).  Host-only types, as pedit.hpp, beside which this
// family stands: pedit.hpp's kernels keep the whole column in one or two dwords, these keep it in blocks (edit_block.hpp).
#pragma once
#include "planes.hpp"
#include "peditl_host.hpp"

namespace sg {

static_assert(kEditlMaxM == SMARTGPU_PEDITL_MAXM && kEditlMaxK == SMARTGPU_PEDITL_MAXK, "the masks of peditl_host.hpp hold the longest pattern");

// What planes_editl_scan and planes_editl_find receive (by value): PlaneEditArgs with wider masks and the switch.
struct PlaneEditlArgs {
    const uint32_t* p0;         // as PlaneArgs
    const uint32_t* p1;
    uint64_t e_begin, e_end;    // the range of the text: nothing before e_begin is read into a distance
    uint32_t m;                 // pattern length, 1 .. kEditlMaxM; the kernels with WORDS dwords take m <= 32 * WORDS
    uint32_t k;                 // <= kEditlMaxK
    uint32_t all_blocks;        // non-zero: every block of every column, no cut-off (SMARTGPU_PEDITL_ALL_BLOCKS)
    uint32_t peq[4][kEditlWords];  // editl_peq_pattern / editl_peq_sets (one plane: peq[0], peq[1])
    unsigned long long* count;  // device result slot (pre-zeroed)
};

// End positions a lane owns and walks one after the other, in pieces of kEditlPiece symbols (four dwords per plane, one
// 16-byte load).  Before its run a lane walks m + k <= 287 symbols without counting (the fresh start of k_pedit.hip), so
// it walks (kEditlRun + m + k) / kEditlRun symbols per owned one: 1.56 at m = 256, k = 31, what pedit.hpp's run of 128
// costs at m = 64, k = 7, and 1.21 at m = 100, k = 7.  What the longer run costs on SHORT texts: a text has n / 512 lanes'
// worth of work, so one below 512 * 64 * 4 * 256 = 32 Mi symbols does not give every SIMD of 256 CUs a wave, and a text of
// 2^20 symbols is walked by 32 waves.  Other run lengths were not measured.
constexpr uint32_t kEditlPiece = 128;
constexpr uint32_t kEditlRun = 512;
constexpr uint32_t kEditlWarmPieces = 3;
static_assert(kEditlRun % kEditlPiece == 0, "a run is whole pieces");
static_assert(kEditlWarmPieces * kEditlPiece >= kEditlMaxM + kEditlMaxK, "the warm-up of the longest pattern at the largest k lies in the pieces before the run");
// the loads: a lane's pieces start at or after dword 0 of a plane (pieces before the text are not loaded: their address is
// clamped, and they are never walked), and the last run's last piece ends less than one run behind the text's last dword
static_assert(kPlaneBackPad >= kEditlRun / 8 + 16, "the last run's loads stay inside the allocation");
static_assert(kFrontPad >= 16, "plane 0 does not start the allocation");

// The find's entries are (e << kEditlShift) | D(e), in no particular order (the output stage runs per 32 owned positions
// of a wave's lanes): the host sorts them.
constexpr uint32_t kEditlShift = 5;
static_assert(kEditlMaxK < (1u << kEditlShift), "a distance fits below the position");

// Grid: a workgroup of 256 lanes per 256 runs, at most 8 per CU.  The launchers of k_peditl.hip are reached through
// pointers that the unit's own static initialiser sets (as pedit.hpp's): match_calls.cpp holds them — null: the editl calls answer
// SMARTGPU_ERR_HIP, they never fall back to anything.
extern hipError_t (*g_planes_editl_scan)(const PlaneEditlArgs& a, int planes, int num_cus, hipStream_t stream);
extern hipError_t (*g_planes_editl_find)(const PlaneEditlArgs& a, unsigned long long* out, unsigned long long cap, int planes, int num_cus,
                                         hipStream_t stream);

}  // namespace sg
