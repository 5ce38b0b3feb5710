// planes.hpp — packed texts (smartgpu_ptext): a text of at most four distinct byte values held as BIT PLANES, and the
// launch interface of its kernels (k_planes.hip).  Host-only types, as kernels.hpp.
//
// Plane b holds bit b of every symbol's code (the rank of its byte value among the values the text holds, ascending),
// 32 symbols per dword: symbol i = bit i % 32 of dword i / 32.  One plane for at most two values, two for three or four.
// One allocation:
//     [kFrontPad zero bytes | plane 0 | kPlaneBackPad zero bytes | plane 1 | kPlaneBackPad zero bytes]
// every plane 256-byte aligned.  The front pad is the byte text's (kernels.hpp): flush_hits finds its staging slots
// kFrontPad - kHitSlotsOff bytes below plane 0, so planes_scan may run as a grid of any size.  The back pad lets every
// load of the scan — a lane's four dwords, the dword behind them, and the same up to kPatWords dwords further on for the
// symbols beyond the 32nd — stay inside the allocation with no bounds check.  Pad bits are zero and look like code 0:
// they are never counted, the range [s_begin, s_end) keeps every window inside the text.
#pragma once
#include "kernels.hpp"

#include "../../include/smartgpu.h"

namespace sg {

constexpr uint32_t kPatWords = (SMARTGPU_XSIZE + 31) / 32 + 1;  // dwords of one plane of a pattern (zero padded), 133
constexpr uint64_t kPlaneBackPad = 4096;                        // bytes behind each plane
static_assert(kPlaneBackPad >= 4 * (SMARTGPU_XSIZE / 32 + 1 + 8) && kPlaneBackPad % 256 == 0, "the scan's farthest load: the pattern's last dword + a lane's five");

constexpr uint64_t plane_bytes(uint64_t n) { return 4 * ((n + 31) / 32); }                                   // pads excluded
constexpr uint64_t plane_stride(uint64_t n) { return ((plane_bytes(n) + 255) & ~255ull) + kPlaneBackPad; }    // plane b at b * stride

// What planes_scan and planes_find receive (by value).
struct PlaneArgs {
    const uint32_t* p0;         // plane 0, dword 0 (flush_hits: the allocation's front pad lies kFrontPad below)
    const uint32_t* p1;         // plane 1 (= p0 for a one-plane text; never read then)
    uint64_t s_begin, s_end;    // start positions to count: s_begin <= s < s_end (s_end <= n - m + 1)
    uint32_t m;                 // pattern length in symbols
    uint32_t x0, x1;            // bits 0 / 1 of the codes of the pattern's first 32 symbols (symbol j = bit j)
    const uint32_t* pat;        // device, m > 32 only: the pattern as planes, u32 X0[kPatWords], X1[kPatWords]
    unsigned long long* count;  // device result slot (pre-zeroed)
};

// byte text -> planes.  values[0..2]: the byte values of codes 0..2 (255 where the text has fewer: no byte is greater);
// the text's back pad (zero bytes) is read up to 31 bytes beyond n, the planes must be zero-filled before
hipError_t launch_planes_pack(const uint8_t* text, uint64_t n, uint32_t* p0, uint32_t* p1, int planes, const uint8_t values[3],
                              hipStream_t stream);
hipError_t launch_planes_scan(const PlaneArgs& a, int planes, int num_cus, hipStream_t stream);

// Positions: planes_scan with an output stage.  a.count (pre-zeroed) is the cursor and receives the number of occurrences;
// out[0 .. min(count, cap)) receives start positions relative to symbol 0 of the text; entries beyond cap are dropped.
// What lies in `out` is a sequence of SPANS: the survivors among the kFindSpan start positions
// [s_begin / 128 * 128 + k * kFindSpan, + kFindSpan) for some k, ascending and contiguous; every k at most once, in no
// particular order.
constexpr uint64_t kFindSpan = 8192;
hipError_t launch_planes_find(const PlaneArgs& a, unsigned long long* out, unsigned long long cap, int planes, int num_cus,
                              hipStream_t stream);

// SET patterns: pattern position j accepts a set of codes instead of one.  What planes_sets_scan and planes_sets_find
// receive (by value): PlaneArgs with membership bits in place of code bits.  A position that accepts every value of the
// text has ALL its bits set (of y[0], y[1] on one plane, of y[0..3] on two), whatever codes the text holds: the kernels
// then spend no instruction on it.  No position is empty (the host answers 0 without a launch).
struct PlaneSetArgs {
    const uint32_t* p0;         // as PlaneArgs
    const uint32_t* p1;
    uint64_t s_begin, s_end;
    uint32_t m;
    uint32_t y[4];              // bit j of y[c]: pattern position j < 32 accepts code c (one plane: y[0], y[1] only)
    const uint32_t* pat;        // device, m > 32 only: the whole pattern as membership planes, u32 Y0..Y3[kPatWords]
    unsigned long long* count;  // device result slot (pre-zeroed)
};
// Grid, occupancy, range convention and — for the find — the spans of `out`: those of launch_planes_scan / launch_planes_find.
hipError_t launch_planes_sets_scan(const PlaneSetArgs& a, int planes, int num_cus, hipStream_t stream);
hipError_t launch_planes_sets_find(const PlaneSetArgs& a, unsigned long long* out, unsigned long long cap, int planes, int num_cus,
                                   hipStream_t stream);

// MISMATCHES: occurrences with at most `budget` positions j where T[s + j] != P[j].  What planes_mis_scan and planes_mis_find
// receive (by value): PlaneArgs with a third plane of the pattern, the SKIP plane — positions that are not compared (pattern
// bytes the text does not hold: a mismatch in every window, counted by the host, which lowers the budget by their number and
// passes it as `foreign`; their code bits are zero).
struct PlaneMisArgs {
    const uint32_t* p0;         // as PlaneArgs
    const uint32_t* p1;
    uint64_t s_begin, s_end;
    uint32_t m;
    uint32_t x0, x1;            // bits 0 / 1 of the codes of the pattern's first 32 symbols
    uint32_t skip;              // bit j: pattern position j < 32 is not compared
    uint32_t budget;            // mismatches allowed at the compared positions, <= SMARTGPU_PMIS_MAX
    uint32_t foreign;           // added to every distance the find reports (budget + foreign <= SMARTGPU_PMIS_MAX)
    const uint32_t* pat;        // device, m > 32 only: u32 X0[kPatWords], X1[kPatWords], SKIP[kPatWords]
    unsigned long long* count;  // device result slot (pre-zeroed)
};
// Grid, occupancy and range convention: launch_planes_scan's.  The find's entries are (position << kMisShift) | distance,
// distance = mismatches at the compared positions + foreign; their spans are planes_find's, taken on the position.
constexpr uint32_t kMisShift = 3;
static_assert(SMARTGPU_PMIS_MAX < (1u << kMisShift), "a distance fits below the position");
hipError_t launch_planes_mis_scan(const PlaneMisArgs& a, int planes, int num_cus, hipStream_t stream);
hipError_t launch_planes_mis_find(const PlaneMisArgs& a, unsigned long long* out, unsigned long long cap, int planes, int num_cus,
                                  hipStream_t stream);

// SET patterns with MISMATCHES: occurrences with at most `budget` positions j where the code of T[s + j] is not a member of
// set j.  What planes_sets_mis_scan and planes_sets_mis_find receive (by value): PlaneSetArgs with PlaneMisArgs' budget and
// foreign.  There is no skip plane: a position that is not compared (an empty set: a mismatch in every window, counted by the
// host, which lowers the budget by their number and passes it as `foreign`) has ALL its bits set, as a position that accepts
// every value of the text has — neither costs an instruction nor is counted on the device.
struct PlaneSetMisArgs {
    const uint32_t* p0;         // as PlaneArgs
    const uint32_t* p1;
    uint64_t s_begin, s_end;
    uint32_t m;
    uint32_t y[4];              // as PlaneSetArgs
    uint32_t budget;            // non-members allowed at the compared positions, <= SMARTGPU_PMIS_MAX
    uint32_t foreign;           // added to every distance the find reports (budget + foreign <= SMARTGPU_PMIS_MAX)
    const uint32_t* pat;        // device, m > 32 only: u32 Y0..Y3[kPatWords]
    unsigned long long* count;  // device result slot (pre-zeroed)
};
// Grid, occupancy, range convention and the find's entries: those of launch_planes_mis_scan / launch_planes_mis_find.
hipError_t launch_planes_sets_mis_scan(const PlaneSetMisArgs& a, int planes, int num_cus, hipStream_t stream);
hipError_t launch_planes_sets_mis_find(const PlaneSetMisArgs& a, unsigned long long* out, unsigned long long cap, int planes, int num_cus,
                                       hipStream_t stream);

}  // namespace sg
