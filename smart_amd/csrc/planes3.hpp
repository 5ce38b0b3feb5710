// planes3.hpp — packed texts of FIVE TO EIGHT distinct byte values: a third bit plane beside planes.hpp's two, and the
// launch interface of its kernels (k_planes3.hip).  Host-only types, as planes.hpp.
//
// A symbol's code (the rank of its byte value among the values the text holds, ascending) has three bits; plane b holds
// bit b, 32 symbols per dword as in planes.hpp.  One allocation, planes.hpp's with a third plane:
//     [kFrontPad zero bytes | plane 0 | kPlaneBackPad | plane 1 | kPlaneBackPad | plane 2 | kPlaneBackPad]
// plane b at b * plane_stride(n), every plane 256-byte aligned, the whole allocation zero-filled before the pack: pad and
// tail bits are zero and look like code 0; they are never counted, the range [s_begin, s_end) keeps every window inside
// the text.  flush_hits finds its staging slots in the front pad below plane 0, as planes_scan does.
//
// A SET over up to eight codes is a uint8_t — the type the sets calls take — and every call on a three-plane text is a
// set call to the kernels: an exact pattern travels as singleton sets, a byte the text does not hold as an empty set.
#pragma once
#include "planes.hpp"

namespace sg {

constexpr int kPlanes3 = 3;
// the scan's farthest load on EACH of the three planes: the pattern's last block (SMARTGPU_XSIZE / 32 dwords behind a
// lane's chunk) plus the lane's five dwords — every plane has its own back pad
static_assert(kPlaneBackPad >= 4 * (SMARTGPU_XSIZE / 32 + 1 + 8) && kPlaneBackPad % 256 == 0 && plane_stride(1) % 256 == 0,
              "three planes: the pattern's last block + a lane's five dwords stay inside every plane's back pad");
static_assert(SMARTGPU_PTEXT_MAXVALUES == 1 << kPlanes3, "a code has one bit per plane");

constexpr size_t kSet8Words = 8 * kPatWords;  // a pattern's eight membership planes, Y0..Y7
// Patterns per batch call on a three-plane text: they are staged at kSet8Words dwords each (4256 bytes, four times a
// two-plane pattern's code planes) in the device's 32 MiB staging buffer and, for m > 32, in its arena.
constexpr uint32_t kBatch3Max = (32u << 20) / (4 * kSet8Words);
static_assert(kBatch3Max == 7884, "the bound include/smartgpu.h documents for the batch calls");

// What planes3_scan and planes3_find receive (by value).  A position that accepts every value of the text, and a position
// the host does not compare (an empty set: a mismatch in every window, counted by the host as `foreign`, the budget lowered
// by their number), has ALL EIGHT bits set, whatever codes the text holds: the kernels spend no instruction on it.
struct Plane3Args {
    const uint32_t* p0;         // plane 0, dword 0 (flush_hits: the allocation's front pad lies kFrontPad below)
    const uint32_t* p1;         // plane 1
    const uint32_t* p2;         // plane 2
    uint64_t s_begin, s_end;    // start positions to count: s_begin <= s < s_end (s_end <= n - m + 1)
    uint32_t m;                 // pattern length in symbols
    uint32_t y[8];              // bit j of y[c]: pattern position j < 32 accepts code c
    uint32_t budget;            // non-members allowed at the compared positions, <= SMARTGPU_PMIS_MAX (0: the live-mask form)
    uint32_t foreign;           // added to every distance the find reports (budget + foreign <= SMARTGPU_PMIS_MAX)
    uint32_t shift;             // the find's entries: position << shift | distance (0: positions alone; kMisShift)
    const uint32_t* pat;        // device, m > 32 only: the whole pattern as membership planes, u32 Y0..Y7[kPatWords]
    unsigned long long* count;  // device result slot (pre-zeroed); the find's cursor
};

// The two-plane halves of a set's tables, k_planes.hip's sets_table / sets_mis_table on two planes: the four low bits of
// a set speak of codes 0..3 (plane 2 clear), the four high bits of codes 4..7 (plane 2 set).
// M & "the code (t1 t0) is a member of s" over M = 0xF0, t0 = 0xCC, t1 = 0xAA
constexpr uint32_t mem2_table(uint32_t s) { return (s & 1u ? 0x10u : 0u) | (s & 2u ? 0x40u : 0u) | (s & 4u ? 0x20u : 0u) | (s & 8u ? 0x80u : 0u); }
// "the code (t1 t0) is NOT a member of s" over t0 = 0xCC, t1 = 0xAA (both nibbles: the first input does not matter)
constexpr uint32_t mis2_table(uint32_t s) { return 0xFFu ^ ((s & 1u ? 0x11u : 0u) | (s & 2u ? 0x44u : 0u) | (s & 4u ? 0x22u : 0u) | (s & 8u ? 0x88u : 0u)); }
static_assert(mem2_table(1) == 0x10 && mem2_table(2) == 0x40 && mem2_table(4) == 0x20 && mem2_table(8) == 0x80 && mem2_table(15) == 0xF0 &&
              mis2_table(1) == 0xEE && mis2_table(2) == 0xBB && mis2_table(4) == 0xDD && mis2_table(8) == 0x77 && mis2_table(0) == 0xFF,
              "singleton sets: planes_kill's and planes_mis_add's tables");

// The launchers of k_planes3.hip are reached through pointers that the unit's own static initialiser sets (as pedit.hpp's):
// match_calls.cpp holds them — null: the calls on a three-plane text answer SMARTGPU_ERR_HIP, they never fall back to anything —
// so a program that includes match_calls.cpp without k_planes3.hip still links.
// byte text -> three planes.  values[0..6]: the byte values of codes 0..6 (255 where the text has fewer: no byte is
// greater); the text's back pad (zero bytes) is read up to 31 bytes beyond n, the planes must be zero-filled before
extern hipError_t (*g_planes3_pack)(const uint8_t* text, uint64_t n, uint32_t* p0, uint32_t* p1, uint32_t* p2, const uint8_t values[7],
                                    hipStream_t stream);
// Grid, range convention and — for the find — the spans of `out`: those of launch_planes_scan / launch_planes_find
// (planes.hpp).  `planes` is 3 (the signature is the other packed launchers').
extern hipError_t (*g_planes3_scan)(const Plane3Args& a, int planes, int num_cus, hipStream_t stream);
extern hipError_t (*g_planes3_find)(const Plane3Args& a, unsigned long long* out, unsigned long long cap, int planes, int num_cus,
                                    hipStream_t stream);

}  // namespace sg
