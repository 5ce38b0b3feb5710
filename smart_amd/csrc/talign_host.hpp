// talign_host.hpp — byte texts: starts and alignments of edit-distance occurrences (smartgpu_align_edit64, talign.hpp): what
// the host and text_edit_align (k_talign.hip) share — the reversal of the pattern, whose 256 masks (tedit_host.hpp) the
// backward walk consumes, and the geometry of a lane's text window.  Host and device, no HIP call, no error text:
// tests/text_align_check.cpp runs all of it without a device.
#pragma once
#include "tedit_host.hpp"

namespace sg {

constexpr uint32_t kTAlignMaxK = 7;  // SMARTGPU_PMIS_MAX (talign.hpp asserts it)

// The walk goes backward from the end position, so the recurrence of edit_align.hpp sees the REVERSED pattern: its bytes
// reversed, or its 32-byte class rows in reverse order (a row itself is a set of byte values and stays as it is).
inline void talign_reverse_bytes(const uint8_t* P, uint32_t m, uint8_t* rev)
{
    for (uint32_t j = 0; j < m; ++j) rev[j] = P[m - 1 - j];
}
inline void talign_reverse_classes(const uint8_t* classes, uint32_t m, uint8_t* rev)
{
    for (uint32_t j = 0; j < m; ++j) std::memcpy(rev + 32u * j, classes + 32u * (m - 1 - j), 32);
}

// THE WINDOW.  A walk from e consumes the bytes e, e - 1, ..., at most 32 * words + kTAlignMaxK of them.  The lane holds the
// ALIGNED dwords that cover them: talign_window_dwords(words) dwords, the last of them text dword e >> 2.  With e % 4 == 0
// byte e is alone in the last dword and the other 32 * words + 6 bytes need ceil(that / 4) more: 11 dwords for one mask
// dword, 19 for two.
SG_HOST_DEVICE constexpr uint32_t talign_window_dwords(uint32_t words) { return 1u + (32u * words + kTAlignMaxK - 1u + 3u) / 4u; }

// The text dword (index relative to text byte 0, in dwords) that window dword 0 holds: negative for e < 4 * (dwords - 1),
// where the window reaches into the zero bytes that lie below text byte 0; a walk never consumes those.
SG_HOST_DEVICE inline long long talign_window_first(uint64_t e, uint32_t dwords)
{
    return static_cast<long long>(e >> 2) - static_cast<long long>(dwords - 1u);
}

// Column j >= 1 of the walk consumes text byte e - (j - 1): byte wb & 3 of window dword wb >> 2, wb as returned here.
// j - 1 < 32 * words + kTAlignMaxK <= 4 * (dwords - 1) + 1, so wb >= 0 whatever e % 4 is.
SG_HOST_DEVICE inline uint32_t talign_window_byte(uint64_t e, uint32_t j, uint32_t dwords)
{
    return 4u * (dwords - 1u) + (static_cast<uint32_t>(e) & 3u) - (j - 1u);
}

// Columns of the walk from e in a range that begins at e_begin <= e: no match starts before e_begin, none is longer than m + k
SG_HOST_DEVICE inline uint32_t talign_columns(uint64_t e, uint64_t e_begin, uint32_t mk)
{
    return e - e_begin + 1 < static_cast<uint64_t>(mk) ? static_cast<uint32_t>(e - e_begin + 1) : mk;
}

}  // namespace sg
