// align_host.hpp — what the host units of the align calls share: match_calls.cpp (smartgpu_palign_edit64, smartgpu_align_edit64
// and their set and class forms) and alignl_calls.cpp (smartgpu_align_editl64).  The checks of a byte-text call, the refusals of
// the lists, the lists' way to the device, the piece-wise loop over the find's buffer, and the staging of a byte text's 256
// masks.  Host only, built on host_ctx.hpp; included by those two units and by no kernel unit.  Every function here was
// match_calls.cpp's own before the long align calls needed it too: codes, messages and the order of the checks are unchanged
// (tests/test_refusal_messages.py).
#pragma once
#include <algorithm>
#include <cstring>

#include "host_ctx.hpp"
#include "tedit_host.hpp"
#include "teditl_host.hpp"

#pragma GCC visibility push(hidden)

// BYTE texts: the checks of the edit, editl, mis and align calls that need no device (defined in match_calls.cpp, beside the
// packed texts' checks); `what` names the pattern argument, max_m and max_k are the family's, `noun` is what k counts,
// `flags_mask` the flag bits the family defines (0 for a call that takes none, which passes flags = 0).
int check_text_args(const char* call, const char* what, int max_m, int max_k, const char* noun, uint32_t flags_mask, const uint8_t* P, uint32_t m,
                    uint32_t k, uint32_t flags, const smartgpu_text* text, uint64_t off, uint64_t n, const uint64_t* count);

// The pattern of a byte text is 256 masks, too many for kernel arguments: they travel as the kernel's table (edit_peq_table:
// 1 or 2 dwords per byte value; editl_peq_table: word-major, 2, 4 or 8) through the staging buffer into the arena, as
// psearch_impl's patterns travel.  The staging buffer is free: every call that fills it ends with a synchronisation.
template <uint32_t W>
inline bool text_table_stage(DeviceCtx* d, const uint32_t (&table)[256][W], uint32_t words, const uint32_t** dev)
{
    if constexpr (W == sg::kTEditlWords) sg::editl_peq_table(table, words, reinterpret_cast<uint32_t*>(d->pinned));
    else sg::edit_peq_table(table, words, reinterpret_cast<uint32_t*>(d->pinned));
    *dev = reinterpret_cast<const uint32_t*>(d->arena);
    return hipMemcpyAsync(d->arena, d->pinned, 256 * 4 * words, hipMemcpyHostToDevice, d->stream) == hipSuccess;
}

// copy_positions the other way: the caller's (pageable) end positions to the device through the pinned staging buffer
inline bool upload_positions(DeviceCtx* d, unsigned long long* dst, const uint64_t* src, uint64_t count)
{
    for (uint64_t done = 0; done < count;) {
        const uint64_t part = std::min<uint64_t>(count - done, d->pinned_bytes / 8);
        std::memcpy(d->pinned, src + done, part * 8);
        if (hipMemcpyAsync(dst + done, d->pinned, part * 8, hipMemcpyHostToDevice, d->stream) != hipSuccess ||
            hipStreamSynchronize(d->stream) != hipSuccess)
            return false;
        done += part;
    }
    return true;
}

// The refusals of the lists, shared by the align calls.  An array that is missing: before every other check
inline int check_align_lists(const char* call, const uint64_t* ends, uint64_t count, const uint64_t* starts)
{
    if (count && !ends) { set_error("%s: ends NULL with count > 0", call); return SMARTGPU_ERR_ARG; }
    if (count && !starts) { set_error("%s: starts NULL with count > 0", call); return SMARTGPU_ERR_ARG; }
    return SMARTGPU_OK;
}

// A listed end outside the range [off, off+n): after the other checks; the message names i and the value
inline bool ends_in_range(const char* call, const uint64_t* ends, uint64_t count, uint64_t off, uint64_t n)
{
    for (uint64_t i = 0; i < count; ++i)
        if (ends[i] < off || ends[i] - off >= n) {
            set_error("%s: ends[%llu] = %llu outside the range [%llu,+%llu)", call, (unsigned long long)i, (unsigned long long)ends[i], (unsigned long long)off, (unsigned long long)n);
            return false;
        }
    return true;
}

// Every align call.  The device works in the find's own buffer (find_reserve, at most kFindKeep entries, so never an
// allocation per call beyond the first): a piece of `part` occurrences is [io: part entries | ops: words * part words], so a
// piece is kFindKeep occurrences without ops and kFindKeep / (1 + words) with them (3 words: the short calls; 10: the long
// ones); longer lists go through piece after piece.  `launch(io, ops, part)` starts the family's kernel on d->stream over
// one piece.  An entry comes back as (start << shift) | distance, or kAlignEntryNone.
constexpr unsigned long long kAlignEntryNone = ~0ull;
template <typename Launch>
inline int align_pieces(const char* call, DeviceCtx* d, Launch launch, uint32_t shift, uint32_t words, const uint64_t* ends, uint64_t count,
                        uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    const uint64_t piece = ops ? kFindKeep / (1 + words) : kFindKeep;
    for (uint64_t done = 0; done < count;) {
        const uint64_t part = std::min<uint64_t>(count - done, piece);
        bool own = false;
        unsigned long long* buf = find_reserve(d, part * (ops ? 1 + words : 1), &own);
        if (!buf) return SMARTGPU_ERR_NOMEM;
        unsigned long long* const dev_ops = ops ? buf + part : nullptr;
        const bool ok = upload_positions(d, buf, ends + done, part) &&
                        launch(buf, dev_ops, part) == hipSuccess &&
                        hipStreamSynchronize(d->stream) == hipSuccess &&
                        copy_positions(d, starts + done, buf, part) &&
                        (!ops || copy_positions(d, ops + words * done, dev_ops, words * part));
        if (!ok) set_error("%s: %s", call, hipGetErrorString(hipGetLastError()));
        if (own) (void)hipFree(buf);
        if (!ok) return SMARTGPU_ERR_HIP;
        for (uint64_t i = done; i < done + part; ++i) {
            const uint64_t v = starts[i];
            const bool none = v == kAlignEntryNone;
            starts[i] = none ? UINT64_MAX : v >> shift;
            if (distances) distances[i] = none ? 255 : static_cast<uint8_t>(v & ((1u << shift) - 1u));
        }
        done += part;
    }
    return SMARTGPU_OK;
}

#pragma GCC visibility pop
