// call_host.hpp — what the host units of the C ABI's call layer share: match_calls.cpp (packed texts, the approximate matchers)
// and align_calls.cpp (the align calls).  Two things, each defined ONCE, here: the refusals that need no device — a kernel that
// is not linked, the argument checks of every family, the align lists' —, whose codes, messages and order are fixed by
// tests/golden/host_call_cases.json (tests/host_calls_check.cpp runs them on the CPU) and tests/golden/refusal_messages.json; and
// what a find and its align call both need before a launch: the pattern as masks or as a staged table, and the head of the
// kernel's arguments.  Host only, built on host_ctx.hpp; included by those two units and by no kernel unit.
#pragma once
#include <cstring>
#include <type_traits>

#include "host_ctx.hpp"
#include "pedit.hpp"
#include "peditl.hpp"
#include "talignl.hpp"
#include "tedit_host.hpp"
#include "teditl_host.hpp"

#pragma GCC visibility push(hidden)

// A call as its family receives it (the families: PlaneCall, PEditCall, TextCall in match_calls.cpp; PAlign, PAlignl, TAlign, TAlignl)
template <typename Text>
struct Question {
    using Q = Question;
    const char* call;    // the entry point's name in messages
    const uint8_t* pat;  // m bytes, or — `sets` — m sets of codes (packed texts) or m classes of 32 bytes (byte texts)
    bool sets;
    bool mis;            // plane kinds only: the call takes k and reports distances
    uint32_t m, k, flags;  // flags: the long edit families only
    const Text* text;
    uint64_t off, n;
};
using PQuestion = Question<smartgpu_ptext>;
using TQuestion = Question<smartgpu_text>;

// ---- refusals ----

// A kernel this program does not hold (its unit is not linked): an error, never a fall-back.
inline int kernel_missing(const char* call, const char* kernel, const char* unit)
{
    set_error("%s: this program holds no %s kernel (%s is not linked)", call, kernel, unit);
    return SMARTGPU_ERR_HIP;
}

// A find with room for entries and no array to put them in; `what` names the array.
inline int check_room(const char* call, const char* what, const void* out, uint64_t cap)
{
    if (!cap || out) return SMARTGPU_OK;
    set_error("%s: %s NULL with cap > 0", call, what);
    return SMARTGPU_ERR_ARG;
}

// A set pattern that names a code the text does not hold.  `bad`: what the set encoders return, the first such position, or
// a negative number for none.
inline int refuse_code(const smartgpu_ptext* t, const uint8_t* sets, int bad)
{
    if (bad < 0) return SMARTGPU_OK;
    set_error("set pattern: position %d: set 0x%02x names a code >= %d, the number of values the text holds", bad, sets[bad], t->nvalues);
    return SMARTGPU_ERR_ARG;
}

inline int check_psearch_args(const uint8_t* P, uint32_t m, const smartgpu_ptext* text, uint64_t off, uint64_t n)
{
    if (!P || m < 1 || m > SMARTGPU_XSIZE) { set_error("pattern length %u outside [1,%d]", m, SMARTGPU_XSIZE); return SMARTGPU_ERR_ARG; }
    if (!text) { set_error("packed text handle is NULL"); return SMARTGPU_ERR_ARG; }
    if (off > text->n || n > text->n - off) { set_error("range [%llu,+%llu) outside the packed text (%llu symbols)", (unsigned long long)off, (unsigned long long)n, (unsigned long long)text->n); return SMARTGPU_ERR_ARG; }
    return SMARTGPU_OK;
}

// The checks of the set, mis and sets-mis calls that need no device; `what` names the pattern argument, k = 0 without mismatches.
inline int check_pext_args(const char* call, const char* what, const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off,
                           uint64_t n, const uint64_t* count)
{
    if (!P) { set_error("%s: %s is NULL", call, what); return SMARTGPU_ERR_ARG; }
    if (k > SMARTGPU_PMIS_MAX) { set_error("%s: k = %u mismatches, at most %d", call, k, SMARTGPU_PMIS_MAX); return SMARTGPU_ERR_ARG; }
    const int rc = check_psearch_args(P, m, text, off, n);
    if (rc != SMARTGPU_OK) return rc;
    if (!count) { set_error("%s: count must not be NULL", call); return SMARTGPU_ERR_ARG; }
    return SMARTGPU_OK;
}

// The edit-distance and alignment calls do not read a third plane.
inline int refuse_planes3(const char* call, const smartgpu_ptext* text)
{
    if (text->planes != 3) return SMARTGPU_OK;
    set_error("%s: three-plane texts (five to eight values) are not offered here: edit distance and alignments read one or two planes", call);
    return SMARTGPU_ERR_ARG;
}

// The checks of the edit, editl and align calls on a packed text that need no device; `what` names the pattern argument,
// max_m and max_k are the family's, flags is 0 for a call that takes none.
inline int check_pedit_args(const char* call, const char* what, const uint8_t* P, uint32_t m, uint32_t max_m, uint32_t k, uint32_t max_k, uint32_t flags,
                            const smartgpu_ptext* text, uint64_t off, uint64_t n, const uint64_t* count)
{
    if (!P) { set_error("%s: %s is NULL", call, what); return SMARTGPU_ERR_ARG; }
    if (m < 1 || m > max_m) { set_error("%s: pattern length %u outside [1,%u]", call, m, max_m); return SMARTGPU_ERR_ARG; }
    if (k > max_k) { set_error("%s: k = %u edits, at most %u", call, k, max_k); return SMARTGPU_ERR_ARG; }
    if (flags & ~SMARTGPU_PEDITL_ALL_BLOCKS) { set_error("%s: flags 0x%x: only SMARTGPU_PEDITL_ALL_BLOCKS (0x%x) is defined", call, flags, SMARTGPU_PEDITL_ALL_BLOCKS); return SMARTGPU_ERR_ARG; }
    if (!text) { set_error("packed text handle is NULL"); return SMARTGPU_ERR_ARG; }
    if (refuse_planes3(call, text) != SMARTGPU_OK) return SMARTGPU_ERR_ARG;
    if (off > text->n || n > text->n - off) { set_error("range [%llu,+%llu) outside the packed text (%llu symbols)", (unsigned long long)off, (unsigned long long)n, (unsigned long long)text->n); return SMARTGPU_ERR_ARG; }
    if (!count) { set_error("%s: count must not be NULL", call); return SMARTGPU_ERR_ARG; }
    return SMARTGPU_OK;
}

// BYTE texts: the checks of the edit, editl, mis and align calls that need no device; `what` names the pattern argument,
// max_m and max_k are the family's, `noun` is what k counts, `flags_mask` the flag bits the family defines (0 for a call
// that takes none, which passes flags = 0).
inline int check_text_args(const char* call, const char* what, int max_m, int max_k, const char* noun, uint32_t flags_mask, const uint8_t* P, uint32_t m,
                           uint32_t k, uint32_t flags, const smartgpu_text* text, uint64_t off, uint64_t n, const uint64_t* count)
{
    if (!P) { set_error("%s: %s is NULL", call, what); return SMARTGPU_ERR_ARG; }
    if (m < 1 || m > (uint32_t)max_m) { set_error("%s: pattern length %u outside [1,%d]", call, m, max_m); return SMARTGPU_ERR_ARG; }
    if (k > (uint32_t)max_k) { set_error("%s: k = %u %s, at most %d", call, k, noun, max_k); return SMARTGPU_ERR_ARG; }
    if (flags & ~flags_mask) { set_error("%s: flags 0x%x: only SMARTGPU_EDITL_ALL_BLOCKS (0x%x) is defined", call, flags, flags_mask); return SMARTGPU_ERR_ARG; }
    if (!text) { set_error("%s: text handle is NULL", call); return SMARTGPU_ERR_ARG; }
    if (off > text->n || n > text->n - off) { set_error("%s: range [%llu,+%llu) outside the text (%llu bytes)", call, (unsigned long long)off, (unsigned long long)n, (unsigned long long)text->n); return SMARTGPU_ERR_ARG; }
    if (!count) { set_error("%s: count must not be NULL", call); return SMARTGPU_ERR_ARG; }
    return SMARTGPU_OK;
}

// The refusals of an align call's lists.  An array that is missing: before every other check
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

// ---- edit distance on a packed text (pedit.hpp, peditl.hpp, palign.hpp): the masks are kernel arguments ----

// The fields that PlaneEditArgs, PlaneEditlArgs and PlaneAlignArgs share
template <typename Args>
inline void edit_head(Args& a, const smartgpu_ptext* text, uint32_t m, uint32_t k, uint64_t off, uint64_t n)
{
    a.p0 = text->plane(0);
    a.p1 = text->plane(text->planes - 1);
    a.e_begin = off;
    a.e_end = off + n;
    a.m = m;
    a.k = k;
}

// The pattern's masks for a checked call (a->peq of PlaneEditArgs and PlaneAlignArgs, two dwords wide, or of PlaneEditlArgs
// and PlaneAlignlArgs, eight): from bytes (sets == false) or from sets.  SMARTGPU_ERR_ARG: a set names a code the text does not hold.
template <typename Args>
inline int edit_masks(const smartgpu_ptext* t, const uint8_t* pat, uint32_t m, bool sets, Args* a)
{
    constexpr bool kLong = std::is_same<decltype(Args::peq), uint32_t[4][sg::kEditlWords]>::value;
    if (!sets) {
        if constexpr (kLong) sg::editl_peq_pattern(t->values, t->nvalues, pat, m, a->peq);
        else sg::edit_peq_pattern(t->values, t->nvalues, pat, m, a->peq);
        return SMARTGPU_OK;
    }
    if constexpr (kLong) return refuse_code(t, pat, sg::editl_peq_sets(t->nvalues, pat, m, a->peq));
    else return refuse_code(t, pat, sg::edit_peq_sets(t->nvalues, pat, m, a->peq));
}

// ---- BYTE texts (tedit.hpp, teditl.hpp, tmis.hpp, talign.hpp, talignl.hpp): the pattern is 256 masks, too many for kernel
// arguments.  They travel as the kernel's table (edit_peq_table: 1 or 2 dwords per byte value; editl_peq_table: word-major,
// 2, 4 or 8) through the staging buffer into the arena, as psearch_impl's patterns travel.  The staging buffer is free: every
// call that fills it ends with a synchronisation. ----

// what TextEditArgs, TextEditlArgs, TextMisArgs, TextAlignArgs and TextAlignlArgs share: the text and the range, the pattern's
// length and k
template <class Args>
inline void text_head(Args& a, const smartgpu_text* text, uint32_t m, uint32_t k, uint64_t off, uint64_t n)
{
    a.text = text->data();
    a.e_begin = off;
    a.e_end = off + n;
    a.m = m;
    a.k = k;
}

template <uint32_t W>
inline bool text_table_stage(DeviceCtx* d, const uint32_t (&table)[256][W], uint32_t words, const uint32_t** dev)
{
    if constexpr (W == sg::kTEditlWords) sg::editl_peq_table(table, words, reinterpret_cast<uint32_t*>(d->pinned));
    else sg::edit_peq_table(table, words, reinterpret_cast<uint32_t*>(d->pinned));
    *dev = reinterpret_cast<const uint32_t*>(d->arena);
    return hipMemcpyAsync(d->arena, d->pinned, 256 * 4 * words, hipMemcpyHostToDevice, d->stream) == hipSuccess;
}

// The short families (m <= 64): bytes or classes as tedit_host.hpp's masks "position j accepts this byte", for the edit calls
// and, with the reversed pattern, the align calls.  kTEditArena: the arena a table needs at most.
constexpr size_t kTEditArena = sizeof(uint32_t) * 256 * sg::kTEditWords;
inline bool tedit_stage(DeviceCtx* d, const uint8_t* pat, bool classes, uint32_t m, const uint32_t** dev)
{
    uint32_t peq[256][sg::kTEditWords];
    if (classes) sg::edit_peq_classes(pat, m, peq); else sg::edit_peq_bytes(pat, m, peq);
    return text_table_stage(d, peq, m <= 32 ? 1u : 2u, dev);
}

// The long families (m <= 256): teditl_host.hpp's masks, eight dwords wide, of which the kernels read talignl_words(m) — the
// WORDS of k_teditl.hip and k_talignl.hip alike: 2, 4 or 8 KiB of table
constexpr size_t kTEditlArena = sizeof(uint32_t) * 256 * sg::kTEditlWords;
inline bool teditl_stage(DeviceCtx* d, const uint8_t* pat, bool classes, uint32_t m, const uint32_t** dev)
{
    uint32_t peq[256][sg::kTEditlWords];
    if (classes) sg::editl_peq_classes(pat, m, peq); else sg::editl_peq_bytes(pat, m, peq);
    return text_table_stage(d, peq, sg::talignl_words(m), dev);
}

#pragma GCC visibility pop
