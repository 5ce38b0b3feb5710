// align_calls.cpp — the C ABI's align calls: starts and alignments of edit-distance occurrences, given as a list of END positions,
// one lane (short patterns) or one wave (long patterns) each.  Four families, one per kernel — packed texts (palign.hpp,
// k_palign.hip), packed texts with long patterns (palignl.hpp, k_palignl.hip), byte texts (talign.hpp, k_talign.hip), byte
// texts with long patterns (talignl.hpp, k_talignl.hip) — and ONE host path for the six calls exported here and for the two of
// palignl_calls.cpp, which reach it through palignl_run: align_prepare and align_run.  Host code, compiled with hipcc as api.cpp
// and match_calls.cpp are; what the units share is host_ctx.hpp (defined in api.cpp) and, with match_calls.cpp, call_host.hpp.
//
// As everywhere in the C ABI there is no CPU path here: a kernel that is not linked is an error, never a fall-back.
#include "../../include/smartgpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "call_host.hpp"
#include "palign.hpp"
#include "palignl.hpp"
#include "talign.hpp"
#include "talignl.hpp"

// The launchers of the four kernel units: this unit holds the pointers (null: the calls answer SMARTGPU_ERR_HIP), each set by
// its unit's own static initialiser where that unit is linked.
namespace sg {
hipError_t (*g_planes_edit_align)(const PlaneAlignArgs&, int, hipStream_t) = nullptr;
hipError_t (*g_planes_editl_align)(const PlaneAlignlArgs&, int, int, hipStream_t) = nullptr;
hipError_t (*g_text_edit_align)(const TextAlignArgs&, hipStream_t) = nullptr;
hipError_t (*g_text_editl_align)(const TextAlignlArgs&, int, hipStream_t) = nullptr;
}

namespace {

// copy_positions the other way: the caller's (pageable) end positions to the device through the pinned staging buffer
bool upload_positions(DeviceCtx* d, unsigned long long* dst, const uint64_t* src, uint64_t count)
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

// The device works in the find's own buffer (find_reserve, at most kFindKeep entries, so never an allocation per call beyond
// the first): a piece of `part` occurrences is [io: part entries | ops: words * part words], so a piece is kFindKeep
// occurrences without ops and kFindKeep / (1 + words) with them (3 words: the short calls; 10: the long ones); longer lists go
// through piece after piece.  `launch(io, ops, part)` starts the family's kernel on d->stream over one piece.  An entry comes
// back as (start << shift) | distance, or kAlignNone.
static_assert(sg::kTextAlignNone == sg::kAlignNone && sg::kTextAlignlNone == sg::kAlignNone && sg::kPlaneAlignlNone == sg::kAlignNone,
              "align_pieces unpacks the entries of all four kernels");
template <typename Launch>
int align_pieces(const char* call, DeviceCtx* d, Launch launch, uint32_t shift, uint32_t words, const uint64_t* ends, uint64_t count,
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
            const bool none = v == sg::kAlignNone;
            starts[i] = none ? UINT64_MAX : v >> shift;
            if (distances) distances[i] = none ? 255 : static_cast<uint8_t>(v & ((1u << shift) - 1u));
        }
        done += part;
    }
    return SMARTGPU_OK;
}

// ---- the families.  A family is the call's Question (call_host.hpp) plus the kernel's arguments and what tells it from the
// others: its names, the entry's shift and the words of operations per occurrence, the arena its table needs (0: the masks are
// kernel arguments), `check` (the argument checks that need no device; `count` is never NULL here), `reverse` (the kernels walk
// backward: the masks or the bytes of the REVERSED pattern, and the arguments' head), `stage` (the table to the arena) and
// `launch`.  The bounds on m and k are those of the finds whose entries the kernels take. ----
struct PAlign : PQuestion {
    static constexpr const char* kKernel = "planes_edit_align";
    static constexpr const char* kUnit = "k_palign.hip";
    static constexpr uint32_t kShift = sg::kMisShift, kOpsWords = 3;
    static constexpr size_t kArena = 0;
    sg::PlaneAlignArgs a;

    static bool linked() { return sg::g_planes_edit_align != nullptr; }
    int check(const uint64_t* count)  // and the masks of the pattern AS GIVEN: a bad set is refused by ITS position
    {
        const int rc = check_pedit_args(call, sets ? "sets" : "P", pat, m, SMARTGPU_PEDIT_MAXM, k, SMARTGPU_PMIS_MAX, 0, text, off, n, count);
        return rc != SMARTGPU_OK ? rc : edit_masks(text, pat, m, sets, &a);
    }
    void reverse()
    {
        uint8_t rev[SMARTGPU_PEDIT_MAXM];
        for (uint32_t j = 0; j < m; ++j) rev[j] = pat[m - 1 - j];
        (void)edit_masks(text, rev, m, sets, &a);
        edit_head(a, text, m, k, off, n);
    }
    hipError_t launch(DeviceCtx* d) { return sg::g_planes_edit_align(a, text->planes, d->stream); }
};

// packed texts, long patterns: the masks are eight dwords wide and still kernel arguments
struct PAlignl : PQuestion {
    static constexpr const char* kKernel = "planes_editl_align";
    static constexpr const char* kUnit = "k_palignl.hip";
    static constexpr uint32_t kShift = sg::kPAlignlShift, kOpsWords = SMARTGPU_ALIGNL_OPS_WORDS;
    static constexpr size_t kArena = 0;
    sg::PlaneAlignlArgs a;

    static bool linked() { return sg::g_planes_editl_align != nullptr; }
    int check(const uint64_t* count)  // and the masks of the pattern AS GIVEN: a bad set is refused by ITS position
    {
        const int rc = check_pedit_args(call, sets ? "sets" : "P", pat, m, SMARTGPU_PEDITL_MAXM, k, SMARTGPU_PEDITL_MAXK, 0, text, off, n, count);
        return rc != SMARTGPU_OK ? rc : edit_masks(text, pat, m, sets, &a);
    }
    void reverse()
    {
        uint8_t rev[SMARTGPU_PEDITL_MAXM];
        for (uint32_t j = 0; j < m; ++j) rev[j] = pat[m - 1 - j];
        (void)edit_masks(text, rev, m, sets, &a);
        edit_head(a, text, m, k, off, n);
    }
    hipError_t launch(DeviceCtx* d) { return sg::g_planes_editl_align(a, text->planes, d->num_cus, d->stream); }
};

// the two families on byte texts: what they share.  The table's masks leave from the staging buffer that upload_positions
// fills next, so align_run synchronises the stream behind `stage`.
template <typename Args, int kMaxM, int kMaxK>
struct TextAlign : TQuestion {
    Args a;
    uint8_t rev[32 * kMaxM];

    int check(const uint64_t* count) { return check_text_args(call, sets ? "classes" : "P", kMaxM, kMaxK, "edits", 0, pat, m, k, 0, text, off, n, count); }
    void reverse()
    {
        if (sets) sg::talign_reverse_classes(pat, m, rev); else sg::talign_reverse_bytes(pat, m, rev);
        text_head(a, text, m, k, off, n);
    }
};

struct TAlign : TextAlign<sg::TextAlignArgs, SMARTGPU_EDIT_MAXM, SMARTGPU_PMIS_MAX> {
    static constexpr const char* kKernel = "text_edit_align";
    static constexpr const char* kUnit = "k_talign.hip";
    static constexpr uint32_t kShift = sg::kMisShift, kOpsWords = 3;
    static constexpr size_t kArena = kTEditArena;

    static bool linked() { return sg::g_text_edit_align != nullptr; }
    bool stage(DeviceCtx* d) { return tedit_stage(d, rev, sets, m, &a.peq); }
    hipError_t launch(DeviceCtx* d) { return sg::g_text_edit_align(a, d->stream); }
};

struct TAlignl : TextAlign<sg::TextAlignlArgs, SMARTGPU_EDITL_MAXM, SMARTGPU_EDITL_MAXK> {
    static constexpr const char* kKernel = "text_editl_align";
    static constexpr const char* kUnit = "k_talignl.hip";
    static constexpr uint32_t kShift = sg::kTAlignlShift, kOpsWords = SMARTGPU_ALIGNL_OPS_WORDS;
    static constexpr size_t kArena = kTEditlArena;

    static bool linked() { return sg::g_text_editl_align != nullptr; }
    bool stage(DeviceCtx* d) { return teditl_stage(d, rev, sets, m, &a.peq); }
    hipError_t launch(DeviceCtx* d) { return sg::g_text_editl_align(a, d->num_cus, d->stream); }
};

// ---- ONE host path.  align_prepare is everything that needs no device, in this order: the lists, the family's checks, the
// listed ends, a list of none (*launch stays false), the refusal of a kernel that is not linked, the reversed pattern and the
// arguments' head.  align_run goes on to the device's context with nothing queued, the arena and the table (byte texts), and
// the pieces. ----
template <typename F>
int align_prepare(F& f, const uint64_t* ends, uint64_t count, const uint64_t* starts, bool* launch)
{
    int rc = check_align_lists(f.call, ends, count, starts);
    if (rc != SMARTGPU_OK) return rc;
    if ((rc = f.check(&count)) != SMARTGPU_OK) return rc;
    if (!ends_in_range(f.call, ends, count, f.off, f.n)) return SMARTGPU_ERR_ARG;
    if (count == 0) return SMARTGPU_OK;
    if (!F::linked()) return kernel_missing(f.call, F::kKernel, F::kUnit);
    f.reverse();
    *launch = true;
    return SMARTGPU_OK;
}

template <typename F>
int align_run(const typename F::Q& q, const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    F f;  // (on the stack of the call, as the families of match_calls.cpp: no allocation)
    static_cast<typename F::Q&>(f) = q;
    bool launch = false;
    const int rc = align_prepare(f, ends, count, starts, &launch);
    if (!launch) return rc;
    DeviceCtx* d = device_ctx_flushed(f.text->device);
    if (!d) return SMARTGPU_ERR_HIP;
    if constexpr (F::kArena != 0) {
        if (!batch_reserve(d, F::kArena, 1)) return SMARTGPU_ERR_NOMEM;
        if (!f.stage(d) || hipStreamSynchronize(d->stream) != hipSuccess) {
            set_error("%s: %s", f.call, hipGetErrorString(hipGetLastError()));
            return SMARTGPU_ERR_HIP;
        }
    }
    return align_pieces(f.call, d,
                        [&](unsigned long long* io, unsigned long long* dev_ops, uint64_t part) {
                            f.a.io = io;
                            f.a.ops = dev_ops;
                            f.a.count = part;
                            return f.launch(d);
                        },
                        F::kShift, F::kOpsWords, ends, count, starts, distances, ops);
}

}  // namespace

// packed texts, long patterns (palignl.hpp, k_palignl.hip): the exported calls are palignl_calls.cpp's, this is their host path
int palignl_run(const PQuestion& q, const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    return align_run<PAlignl>(q, ends, count, starts, distances, ops);
}

extern "C" {

/* ---- packed texts (palign.hpp, k_palign.hip) --------------------------------------------------------------------------- */
int smartgpu_palign_edit64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                           const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    return align_run<PAlign>({"palign_edit64", P, false, false, m, k, 0, text, off, n}, ends, count, starts, distances, ops);
}

int smartgpu_palign_sets_edit64(const uint8_t* sets, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                                const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    return align_run<PAlign>({"palign_sets_edit64", sets, true, false, m, k, 0, text, off, n}, ends, count, starts, distances, ops);
}

/* ---- byte texts (talign.hpp, k_talign.hip) ------------------------------------------------------------------------------ */
int smartgpu_align_edit64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                          const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    return align_run<TAlign>({"align_edit64", P, false, false, m, k, 0, text, off, n}, ends, count, starts, distances, ops);
}

int smartgpu_align_edit_classes64(const uint8_t* classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                                  const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    return align_run<TAlign>({"align_edit_classes64", classes, true, false, m, k, 0, text, off, n}, ends, count, starts, distances, ops);
}

/* ---- byte texts, long patterns: m <= 256, k <= 31 (talignl.hpp, k_talignl.hip) ------------------------------------------ */
int smartgpu_align_editl64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                           const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    return align_run<TAlignl>({"align_editl64", P, false, false, m, k, 0, text, off, n}, ends, count, starts, distances, ops);
}

int smartgpu_align_editl_classes64(const uint8_t* classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                                   const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    return align_run<TAlignl>({"align_editl_classes64", classes, true, false, m, k, 0, text, off, n}, ends, count, starts, distances, ops);
}

}  // extern "C"
