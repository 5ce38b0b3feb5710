// alignl_calls.cpp — the C ABI's align calls for LONG patterns on byte texts: smartgpu_align_editl64 and
// smartgpu_align_editl_classes64 (talignl.hpp, k_talignl.hip).  Host code, compiled with hipcc as api.cpp and match_calls.cpp
// are; what the three units share is host_ctx.hpp (defined in api.cpp) and, with match_calls.cpp's short align calls,
// align_host.hpp.
//
// As everywhere in the C ABI there is no CPU path here: a kernel that is not linked is an error, never a fall-back.
#include "../../include/smartgpu.h"

#include <hip/hip_runtime.h>

#include "host_ctx.hpp"
#include "align_host.hpp"
#include "talignl.hpp"

// The launcher of k_talignl.hip: this unit holds the pointer (null: the calls answer SMARTGPU_ERR_HIP), set by that unit's
// own static initialiser where it is linked.
namespace sg {
hipError_t (*g_text_editl_align)(const TextAlignlArgs&, int, hipStream_t) = nullptr;
}

namespace {

// smartgpu_align_edit64's host path (talign_run in match_calls.cpp) with the long family's bounds, table and entry: the
// checks in the same order, the 256 masks of the REVERSED pattern staged as TEditl::stage stages the forward ones, the
// stream synchronised before upload_positions fills the same staging buffer, then piece after piece.
int talignl_run(const char* call, const uint8_t* pat, bool classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    int rc = check_align_lists(call, ends, count, starts);
    if (rc != SMARTGPU_OK) return rc;
    rc = check_text_args(call, classes ? "classes" : "P", SMARTGPU_EDITL_MAXM, SMARTGPU_EDITL_MAXK, "edits", 0, pat, m, k, 0, text, off, n, &count);
    if (rc != SMARTGPU_OK) return rc;
    if (!ends_in_range(call, ends, count, off, n)) return SMARTGPU_ERR_ARG;
    if (count == 0) return SMARTGPU_OK;
    if (!sg::g_text_editl_align) {
        set_error("%s: this program holds no %s kernel (%s is not linked)", call, "text_editl_align", "k_talignl.hip");
        return SMARTGPU_ERR_HIP;
    }
    uint8_t rev[32 * SMARTGPU_EDITL_MAXM];
    if (classes) sg::talign_reverse_classes(pat, m, rev); else sg::talign_reverse_bytes(pat, m, rev);
    DeviceCtx* d = device_ctx_flushed(text->device);
    if (!d) return SMARTGPU_ERR_HIP;
    if (!batch_reserve(d, sizeof(uint32_t) * 256 * sg::kTEditlWords, 1)) return SMARTGPU_ERR_NOMEM;
    sg::TextAlignlArgs a;
    uint32_t peq[256][sg::kTEditlWords];
    if (classes) sg::editl_peq_classes(rev, m, peq); else sg::editl_peq_bytes(rev, m, peq);
    if (!text_table_stage(d, peq, sg::talignl_words(m), &a.peq) || hipStreamSynchronize(d->stream) != hipSuccess) {
        set_error("%s: %s", call, hipGetErrorString(hipGetLastError()));
        return SMARTGPU_ERR_HIP;
    }
    static_assert(sg::kTextAlignlNone == kAlignEntryNone, "align_pieces unpacks the kernel's entries");
    a.text = text->data();
    a.e_begin = off;
    a.e_end = off + n;
    a.m = m;
    a.k = k;
    return align_pieces(call, d,
                        [&](unsigned long long* io, unsigned long long* dev_ops, uint64_t part) {
                            a.io = io;
                            a.ops = dev_ops;
                            a.count = part;
                            return sg::g_text_editl_align(a, d->num_cus, d->stream);
                        },
                        sg::kTAlignlShift, SMARTGPU_ALIGNL_OPS_WORDS, ends, count, starts, distances, ops);
}

}  // namespace

extern "C" {

int smartgpu_align_editl64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                           const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    return talignl_run("align_editl64", P, false, m, k, text, off, n, ends, count, starts, distances, ops);
}

int smartgpu_align_editl_classes64(const uint8_t* classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                                   const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    return talignl_run("align_editl_classes64", classes, true, m, k, text, off, n, ends, count, starts, distances, ops);
}

}  // extern "C"
