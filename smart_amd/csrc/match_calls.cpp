// match_calls.cpp — the C ABI's calls on PACKED texts (bit planes: planes.hpp, planes3.hpp) and the approximate matchers on both
// kinds of text (mismatches, edit distance).  Host code, compiled with hipcc as api.cpp is.  api.cpp keeps texts, plans, the
// launch queue and the exact calls on byte texts, and defines what host_ctx.hpp declares for this unit; the align calls are
// align_calls.cpp, which shares call_host.hpp with this unit: the refusals that need no device, the masks, the staged tables.
//
// As in api.cpp there is no CPU search path here: a kernel that is not linked is an error, never a fall-back.
#include "../../include/smartgpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "call_host.hpp"
#include "pedit.hpp"
#include "peditl.hpp"
#include "tedit.hpp"
#include "teditl.hpp"
#include "tmis.hpp"
#include "planes.hpp"
#include "planes_host.hpp"
#include "planes3.hpp"
#include "planes3_host.hpp"

// The launchers of the units that register themselves: this unit holds the pointers (null: the calls answer
// SMARTGPU_ERR_HIP), each set by its unit's own static initialiser where that unit is linked.
namespace sg {
// pedit.hpp: k_pedit.hip
hipError_t (*g_planes_edit_scan)(const PlaneEditArgs&, int, int, hipStream_t) = nullptr;
hipError_t (*g_planes_edit_find)(const PlaneEditArgs&, unsigned long long*, unsigned long long, int, int, hipStream_t) = nullptr;
// peditl.hpp: k_peditl.hip
hipError_t (*g_planes_editl_scan)(const PlaneEditlArgs&, int, int, hipStream_t) = nullptr;
hipError_t (*g_planes_editl_find)(const PlaneEditlArgs&, unsigned long long*, unsigned long long, int, int, hipStream_t) = nullptr;
// tedit.hpp: k_tedit.hip
hipError_t (*g_text_edit_scan)(const TextEditArgs&, int, hipStream_t) = nullptr;
hipError_t (*g_text_edit_find)(const TextEditArgs&, unsigned long long*, unsigned long long, int, hipStream_t) = nullptr;
// teditl.hpp: k_teditl.hip
hipError_t (*g_text_editl_scan)(const TextEditlArgs&, int, hipStream_t) = nullptr;
hipError_t (*g_text_editl_find)(const TextEditlArgs&, unsigned long long*, unsigned long long, int, hipStream_t) = nullptr;
// tmis.hpp: k_tmis.hip
hipError_t (*g_text_mis_scan)(const TextMisArgs&, int, hipStream_t) = nullptr;
hipError_t (*g_text_mis_find)(const TextMisArgs&, unsigned long long*, unsigned long long, int, hipStream_t) = nullptr;
// planes3.hpp: k_planes3.hip
hipError_t (*g_planes3_pack)(const uint8_t*, uint64_t, uint32_t*, uint32_t*, uint32_t*, const uint8_t[7], hipStream_t) = nullptr;
hipError_t (*g_planes3_scan)(const Plane3Args&, int, int, hipStream_t) = nullptr;
hipError_t (*g_planes3_find)(const Plane3Args&, unsigned long long*, unsigned long long, int, int, hipStream_t) = nullptr;
}

namespace {

// ---- ONE host path for every single-pattern count and find on a packed text and for the approximate matchers on a byte
// text: count_run and find_run.  The skeleton fixes the order of the steps — the device's context with nothing queued, the
// arena (batch_reserve), for a find the entries' device buffer (find_reserve; none: the call still counts), the family's
// staging, the slot's memset, the kernel, the read-back, the synchronisation —, the refusal of a count or cursor beyond
// the bound, what *count receives, the find's outcomes (planes_host.hpp: find_outcome) with their return codes and texts,
// and the times (pre: arena and staging; run: memset to synchronisation; counts only).  A family supplies its names
// (RunNames), its bound — n - m + 1 start positions, or n end positions whatever m is —, the bytes it stages into the
// arena, and two lambdas: `stage` (may do nothing; false is a HIP error) and `launch` (fills what its arguments need of the
// device — the result slot is d->batch_counts — and launches).  A find adds a third, `order`: the entries in ascending
// order, or set_error and false for what its kernel cannot have written.  What needs no launch a family answers before
// it comes here (its prepare step, below). ----
struct RunNames {
    const char* call;     // the entry point: "<call>: ..." for what the caller can mend
    const char* kernel;   // the kernel, for refusals of what the device wrote
    const char* bound;    // what the bound counts: "start positions", "end positions"
    const char* entries;  // what a find lists: "positions", "entries"
};

template <typename Stage, typename Launch>
int count_run(const RunNames& w, int device, size_t arena_bytes, uint64_t bound, Stage stage, Launch launch, uint64_t* count, double* pre_ms,
              double* run_ms)
{
    DeviceCtx* d = device_ctx_flushed(device);
    if (!d) return SMARTGPU_ERR_HIP;
    const double t_pre = now_ms();
    if (!batch_reserve(d, arena_bytes, 1)) return SMARTGPU_ERR_NOMEM;
    if (!stage(d)) { set_error("%s: %s", w.call, hipGetErrorString(hipGetLastError())); return SMARTGPU_ERR_HIP; }
    const double pre = now_ms() - t_pre;
    const double t0 = now_ms();
    HIP_TRY(hipMemsetAsync(d->batch_counts, 0, sizeof(unsigned long long), d->stream), return SMARTGPU_ERR_HIP);
    HIP_TRY(launch(d), return SMARTGPU_ERR_HIP);
    HIP_TRY(hipMemcpyAsync(d->pinned_counts, d->batch_counts, sizeof(unsigned long long), hipMemcpyDeviceToHost, d->stream), return SMARTGPU_ERR_HIP);
    HIP_TRY(hipStreamSynchronize(d->stream), return SMARTGPU_ERR_HIP);
    const double run = now_ms() - t0;
    // more occurrences than positions: refused like a poisoned count, never reported
    if (d->pinned_counts[0] > bound) { set_error("%s: count %llu exceeds the %llu %s", w.kernel, (unsigned long long)d->pinned_counts[0], (unsigned long long)bound, w.bound); return SMARTGPU_ERR_HIP; }
    return pcount_done(d->pinned_counts[0], pre, run, count, pre_ms, run_ms);
}

// *count receives the number of occurrences whenever the device answered with a cursor within the bound, on
// SMARTGPU_ERR_NOMEM too; `entries` receives the list, in order, on SMARTGPU_OK only, and nothing behind entries[cap] is
// touched.  The entries reach `order` as the kernel wrote them; unpacking distances is the caller's.
template <typename Stage, typename Launch, typename Order>
int find_run(const RunNames& w, int device, size_t arena_bytes, uint64_t bound, Stage stage, Launch launch, Order order, uint64_t* entries,
             uint64_t cap, uint64_t* count)
{
    DeviceCtx* d = device_ctx_flushed(device);
    if (!d) return SMARTGPU_ERR_HIP;
    if (!batch_reserve(d, arena_bytes, 1)) return SMARTGPU_ERR_NOMEM;
    const uint64_t room = cap < bound ? cap : bound;  // no more entries than positions
    bool own = false;
    unsigned long long* out = nullptr;
    uint64_t room_got = room;
    if (room && !(out = find_reserve(d, room, &own))) room_got = 0;  // no device room: the call still counts
    const bool ok = stage(d) && hipMemsetAsync(d->batch_counts, 0, sizeof(unsigned long long), d->stream) == hipSuccess &&
                    launch(d, out, room_got) == hipSuccess &&
                    hipMemcpyAsync(d->pinned_counts, d->batch_counts, sizeof(unsigned long long), hipMemcpyDeviceToHost, d->stream) == hipSuccess &&
                    hipStreamSynchronize(d->stream) == hipSuccess;
    const unsigned long long total = ok ? d->pinned_counts[0] : 0;
    int r = SMARTGPU_OK;
    if (!ok) {
        set_error("%s: %s", w.call, hipGetErrorString(hipGetLastError()));
        r = SMARTGPU_ERR_HIP;
    } else switch (sg::find_outcome(total, bound, room_got, cap)) {
    case sg::FindOutcome::kBeyondBound:
        set_error("%s: cursor %llu exceeds the %llu %s", w.kernel, total, (unsigned long long)bound, w.bound);
        r = SMARTGPU_ERR_HIP;
        break;
    case sg::FindOutcome::kComplete:
        if (total && !copy_positions(d, entries, out, total)) {
            set_error("%s: %s", w.call, hipGetErrorString(hipGetLastError()));
            r = SMARTGPU_ERR_HIP;
        } else if (total && !order(entries, total)) {
            r = SMARTGPU_ERR_HIP;
        }
        break;
    case sg::FindOutcome::kOverCap:
        set_error("%s: %llu occurrences, room for %llu", w.call, total, (unsigned long long)cap);
        r = SMARTGPU_ERR_NOMEM;
        break;
    case sg::FindOutcome::kNoRoom:
        set_error("%s: %llu occurrences, room for %llu, but the device has no memory for %llu %s", w.call, total, (unsigned long long)cap, (unsigned long long)room, w.entries);
        r = SMARTGPU_ERR_NOMEM;
        break;
    }
    if (own) (void)hipFree(out);
    if (r != SMARTGPU_ERR_HIP) *count = total;
    return r;
}

// find_run's `order` for the kernels that write spans (planes.hpp): order_spans over the positions [lo, hi]
bool spans_in_order(const RunNames& w, uint64_t* entries, uint64_t total, uint64_t lo, uint64_t hi, uint32_t shift)
{
    if (sg::order_spans(entries, total, lo, hi, shift)) return true;
    set_error("%s: the %s are not ascending spans of %llu %s", w.kernel, w.entries, (unsigned long long)sg::kFindSpan, w.bound);
    return false;
}

// and for the long-pattern edit kernels, which write their entries in no order (peditl.hpp, teditl.hpp): order_editl sorts them
bool editl_in_order(const RunNames& w, uint64_t* entries, uint64_t total, uint64_t lo, uint64_t hi, uint32_t k, uint32_t shift)
{
    if (sg::order_editl(entries, total, lo, hi, k, shift)) return true;
    set_error("%s: the entries are not distinct end positions of the range with distances <= %u", w.kernel, k);
    return false;
}

// A find without a launch: `total` occurrences at the first `total` start positions of the range (0: none; full sets: all)
int find_every_start(const char* call, uint64_t off, uint64_t total, uint64_t* positions, uint64_t cap, uint64_t* count)
{
    *count = total;
    if (total > cap) { set_error("%s: %llu occurrences, room for %llu", call, (unsigned long long)total, (unsigned long long)cap); return SMARTGPU_ERR_NOMEM; }
    for (uint64_t i = 0; i < total; ++i) positions[i] = off + i;
    return SMARTGPU_OK;
}

// The entries of a find with distances, position << shift | distance in ascending order, unpacked in place.
void unpack_mis(uint64_t* positions, uint8_t* mismatches, uint64_t count, uint32_t shift = sg::kMisShift)
{
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t e = positions[i];
        if (mismatches) mismatches[i] = static_cast<uint8_t>(e & ((1u << shift) - 1u));
        positions[i] = e >> shift;
    }
}

// ---- ONE prepare step per family, used by its count and by its find.  A call is a Question (call_host.hpp); a family (PlaneCall,
// PEditCall, TextCall below) is the question plus what `prepare` leaves for count_run / find_run.  prepare decides, in this order: the
// checks that need no device, the pattern's masks, what is answered without a launch, the refusal of a kernel that is not
// linked, the arguments' head, the names and the bound.  Behind it a family has `stage`, `scan`, `find`, `order` (find_run's
// lambdas) and `post` (the entries as the caller gets them).  run_count and run_find are all that tells a count from a
// find: *count = 0 against pcount_done(0), find_every_start, the room check, the launcher.  Families live on the stack of
// the call: no allocation, no indirect call beyond the launcher's pointer. ----

// What prepare answers.  rc != SMARTGPU_OK: refused, the message is set.  Otherwise a launch, or none: the first `every` start
// positions of the range are the occurrences (0: there is none; n - m + 1: a pattern of full sets).
struct Prepared {
    int rc;
    bool launch;
    uint64_t every;
};
constexpr Prepared refused(int rc) { return {rc, false, 0}; }
constexpr Prepared answered(uint64_t every) { return {SMARTGPU_OK, false, every}; }
constexpr Prepared kLaunch = {SMARTGPU_OK, true, 0};

template <typename Call, typename Q>
int run_count(const Q& q, uint64_t* count, double* pre_ms, double* run_ms)
{
    Call f{q};
    const Prepared p = f.prepare(false, count);
    if (p.rc != SMARTGPU_OK) return p.rc;
    if (!p.launch) return pcount_done(p.every, 0.0, 0.0, count, pre_ms, run_ms);
    return count_run(f.w, q.text->device, f.arena, f.bound, [&](DeviceCtx* d) { return f.stage(d); }, [&](DeviceCtx* d) { return f.scan(d); }, count,
                     pre_ms, run_ms);
}

// `what` names the entries' array for the refusal of room without one, which comes before every other check
template <typename Call, typename Q>
int run_find(const Q& q, const char* what, uint64_t* entries, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    const int rc = check_room(q.call, what, entries, cap);
    if (rc != SMARTGPU_OK) return rc;
    Call f{q};
    const Prepared p = f.prepare(true, count);
    if (p.rc != SMARTGPU_OK) return p.rc;
    if (!p.launch) return find_every_start(q.call, q.off, p.every, entries, cap, count);
    const int r = find_run(f.w, q.text->device, f.arena, f.bound, [&](DeviceCtx* d) { return f.stage(d); },
                           [&](DeviceCtx* d, unsigned long long* out, uint64_t room) { return f.find(d, out, room); },
                           [&](uint64_t* e, uint64_t total) { return f.order(e, total); }, entries, cap, count);
    if (r == SMARTGPU_OK) f.post(entries, distances, *count);
    return r;
}

// the name to report of a family's kernel that is not linked (null: it is), for the families whose launchers are a pair of pointers
template <typename F>
const char* missing_kernel(bool find)
{
    return (find ? F::find() != nullptr : F::scan() != nullptr) ? nullptr : F::kKernel[find];
}

// ---- the plane matchers (planes.hpp, planes3.hpp): exact, sets, mis and sets-mis on one or two planes, and ALL of them
// through one kernel pair on three ----

// The head every packed kernel's arguments share (PlaneArgs, PlaneSetArgs, PlaneMisArgs, PlaneSetMisArgs), n >= m: the planes,
// the start positions, the pattern's planes in the device's arena (read when m > 32 only) and result slot d->batch_counts[k].
template <typename Args>
void plane_head(Args& a, const DeviceCtx* d, const smartgpu_ptext* text, uint32_t m, uint64_t off, uint64_t n, uint32_t k = 0)
{
    a.p0 = text->plane(0);
    a.p1 = text->plane(text->planes - 1);
    a.s_begin = off;
    a.s_end = off + n - m + 1;
    a.m = m;
    a.pat = reinterpret_cast<const uint32_t*>(d->arena);
    a.count = d->batch_counts + k;
}

// plane_head for a three-plane text (Plane3Args: planes3.hpp)
void plane_head(sg::Plane3Args& a, const DeviceCtx* d, const smartgpu_ptext* text, uint32_t m, uint64_t off, uint64_t n, uint32_t k = 0)
{
    plane_head<sg::Plane3Args>(a, d, text, m, off, n, k);
    a.p1 = text->plane(1);
    a.p2 = text->plane(2);
}

// a.y of PlaneSetArgs and PlaneSetMisArgs (four membership planes) and of Plane3Args (eight): the first dword of each plane at Y
template <typename Args>
void set_words(Args& a, const uint32_t* Y)
{
    for (uint32_t c = 0; c < sizeof a.y / sizeof a.y[0]; ++c) a.y[c] = Y[c * sg::kPatWords];
}

// encode_sets for a checked call.  SMARTGPU_ERR_ARG: a set names a code the text does not hold.
int sets_planes(const smartgpu_ptext* t, const uint8_t* sets, uint32_t m, bool fill_empty, uint32_t* Y, uint32_t* empty, bool* full)
{
    return refuse_code(t, sets, sg::encode_sets(t->nvalues, sets, m, fill_empty, Y, empty, full));
}

// The pattern's planes (`bytes` at `words`) through the staging buffer into the device's arena, for m > 32 only: the first
// 32 positions travel as kernel arguments.
bool stage_pattern(DeviceCtx* d, const uint32_t* words, size_t bytes, uint32_t m)
{
    if (m <= 32) return true;
    // (the staging buffer is free: every call that fills it ends with a synchronisation of the device's stream)
    std::memcpy(d->pinned, words, bytes);
    return hipMemcpyAsync(d->arena, d->pinned, bytes, hipMemcpyHostToDevice, d->stream) == hipSuccess;
}

// A KIND of plane matcher: its arguments, the dwords of a pattern's planes, its kernel pair and `encode` — the pattern as
// planes at W[kWords] (staged when m > 32) and as the kind's own fields of *a; *none: the positions that accept nothing (a
// byte the text does not hold, an empty set), which a mismatch kind adds to every distance as a.foreign, leaving
// a.budget = k - *none for the compared positions; *full: every position accepts every value.  SMARTGPU_ERR_ARG: a set
// names a code the text does not hold.  Exact and Three also serve the batch calls (psearch_impl): there pattern k of a set
// is staged at host_pat + k * kWords and, for m > 32, at the same stride in the device's arena.
struct Exact {
    using Args = sg::PlaneArgs;
    static constexpr size_t kWords = 2 * sg::kPatWords;  // one pattern's two code planes
    static constexpr const char* kKernel[2] = {"planes_scan", "planes_find"};
    static constexpr const char* kUnit = "k_planes.hip";
    static const char* missing(bool) { return nullptr; }  // k_planes.hip is part of every program
    static auto scan() { return sg::launch_planes_scan; }
    static auto find() { return sg::launch_planes_find; }
    static int encode(const PQuestion& q, uint32_t* X, Args* a, uint32_t* none, bool*)
    {
        *none = sg::encode_pattern(q.text->values, q.text->nvalues, q.pat, q.m, X, X + sg::kPatWords, nullptr);
        a->x0 = X[0];
        a->x1 = X[sg::kPatWords];
        return SMARTGPU_OK;
    }
    static bool batch_encode(const smartgpu_ptext* t, const uint8_t* P, uint32_t m, uint32_t* X)  // true: every byte is one the text holds
    {
        return sg::encode_pattern(t->values, t->nvalues, P, m, X, X + sg::kPatWords, nullptr) == 0;
    }
    static Args batch_args(const DeviceCtx* d, const smartgpu_ptext* text, const uint32_t* host_pat, uint32_t k, uint32_t m, uint64_t off, uint64_t n)
    {
        Args a;
        plane_head(a, d, text, m, off, n, k);
        a.x0 = host_pat[kWords * k];
        a.x1 = host_pat[kWords * k + sg::kPatWords];
        a.pat += kWords * k;
        return a;
    }
};

struct Sets : Exact {  // (the two-plane kinds: Exact's unit, each its own arguments, planes and kernel pair)
    using Args = sg::PlaneSetArgs;
    static constexpr size_t kWords = sg::kSetWords;
    static constexpr const char* kKernel[2] = {"planes_sets_scan", "planes_sets_find"};
    static auto scan() { return sg::launch_planes_sets_scan; }
    static auto find() { return sg::launch_planes_sets_find; }
    static int encode(const PQuestion& q, uint32_t* Y, Args* a, uint32_t* none, bool* full)
    {
        const int rc = sets_planes(q.text, q.pat, q.m, false, Y, none, full);
        if (rc == SMARTGPU_OK) set_words(*a, Y);
        return rc;
    }
};

struct Mis : Exact {
    using Args = sg::PlaneMisArgs;
    static constexpr size_t kWords = 3 * sg::kPatWords;  // a pattern's two code planes and its skip plane
    static constexpr const char* kKernel[2] = {"planes_mis_scan", "planes_mis_find"};
    static auto scan() { return sg::launch_planes_mis_scan; }
    static auto find() { return sg::launch_planes_mis_find; }
    static int encode(const PQuestion& q, uint32_t* X, Args* a, uint32_t* none, bool*)
    {
        *none = a->foreign = sg::encode_pattern(q.text->values, q.text->nvalues, q.pat, q.m, X, X + sg::kPatWords, X + 2 * sg::kPatWords);
        a->budget = *none > q.k ? 0 : q.k - *none;
        a->x0 = X[0];
        a->x1 = X[sg::kPatWords];
        a->skip = X[2 * sg::kPatWords];
        return SMARTGPU_OK;
    }
};

struct SetsMis : Exact {
    using Args = sg::PlaneSetMisArgs;
    static constexpr size_t kWords = sg::kSetWords;
    static constexpr const char* kKernel[2] = {"planes_sets_mis_scan", "planes_sets_mis_find"};
    static auto scan() { return sg::launch_planes_sets_mis_scan; }
    static auto find() { return sg::launch_planes_sets_mis_find; }
    static int encode(const PQuestion& q, uint32_t* Y, Args* a, uint32_t* none, bool* full)
    {
        const int rc = sets_planes(q.text, q.pat, q.m, true, Y, none, full);
        a->foreign = *none;
        a->budget = *none > q.k ? 0 : q.k - *none;
        if (rc == SMARTGPU_OK) set_words(*a, Y);
        return rc;
    }
};

// Three planes: bytes, sets, with and without mismatches as eight membership planes, through planes3_scan / planes3_find,
// which need k_planes3.hip in the program.  In a batch: an exact pattern, singleton sets, budget 0.
struct Three {
    using Args = sg::Plane3Args;
    static constexpr size_t kWords = sg::kSet8Words;
    static constexpr const char* kKernel[2] = {"planes3_scan", "planes3_find"};
    static constexpr const char* kUnit = "k_planes3.hip";
    static const char* missing(bool) { return sg::g_planes3_scan && sg::g_planes3_find ? nullptr : "planes3_scan / planes3_find"; }
    static auto scan() { return sg::g_planes3_scan; }
    static auto find() { return sg::g_planes3_find; }
    static int encode(const PQuestion& q, uint32_t* Y, Args* a, uint32_t* none, bool* full)
    {
        int rc = SMARTGPU_OK;
        if (q.sets) rc = refuse_code(q.text, q.pat, sg::encode_sets8(q.text->nvalues, q.pat, q.m, true, Y, none, full));
        else *none = sg::encode_pattern8(q.text->values, q.text->nvalues, q.pat, q.m, true, Y);
        a->foreign = *none;
        a->budget = *none > q.k ? 0 : q.k - *none;
        a->shift = 0;
        if (rc == SMARTGPU_OK) set_words(*a, Y);
        return rc;
    }
    static bool batch_encode(const smartgpu_ptext* t, const uint8_t* P, uint32_t m, uint32_t* Y)
    {
        return sg::encode_pattern8(t->values, t->nvalues, P, m, false, Y) == 0;
    }
    static Args batch_args(const DeviceCtx* d, const smartgpu_ptext* text, const uint32_t* host_pat, uint32_t k, uint32_t m, uint64_t off, uint64_t n)
    {
        Args a;
        plane_head(a, d, text, m, off, n, k);
        set_words(a, host_pat + kWords * k);
        a.budget = a.foreign = a.shift = 0;
        a.pat += kWords * k;
        return a;
    }
};

// The family of the plane matchers: start positions, n - m + 1 of them; a find's entries are spans (order_spans), with
// mismatches position << kMisShift | distance.  A pattern of full sets is every start position for the set calls and is
// launched by the mismatch calls (which report distances).
template <typename K>
struct PlaneCall : PQuestion {
    typename K::Args a;
    uint32_t words[K::kWords];
    uint32_t shift;
    RunNames w;
    uint64_t bound;
    static constexpr size_t arena = sizeof(uint32_t) * K::kWords;

    Prepared prepare(bool find, const uint64_t* count)
    {
        // (the exact kind's only caller here is smartgpu_pfind64, which has made its checks, with a message of its own)
        int rc = (sets || mis) ? check_pext_args(call, sets ? "sets" : "P", pat, m, k, text, off, n, count) : SMARTGPU_OK;
        if (rc != SMARTGPU_OK) return refused(rc);
        uint32_t none = 0;
        bool full = false;
        if ((rc = K::encode(*this, words, &a, &none, &full)) != SMARTGPU_OK) return refused(rc);
        if (none > k || m > n) return answered(0);      // more positions that accept nothing than mismatches allowed, or no window fits
        if (full && !mis) return answered(n - m + 1);   // every start position of the range
        if (const char* kernel = K::missing(find)) return refused(kernel_missing(call, kernel, K::kUnit));
        shift = find && mis ? sg::kMisShift : 0u;
        if constexpr (std::is_same<K, Three>::value) a.shift = shift;
        w = {call, K::kKernel[find], "start positions", "positions"};
        bound = n - m + 1;
        return kLaunch;
    }
    bool stage(DeviceCtx* d) { return stage_pattern(d, words, arena, m); }
    hipError_t scan(DeviceCtx* d) { plane_head(a, d, text, m, off, n); return K::scan()(a, text->planes, d->num_cus, d->stream); }
    hipError_t find(DeviceCtx* d, unsigned long long* out, uint64_t room) { plane_head(a, d, text, m, off, n); return K::find()(a, out, room, text->planes, d->num_cus, d->stream); }
    bool order(uint64_t* e, uint64_t total) const { return spans_in_order(w, e, total, off, off + n - m, shift); }
    void post(uint64_t* positions, uint8_t* mismatches, uint64_t count) const { if (mis) unpack_mis(positions, mismatches, count); }
};

// A plane call by the text it is asked of: kind Two on one or two planes, Three on three (a NULL text: Two's checks refuse it)
template <typename Two>
int plane_count(const PQuestion& q, uint64_t* count, double* pre_ms, double* run_ms)
{
    if (q.text && q.text->planes == 3) return run_count<PlaneCall<Three>>(q, count, pre_ms, run_ms);
    return run_count<PlaneCall<Two>>(q, count, pre_ms, run_ms);
}

template <typename Two>
int plane_find(const PQuestion& q, uint64_t* positions, uint8_t* mismatches, uint64_t cap, uint64_t* count)
{
    if (q.text && q.text->planes == 3) return run_find<PlaneCall<Three>>(q, "positions", positions, mismatches, cap, count);
    return run_find<PlaneCall<Two>>(q, "positions", positions, mismatches, cap, count);
}

// ---- the batch calls.  K patterns of m symbols: their planes to the device's arena (m > 32 only: shorter patterns travel as
// kernel arguments), K launches back to back on the device's stream, ONE read-back.  A pattern with a byte the text does
// not hold: no launch.  Enc is Exact or Three (on three planes K <= kBatch3Max: checked by the callers before any HIP call). ----
template <typename Enc>
int psearch_impl(const uint8_t* const* P, uint32_t m, uint32_t K, const smartgpu_ptext* text, uint64_t off, uint64_t n, uint64_t* counts,
                 double* pre_ms, double* run_ms)
{
    if (const char* kernel = Enc::missing(false)) return kernel_missing("psearch64", kernel, Enc::kUnit);
    DeviceCtx* d = device_ctx_flushed(text->device);
    if (!d) return SMARTGPU_ERR_HIP;
    const double t_pre = now_ms();
    constexpr size_t kPatBytes = 4 * Enc::kWords;
    if (static_cast<size_t>(K) * kPatBytes > d->pinned_bytes) { set_error("psearch_batch: %u patterns exceed the staging buffer", K); return SMARTGPU_ERR_ARG; }
    if (!batch_reserve(d, static_cast<size_t>(K) * kPatBytes, K)) return SMARTGPU_ERR_NOMEM;
    // (the staging buffer is free: every call that fills it ends with a synchronisation of the device's stream)
    uint32_t* host_pat = reinterpret_cast<uint32_t*>(d->pinned);
    std::vector<uint8_t> present(K, 0);
    for (uint32_t k = 0; k < K; ++k) {
        if (!P[k]) { set_error("pattern %u is NULL", k); return SMARTGPU_ERR_ARG; }
        present[k] = Enc::batch_encode(text, P[k], m, host_pat + Enc::kWords * k);
    }
    const bool fits = n >= m;  // m > n: no window fits, count 0
    if (m > 32 && fits)
        HIP_TRY(hipMemcpyAsync(d->arena, host_pat, static_cast<size_t>(K) * kPatBytes, hipMemcpyHostToDevice, d->stream), return SMARTGPU_ERR_HIP);
    if (pre_ms) *pre_ms = now_ms() - t_pre;
    const double t0 = now_ms();
    HIP_TRY(hipMemsetAsync(d->batch_counts, 0, static_cast<size_t>(K) * 8, d->stream), return SMARTGPU_ERR_HIP);
    for (uint32_t k = 0; k < K && fits; ++k) {
        if (!present[k]) continue;
        const typename Enc::Args a = Enc::batch_args(d, text, host_pat, k, m, off, n);
        HIP_TRY(Enc::scan()(a, text->planes, d->num_cus, d->stream), return SMARTGPU_ERR_HIP);
    }
    HIP_TRY(hipMemcpyAsync(d->pinned_counts, d->batch_counts, static_cast<size_t>(K) * 8, hipMemcpyDeviceToHost, d->stream), return SMARTGPU_ERR_HIP);
    HIP_TRY(hipStreamSynchronize(d->stream), return SMARTGPU_ERR_HIP);
    if (run_ms) *run_ms = now_ms() - t0;
    for (uint32_t k = 0; k < K; ++k) {
        // more occurrences than start positions: refused like a poisoned count, never reported
        if (d->pinned_counts[k] > (fits ? n - m + 1 : 0)) { set_error("%s: count %llu exceeds the %llu start positions", Enc::kKernel[0], (unsigned long long)d->pinned_counts[k], (unsigned long long)(fits ? n - m + 1 : 0)); return SMARTGPU_ERR_HIP; }
        counts[k] = d->pinned_counts[k];
    }
    return SMARTGPU_OK;
}

// psearch_impl by the text's planes, for the two count calls
int psearch_any(const uint8_t* const* P, uint32_t m, uint32_t K, const smartgpu_ptext* text, uint64_t off, uint64_t n, uint64_t* counts,
                double* pre_ms, double* run_ms)
{
    return text->planes == 3 ? psearch_impl<Three>(P, m, K, text, off, n, counts, pre_ms, run_ms) : psearch_impl<Exact>(P, m, K, text, off, n, counts, pre_ms, run_ms);
}

// The batch calls' bound on a three-plane text (planes3.hpp: kBatch3Max), decided before any HIP call.
int check_batch3(const char* call, const smartgpu_ptext* text, uint32_t K)
{
    if (text->planes != 3 || K <= sg::kBatch3Max) return SMARTGPU_OK;
    set_error("%s: %u patterns on a three-plane text, at most %u per call (eight membership planes per pattern in the staging buffer)", call, K, sg::kBatch3Max);
    return SMARTGPU_ERR_ARG;
}

// smartgpu_pfind_batch64 behind its checks: two passes over K cursors
template <typename Enc>
int pfind_batch_impl(const uint8_t* const* P, uint32_t m, uint32_t K, const smartgpu_ptext* text, uint64_t off, uint64_t n, uint64_t* positions,
                     uint64_t cap, uint64_t* starts)
{
    // pass 1: the K counts (the planes are read twice: a one-pass ordered batch is not built)
    std::vector<uint64_t> counts(K);
    const int r1 = psearch_impl<Enc>(P, m, K, text, off, n, counts.data(), nullptr, nullptr);
    if (r1 != SMARTGPU_OK) return r1;
    starts[0] = 0;
    for (uint32_t k = 0; k < K; ++k) starts[k + 1] = starts[k] + counts[k];
    const uint64_t total = starts[K];
    if (total > cap) { set_error("pfind_batch: %llu occurrences, room for %llu", (unsigned long long)total, (unsigned long long)cap); return SMARTGPU_ERR_NOMEM; }
    if (total == 0) return SMARTGPU_OK;
    // pass 2: a find for every pattern that occurs, each with its own cursor and its own slice as base and cap.  The
    // patterns' planes are where psearch_impl left them: the staging buffer and, for m > 32, the arena.
    DeviceCtx* d = device_ctx_flushed(text->device);
    if (!d) return SMARTGPU_ERR_HIP;
    const uint32_t* host_pat = reinterpret_cast<const uint32_t*>(d->pinned);
    bool own = false;
    unsigned long long* out = find_reserve(d, total, &own);
    if (!out) return SMARTGPU_ERR_NOMEM;
    bool ok = hipMemsetAsync(d->batch_counts, 0, static_cast<size_t>(K) * 8, d->stream) == hipSuccess;
    for (uint32_t k = 0; k < K && ok; ++k) {
        if (counts[k] == 0) continue;
        const typename Enc::Args a = Enc::batch_args(d, text, host_pat, k, m, off, n);
        ok = Enc::find()(a, out + starts[k], counts[k], text->planes, d->num_cus, d->stream) == hipSuccess;
    }
    ok = ok && hipMemcpyAsync(d->pinned_counts, d->batch_counts, static_cast<size_t>(K) * 8, hipMemcpyDeviceToHost, d->stream) == hipSuccess &&
         hipStreamSynchronize(d->stream) == hipSuccess && copy_positions(d, positions, out, total);
    int r = SMARTGPU_OK;
    if (!ok) {
        set_error("pfind_batch: %s", hipGetErrorString(hipGetLastError()));
        r = SMARTGPU_ERR_HIP;
    }
    for (uint32_t k = 0; k < K && r == SMARTGPU_OK; ++k) {
        if (d->pinned_counts[k] != counts[k]) {  // the two passes disagree: refused, never reported
            set_error("planes_find: pattern %u: cursor %llu, planes_scan counted %llu", k, d->pinned_counts[k], (unsigned long long)counts[k]);
            r = SMARTGPU_ERR_HIP;
        } else if (!sg::order_spans(positions + starts[k], counts[k], off, off + n - m)) {
            set_error("planes_find: pattern %u: the positions are not ascending spans of %llu start positions", k, (unsigned long long)sg::kFindSpan);
            r = SMARTGPU_ERR_HIP;
        }
    }
    if (own) (void)hipFree(out);
    return r;
}

// ---- edit distance on a packed text (pedit.hpp, peditl.hpp).  These families, and the edit families on byte texts below,
// count and list END positions, n of them whatever m is, and m > n is legal; their entries are end << shift | distance.
// They stage no planes: the masks are kernel arguments here, and a table in the arena on byte texts. ----

// What tells the two families apart.  Short (pedit.hpp): m <= 64, k <= 7, entries in spans.  Long (peditl.hpp): m <= 256,
// k <= 31, a switch that travels with the call, and entries that the kernel writes in no order (order_editl sorts them).
struct PEdit {
    using Args = sg::PlaneEditArgs;
    static constexpr uint32_t kMaxM = SMARTGPU_PEDIT_MAXM, kMaxK = SMARTGPU_PMIS_MAX, kShift = sg::kMisShift;
    static constexpr bool kLong = false;
    static constexpr const char* kKernel[2] = {"planes_edit_scan", "planes_edit_find"};
    static constexpr const char* kUnit = "k_pedit.hip";
    static auto scan() { return sg::g_planes_edit_scan; }
    static auto find() { return sg::g_planes_edit_find; }
};

struct PEditl {
    using Args = sg::PlaneEditlArgs;
    static constexpr uint32_t kMaxM = SMARTGPU_PEDITL_MAXM, kMaxK = SMARTGPU_PEDITL_MAXK, kShift = sg::kEditlShift;
    static constexpr bool kLong = true;
    static constexpr const char* kKernel[2] = {"planes_editl_scan", "planes_editl_find"};
    static constexpr const char* kUnit = "k_peditl.hip";
    static auto scan() { return sg::g_planes_editl_scan; }
    static auto find() { return sg::g_planes_editl_find; }
};

// find_run's `order` for the edit families: spans of end positions, or (kLong) entries in no order
template <typename F>
bool ends_in_order(const RunNames& w, uint64_t* e, uint64_t total, uint64_t off, uint64_t n, uint32_t k)
{
    if constexpr (F::kLong) return editl_in_order(w, e, total, off, off + n - 1, k, F::kShift);
    else return spans_in_order(w, e, total, off, off + n - 1, F::kShift);
}

template <typename F>
struct PEditCall : PQuestion {
    typename F::Args a;
    RunNames w;
    uint64_t bound;
    static constexpr size_t arena = 0;

    Prepared prepare(bool find, const uint64_t* count)
    {
        int rc = check_pedit_args(call, sets ? "sets" : "P", pat, m, F::kMaxM, k, F::kMaxK, flags, text, off, n, count);
        if (rc != SMARTGPU_OK) return refused(rc);
        if ((rc = edit_masks(text, pat, m, sets, &a)) != SMARTGPU_OK) return refused(rc);
        if (n + k < m) return answered(0);  // not even with k deletions: no launch
        if (const char* kernel = missing_kernel<F>(find)) return refused(kernel_missing(call, kernel, F::kUnit));
        edit_head(a, text, m, k, off, n);
        if constexpr (F::kLong) a.all_blocks = flags & SMARTGPU_PEDITL_ALL_BLOCKS;
        w = {call, F::kKernel[find], "end positions", "entries"};
        bound = n;
        return kLaunch;
    }
    bool stage(DeviceCtx*) { return true; }
    hipError_t scan(DeviceCtx* d) { a.count = d->batch_counts; return F::scan()(a, text->planes, d->num_cus, d->stream); }
    hipError_t find(DeviceCtx* d, unsigned long long* out, uint64_t room) { a.count = d->batch_counts; return F::find()(a, out, room, text->planes, d->num_cus, d->stream); }
    bool order(uint64_t* e, uint64_t total) const { return ends_in_order<F>(w, e, total, off, n, k); }
    void post(uint64_t* ends, uint8_t* distances, uint64_t count) const { unpack_mis(ends, distances, count, F::kShift); }
};

// ---- BYTE texts: edit distance (tedit.hpp, teditl.hpp) and mismatches (tmis.hpp), the contracts of the packed calls above
// with a smartgpu_text in place of the planes ----

// What tells the three families apart: the bounds, what k counts, the flag bits, the table, and what is counted — END
// positions (kStarts == false: n of them, no launch when n + k < m), or, for mismatches, START positions (n - m + 1, no
// launch when m > n; the kernel's entries hold the windows' ENDS, the spans order_spans knows, and a window's start is
// m - 1 below its end).  kLong: the switch, and entries in no order.
struct TEdit {
    using Args = sg::TextEditArgs;
    static constexpr int kMaxM = SMARTGPU_EDIT_MAXM, kMaxK = SMARTGPU_PMIS_MAX;
    static constexpr uint32_t kFlags = 0, kShift = sg::kMisShift;
    static constexpr bool kLong = false, kStarts = false;
    static constexpr const char* kNoun = "edits";
    static constexpr const char* kKernel[2] = {"text_edit_scan", "text_edit_find"};
    static constexpr const char* kUnit = "k_tedit.hip";
    static constexpr size_t kArena = kTEditArena;
    static auto scan() { return sg::g_text_edit_scan; }
    static auto find() { return sg::g_text_edit_find; }
    static bool stage(DeviceCtx* d, const TQuestion& q, Args& a) { return tedit_stage(d, q.pat, q.sets, q.m, &a.peq); }
};

struct TEditl {
    using Args = sg::TextEditlArgs;
    static constexpr int kMaxM = SMARTGPU_EDITL_MAXM, kMaxK = SMARTGPU_EDITL_MAXK;
    static constexpr uint32_t kFlags = SMARTGPU_EDITL_ALL_BLOCKS, kShift = sg::kTEditlShift;
    static constexpr bool kLong = true, kStarts = false;
    static constexpr const char* kNoun = "edits";
    static constexpr const char* kKernel[2] = {"text_editl_scan", "text_editl_find"};
    static constexpr const char* kUnit = "k_teditl.hip";
    static constexpr size_t kArena = kTEditlArena;
    static auto scan() { return sg::g_text_editl_scan; }
    static auto find() { return sg::g_text_editl_find; }
    static bool stage(DeviceCtx* d, const TQuestion& q, Args& a) { return teditl_stage(d, q.pat, q.sets, q.m, &a.peq); }
};

struct TMis {
    using Args = sg::TextMisArgs;
    static constexpr int kMaxM = SMARTGPU_MIS_MAXM, kMaxK = SMARTGPU_PMIS_MAX;
    static constexpr uint32_t kFlags = 0, kShift = sg::kMisShift;
    static constexpr bool kLong = false, kStarts = true;
    static constexpr const char* kNoun = "mismatches";
    static constexpr const char* kKernel[2] = {"text_mis_scan", "text_mis_find"};
    static constexpr const char* kUnit = "k_tmis.hip";
    static constexpr size_t kArena = TEdit::kArena;
    static auto scan() { return sg::g_text_mis_scan; }
    static auto find() { return sg::g_text_mis_find; }
    static bool stage(DeviceCtx* d, const TQuestion& q, Args& a)  // tmis_host.hpp's masks "position j does NOT accept this byte": tedit_stage's table and arena (call_host.hpp)
    {
        uint32_t neq[256][sg::kTEditWords];
        if (q.sets) sg::mis_neq_classes(q.pat, q.m, neq); else sg::mis_neq_bytes(q.pat, q.m, neq);
        return text_table_stage(d, neq, static_cast<uint32_t>(sg::mis_words(q.m)), &a.neq);
    }
};

template <typename F>
struct TextCall : TQuestion {
    typename F::Args a;
    RunNames w;
    uint64_t bound;
    static constexpr size_t arena = F::kArena;

    Prepared prepare(bool find, const uint64_t* count)
    {
        const int rc = check_text_args(call, sets ? "classes" : "P", F::kMaxM, F::kMaxK, F::kNoun, F::kFlags, pat, m, k, flags, text, off, n, count);
        if (rc != SMARTGPU_OK) return refused(rc);
        if (F::kStarts ? m > n : n + k < m) return answered(0);  // no window fits / not even with k deletions: no launch
        if (const char* kernel = missing_kernel<F>(find)) return refused(kernel_missing(call, kernel, F::kUnit));
        text_head(a, text, m, k, off, n);
        if constexpr (F::kLong) a.all_blocks = flags & F::kFlags;
        w = {call, F::kKernel[find], F::kStarts ? "start positions" : "end positions", F::kStarts ? "positions" : "entries"};
        bound = F::kStarts ? n - m + 1 : n;
        return kLaunch;
    }
    bool stage(DeviceCtx* d) { return F::stage(d, *this, a); }
    hipError_t scan(DeviceCtx* d) { a.count = d->batch_counts; return F::scan()(a, d->num_cus, d->stream); }
    hipError_t find(DeviceCtx* d, unsigned long long* out, uint64_t room) { a.count = d->batch_counts; return F::find()(a, out, room, d->num_cus, d->stream); }
    bool order(uint64_t* e, uint64_t total) const { return ends_in_order<F>(w, e, total, off, n, k); }
    void post(uint64_t* entries, uint8_t* distances, uint64_t count) const
    {
        unpack_mis(entries, distances, count, F::kShift);
        if (F::kStarts)
            for (uint64_t i = 0; i < count; ++i) entries[i] -= m - 1;
    }
};

}  // namespace

extern "C" {

int smartgpu_ptext_layout(uint64_t n, int nvalues, int* planes, uint64_t* plane_bytes)
{
    if (nvalues < 1 || nvalues > 4) { set_error("a packed text holds 1 to 4 distinct byte values, not %d", nvalues); return SMARTGPU_ERR_ARG; }
    if (planes) *planes = nvalues <= 2 ? 1 : 2;
    if (plane_bytes) *plane_bytes = sg::plane_bytes(n);
    return SMARTGPU_OK;
}

int smartgpu_ptext_layout8(uint64_t n, int nvalues, int* planes, uint64_t* plane_bytes)
{
    if (nvalues < 1 || nvalues > SMARTGPU_PTEXT_MAXVALUES) { set_error("a packed text of the ...8 constructors holds 1 to %d distinct byte values, not %d", SMARTGPU_PTEXT_MAXVALUES, nvalues); return SMARTGPU_ERR_ARG; }
    if (planes) *planes = nvalues <= 2 ? 1 : nvalues <= 4 ? 2 : 3;
    if (plane_bytes) *plane_bytes = sg::plane_bytes(n);
    return SMARTGPU_OK;
}

// smartgpu_ptext_pack (most = 4) and smartgpu_ptext_pack8 (most = 8): at most four values give one or two planes through
// planes_pack either way, five to eight three planes through planes3_pack.
static smartgpu_ptext* ptext_pack_impl(const smartgpu_text* t, int most)
{
    if (!t) { set_error("text handle is NULL"); return nullptr; }
    uint8_t values[8] = {255, 255, 255, 255, 255, 255, 255, 255};
    int k = 0;
    for (int c = 0; c < 256; ++c)
        if (t->alphabet[c >> 5] >> (c & 31) & 1u) {
            if (k < 8) values[k] = static_cast<uint8_t>(c);
            ++k;
        }
    if (k > most) { set_error("the text holds %d distinct byte values: a packed text holds at most %d", k, most); return nullptr; }
    if (k > 4 && !sg::g_planes3_pack) { (void)kernel_missing("ptext_pack8", "planes3_pack", "k_planes3.hip"); return nullptr; }
    DeviceCtx* d = device_ctx_flushed(t->device);
    if (!d) return nullptr;
    smartgpu_ptext* p = new smartgpu_ptext;
    p->device = t->device;
    p->n = t->n;
    p->planes = k <= 2 ? 1 : k <= 4 ? 2 : 3;
    p->nvalues = k;
    for (int i = 0; i < k; ++i) p->values[i] = values[i];
    if (hipMalloc(reinterpret_cast<void**>(&p->base), p->alloc_bytes()) != hipSuccess) {
        set_error("hipMalloc of %llu bytes failed", (unsigned long long)p->alloc_bytes());
        delete p;
        return nullptr;
    }
    // code = number of these below the byte (255: none is)
    hipError_t e = hipMemsetAsync(p->base, 0, p->alloc_bytes(), d->stream);  // pads and tail bits are zero
    if (e == hipSuccess)
        e = p->planes == 3 ? sg::g_planes3_pack(t->data(), t->n, p->plane(0), p->plane(1), p->plane(2), values, d->stream)
                           : sg::launch_planes_pack(t->data(), t->n, p->plane(0), p->plane(p->planes - 1), p->planes, values, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) {
        set_error("%s failed: %s", p->planes == 3 ? "planes3_pack" : "planes_pack", hipGetErrorString(e));
        smartgpu_ptext_free(p);
        return nullptr;
    }
    return p;
}

smartgpu_ptext* smartgpu_ptext_pack(const smartgpu_text* t) { return ptext_pack_impl(t, 4); }
smartgpu_ptext* smartgpu_ptext_pack8(const smartgpu_text* t) { return ptext_pack_impl(t, SMARTGPU_PTEXT_MAXVALUES); }

smartgpu_ptext* smartgpu_ptext_upload(const void* host, uint64_t n, int device)
{
    smartgpu_text* t = smartgpu_text_upload(host, n, device);
    if (!t) return nullptr;
    smartgpu_ptext* p = smartgpu_ptext_pack(t);
    smartgpu_text_free(t);
    return p;
}

smartgpu_ptext* smartgpu_ptext_upload8(const void* host, uint64_t n, int device)
{
    smartgpu_text* t = smartgpu_text_upload(host, n, device);
    if (!t) return nullptr;
    smartgpu_ptext* p = smartgpu_ptext_pack8(t);
    smartgpu_text_free(t);
    return p;
}

void smartgpu_ptext_free(smartgpu_ptext* t)
{
    if (!t) return;
    if (t->base) {
        hipSetDevice(t->device);
        hipFree(t->base);
    }
    delete t;
}

uint64_t smartgpu_ptext_length(const smartgpu_ptext* t) { return t ? t->n : 0; }
int smartgpu_ptext_device(const smartgpu_ptext* t) { return t ? t->device : -1; }
int smartgpu_ptext_planes(const smartgpu_ptext* t) { return t ? t->planes : 0; }
uint64_t smartgpu_ptext_bytes(const smartgpu_ptext* t) { return t ? static_cast<uint64_t>(t->planes) * sg::plane_bytes(t->n) : 0; }

int smartgpu_ptext_symbols(const smartgpu_ptext* t, uint8_t values[4])
{
    if (!t || !values) { set_error("bad ptext_symbols arguments"); return SMARTGPU_ERR_ARG; }
    if (t->planes == 3) { set_error("ptext_symbols: a three-plane text holds %d values, more than the four entries of this call: use smartgpu_ptext_symbols8", t->nvalues); return SMARTGPU_ERR_ARG; }
    std::memcpy(values, t->values, 4);
    return t->nvalues;
}

int smartgpu_ptext_symbols8(const smartgpu_ptext* t, uint8_t values[8])
{
    if (!t || !values) { set_error("bad ptext_symbols8 arguments"); return SMARTGPU_ERR_ARG; }
    std::memcpy(values, t->values, 8);
    return t->nvalues;
}

int smartgpu_ptext_read(const smartgpu_ptext* t, uint64_t off, uint64_t len, void* host)
{
    if (!t || (!host && len) || off > t->n || len > t->n - off) { set_error("bad ptext_read range"); return SMARTGPU_ERR_ARG; }
    if (len == 0) return SMARTGPU_OK;
    DeviceCtx* d = device_ctx_flushed(t->device);
    if (!d) return SMARTGPU_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(d->stream), return SMARTGPU_ERR_HIP);
    const uint64_t w0 = off / 32, nw = (off + len + 31) / 32 - w0;
    std::vector<uint32_t> w[3];
    for (int b = 0; b < t->planes; ++b) {
        w[b].resize(nw);
        HIP_TRY(hipMemcpy(w[b].data(), t->plane(b) + w0, nw * 4, hipMemcpyDeviceToHost), return SMARTGPU_ERR_HIP);
    }
    uint8_t* out = static_cast<uint8_t*>(host);
    for (uint64_t i = 0; i < len; ++i) {
        const uint64_t s = off + i - 32 * w0;
        uint32_t code = w[0][s >> 5] >> (s & 31) & 1u;
        if (t->planes >= 2) code |= (w[1][s >> 5] >> (s & 31) & 1u) << 1;
        if (t->planes == 3) code |= (w[2][s >> 5] >> (s & 31) & 1u) << 2;
        out[i] = t->values[code];
    }
    return SMARTGPU_OK;
}

int smartgpu_ptext_probe_read_ms(const smartgpu_ptext* t, int reps, double* ms_per_pass)
{
    if (!t || reps < 1 || !ms_per_pass) { set_error("bad probe arguments"); return SMARTGPU_ERR_ARG; }
    DeviceCtx* d = device_ctx_flushed(t->device);
    if (!d) return SMARTGPU_ERR_HIP;
    // the planes and the pad between them: one contiguous region of the allocation
    const uint8_t* first = reinterpret_cast<const uint8_t*>(t->plane(0));
    const uint64_t bytes = static_cast<uint64_t>(t->planes - 1) * sg::plane_stride(t->n) + sg::plane_bytes(t->n);
    if (!batch_reserve(d, 0, 1)) return SMARTGPU_ERR_NOMEM;
    // (the sink: probe_read adds to it practically never; every search zeroes its slots first)
    return probe_read_ms(d, first, bytes, d->batch_counts, reps, ms_per_pass);
}

/* ---- exact occurrences: the count goes through the batch path with a set of one -------------------------------------- */
int smartgpu_psearch64(const uint8_t* P, uint32_t m, const smartgpu_ptext* text, uint64_t off, uint64_t n, uint64_t* count,
                       double* pre_ms, double* run_ms)
{
    const int rc = check_psearch_args(P, m, text, off, n);
    if (rc != SMARTGPU_OK) return rc;
    const uint8_t* set[1] = {P};
    uint64_t c = 0;
    double pre = 0.0, run = 0.0;
    const int r = psearch_any(set, m, 1, text, off, n, &c, &pre, &run);
    if (r != SMARTGPU_OK) return r;
    return pcount_done(c, pre, run, count, pre_ms, run_ms);
}

int smartgpu_psearch_batch64(const uint8_t* const* P, uint32_t m, uint32_t K, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                             uint64_t* counts, double* batch_ms)
{
    if (!P || K < 1 || !counts) { set_error("psearch_batch: P/counts NULL or K = 0"); return SMARTGPU_ERR_ARG; }
    int rc = check_psearch_args(P[0], m, text, off, n);
    if (rc != SMARTGPU_OK) return rc;
    if ((rc = check_batch3("psearch_batch", text, K)) != SMARTGPU_OK) return rc;
    double pre = 0.0, run = 0.0;
    const int r = psearch_any(P, m, K, text, off, n, counts, &pre, &run);
    if (r != SMARTGPU_OK) return r;
    if (batch_ms) *batch_ms = run;
    return pcount_done(0, pre / K, run / K, nullptr, nullptr, nullptr);  // the times per pattern, for smartgpu_last_times alone
}

/* ---- occurrence positions on a packed text (planes_find) ---------------------------------------------------------- */
int smartgpu_pfind64(const uint8_t* P, uint32_t m, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                     uint64_t* positions, uint64_t cap, uint64_t* count)
{
    const int rc = check_psearch_args(P, m, text, off, n);
    if (rc != SMARTGPU_OK) return rc;
    if (!count || (cap && !positions)) { set_error("pfind64: count must not be NULL, positions only with cap = 0"); return SMARTGPU_ERR_ARG; }
    // (a byte the text does not hold, or no window fits: no launch)
    return plane_find<Exact>({"pfind64", P, false, false, m, 0, 0, text, off, n}, positions, nullptr, cap, count);
}

int smartgpu_pfind_batch64(const uint8_t* const* P, uint32_t m, uint32_t K, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                           uint64_t* positions, uint64_t cap, uint64_t* starts)
{
    if (!P || K < 1 || !starts) { set_error("pfind_batch: P/starts NULL or K = 0"); return SMARTGPU_ERR_ARG; }
    int rc = check_psearch_args(P[0], m, text, off, n);
    if (rc != SMARTGPU_OK) return rc;
    if ((rc = check_room("pfind_batch", "positions", positions, cap)) != SMARTGPU_OK) return rc;
    if ((rc = check_batch3("pfind_batch", text, K)) != SMARTGPU_OK) return rc;
    return text->planes == 3 ? pfind_batch_impl<Three>(P, m, K, text, off, n, positions, cap, starts)
                             : pfind_batch_impl<Exact>(P, m, K, text, off, n, positions, cap, starts);
}

/* ---- set patterns: every pattern position accepts a set of the text's values ---------------------------------------- */
int smartgpu_psearch_sets64(const uint8_t* sets, uint32_t m, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                            uint64_t* count, double* pre_ms, double* run_ms)
{
    return plane_count<Sets>({"psearch_sets64", sets, true, false, m, 0, 0, text, off, n}, count, pre_ms, run_ms);
}

int smartgpu_pfind_sets64(const uint8_t* sets, uint32_t m, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                          uint64_t* positions, uint64_t cap, uint64_t* count)
{
    return plane_find<Sets>({"pfind_sets64", sets, true, false, m, 0, 0, text, off, n}, positions, nullptr, cap, count);
}

/* ---- mismatches: occurrences within Hamming distance k ---------------------------------------------------------------- */
int smartgpu_psearch_mis64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                           uint64_t* count, double* pre_ms, double* run_ms)
{
    return plane_count<Mis>({"psearch_mis64", P, false, true, m, k, 0, text, off, n}, count, pre_ms, run_ms);
}

int smartgpu_pfind_mis64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                         uint64_t* positions, uint8_t* mismatches, uint64_t cap, uint64_t* count)
{
    return plane_find<Mis>({"pfind_mis64", P, false, true, m, k, 0, text, off, n}, positions, mismatches, cap, count);
}

/* ---- set patterns with mismatches: at most k positions whose symbol is no member of the position's set ---------------- */
int smartgpu_psearch_sets_mis64(const uint8_t* sets, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                                uint64_t* count, double* pre_ms, double* run_ms)
{
    return plane_count<SetsMis>({"psearch_sets_mis64", sets, true, true, m, k, 0, text, off, n}, count, pre_ms, run_ms);
}

int smartgpu_pfind_sets_mis64(const uint8_t* sets, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                              uint64_t* positions, uint8_t* mismatches, uint64_t cap, uint64_t* count)
{
    return plane_find<SetsMis>({"pfind_sets_mis64", sets, true, true, m, k, 0, text, off, n}, positions, mismatches, cap, count);
}

/* ---- edit distance: end positions within k substitutions, insertions and deletions (pedit.hpp, k_pedit.hip) ------------ */
int smartgpu_psearch_edit64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                            uint64_t* count, double* pre_ms, double* run_ms)
{
    return run_count<PEditCall<PEdit>>(PQuestion{"psearch_edit64", P, false, false, m, k, 0, text, off, n}, count, pre_ms, run_ms);
}

int smartgpu_pfind_edit64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                          uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return run_find<PEditCall<PEdit>>(PQuestion{"pfind_edit64", P, false, false, m, k, 0, text, off, n}, "ends", ends, distances, cap, count);
}

int smartgpu_psearch_sets_edit64(const uint8_t* sets, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                                 uint64_t* count, double* pre_ms, double* run_ms)
{
    return run_count<PEditCall<PEdit>>(PQuestion{"psearch_sets_edit64", sets, true, false, m, k, 0, text, off, n}, count, pre_ms, run_ms);
}

int smartgpu_pfind_sets_edit64(const uint8_t* sets, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                               uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return run_find<PEditCall<PEdit>>(PQuestion{"pfind_sets_edit64", sets, true, false, m, k, 0, text, off, n}, "ends", ends, distances, cap, count);
}

/* ---- edit distance on byte texts: the same question of a smartgpu_text (tedit.hpp, k_tedit.hip) ------------------------- */
int smartgpu_search_edit64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                           uint64_t* count, double* pre_ms, double* run_ms)
{
    return run_count<TextCall<TEdit>>(TQuestion{"search_edit64", P, false, false, m, k, 0, text, off, n}, count, pre_ms, run_ms);
}

int smartgpu_find_edit64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                         uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return run_find<TextCall<TEdit>>(TQuestion{"find_edit64", P, false, false, m, k, 0, text, off, n}, "ends", ends, distances, cap, count);
}

int smartgpu_search_edit_classes64(const uint8_t* classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                                   uint64_t* count, double* pre_ms, double* run_ms)
{
    return run_count<TextCall<TEdit>>(TQuestion{"search_edit_classes64", classes, true, false, m, k, 0, text, off, n}, count, pre_ms, run_ms);
}

int smartgpu_find_edit_classes64(const uint8_t* classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                                 uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return run_find<TextCall<TEdit>>(TQuestion{"find_edit_classes64", classes, true, false, m, k, 0, text, off, n}, "ends", ends, distances, cap, count);
}

/* ---- edit distance on byte texts, long patterns: m <= 256, k <= 31 (teditl.hpp, k_teditl.hip) --------------------------- */
int smartgpu_search_editl64(const uint8_t* P, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_text* text, uint64_t off, uint64_t n,
                            uint64_t* count, double* pre_ms, double* run_ms)
{
    return run_count<TextCall<TEditl>>(TQuestion{"search_editl64", P, false, false, m, k, flags, text, off, n}, count, pre_ms, run_ms);
}

int smartgpu_find_editl64(const uint8_t* P, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_text* text, uint64_t off, uint64_t n,
                          uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return run_find<TextCall<TEditl>>(TQuestion{"find_editl64", P, false, false, m, k, flags, text, off, n}, "ends", ends, distances, cap, count);
}

int smartgpu_search_editl_classes64(const uint8_t* classes, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_text* text, uint64_t off,
                                    uint64_t n, uint64_t* count, double* pre_ms, double* run_ms)
{
    return run_count<TextCall<TEditl>>(TQuestion{"search_editl_classes64", classes, true, false, m, k, flags, text, off, n}, count, pre_ms, run_ms);
}

int smartgpu_find_editl_classes64(const uint8_t* classes, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_text* text, uint64_t off,
                                  uint64_t n, uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return run_find<TextCall<TEditl>>(TQuestion{"find_editl_classes64", classes, true, false, m, k, flags, text, off, n}, "ends", ends, distances, cap, count);
}

/* ---- mismatches on byte texts: smartgpu_psearch_mis64's question of a smartgpu_text (tmis.hpp, k_tmis.hip) --------------- */
int smartgpu_search_mis64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                          uint64_t* count, double* pre_ms, double* run_ms)
{
    return run_count<TextCall<TMis>>(TQuestion{"search_mis64", P, false, false, m, k, 0, text, off, n}, count, pre_ms, run_ms);
}

int smartgpu_find_mis64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                        uint64_t* positions, uint8_t* mismatches, uint64_t cap, uint64_t* count)
{
    return run_find<TextCall<TMis>>(TQuestion{"find_mis64", P, false, false, m, k, 0, text, off, n}, "positions", positions, mismatches, cap, count);
}

int smartgpu_search_mis_classes64(const uint8_t* classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                                  uint64_t* count, double* pre_ms, double* run_ms)
{
    return run_count<TextCall<TMis>>(TQuestion{"search_mis_classes64", classes, true, false, m, k, 0, text, off, n}, count, pre_ms, run_ms);
}

int smartgpu_find_mis_classes64(const uint8_t* classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                                uint64_t* positions, uint8_t* mismatches, uint64_t cap, uint64_t* count)
{
    return run_find<TextCall<TMis>>(TQuestion{"find_mis_classes64", classes, true, false, m, k, 0, text, off, n}, "positions", positions, mismatches, cap, count);
}

/* ---- edit distance, long patterns: m <= 256, k <= 31 (peditl.hpp, k_peditl.hip) ---------------------------------------- */
int smartgpu_psearch_editl64(const uint8_t* P, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                             uint64_t* count, double* pre_ms, double* run_ms)
{
    return run_count<PEditCall<PEditl>>(PQuestion{"psearch_editl64", P, false, false, m, k, flags, text, off, n}, count, pre_ms, run_ms);
}

int smartgpu_pfind_editl64(const uint8_t* P, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                           uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return run_find<PEditCall<PEditl>>(PQuestion{"pfind_editl64", P, false, false, m, k, flags, text, off, n}, "ends", ends, distances, cap, count);
}

int smartgpu_psearch_sets_editl64(const uint8_t* sets, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                                  uint64_t* count, double* pre_ms, double* run_ms)
{
    return run_count<PEditCall<PEditl>>(PQuestion{"psearch_sets_editl64", sets, true, false, m, k, flags, text, off, n}, count, pre_ms, run_ms);
}

int smartgpu_pfind_sets_editl64(const uint8_t* sets, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                                uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return run_find<PEditCall<PEditl>>(PQuestion{"pfind_sets_editl64", sets, true, false, m, k, flags, text, off, n}, "ends", ends, distances, cap, count);
}

// smartgpu_iupac_sets (most = 4) and smartgpu_iupac_sets8 (most = 8): one set of rules
static int iupac_sets_impl(const char* call, int most, const uint8_t* values, int nvalues, const char* P, uint32_t m, uint8_t* sets)
{
    if (!values || (m && (!P || !sets))) { set_error("%s: NULL argument", call); return SMARTGPU_ERR_ARG; }
    if (nvalues < 1 || nvalues > most) { set_error("%s: a packed text holds 1 to %d distinct byte values, not %d", call, most, nvalues); return SMARTGPU_ERR_ARG; }
    // the bases a letter accepts, bit 0..3 = A C G T
    static const struct { char letter; uint8_t bases; } kIupac[] = {
        {'A', 1}, {'C', 2}, {'G', 4}, {'T', 8}, {'U', 8}, {'R', 1 | 4}, {'Y', 2 | 8}, {'S', 2 | 4}, {'W', 1 | 8}, {'K', 4 | 8}, {'M', 1 | 2},
        {'B', 2 | 4 | 8}, {'D', 1 | 4 | 8}, {'H', 1 | 2 | 8}, {'V', 1 | 2 | 4}, {'N', 15}};
    int bases_of[256];
    for (int c = 0; c < 256; ++c) bases_of[c] = -1;
    for (const auto& e : kIupac) bases_of[(uint8_t)e.letter] = bases_of[(uint8_t)(e.letter | 0x20)] = e.bases;
    uint8_t base_of_code[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the base (one bit) value v stands for; 0: none (N, a separator)
    for (int v = 0; v < nvalues; ++v) {
        const int b = bases_of[values[v]];
        if (b == 1 || b == 2 || b == 4 || b == 8) base_of_code[v] = static_cast<uint8_t>(b);
    }
    for (uint32_t j = 0; j < m; ++j)
        if (bases_of[(uint8_t)P[j]] < 0) {
            set_error("%s: position %u: byte 0x%02x is no IUPAC nucleotide letter", call, j, (unsigned)(uint8_t)P[j]);
            return SMARTGPU_ERR_ARG;
        }
    for (uint32_t j = 0; j < m; ++j) {
        uint8_t s = 0;
        for (int v = 0; v < nvalues; ++v)
            if (bases_of[(uint8_t)P[j]] & base_of_code[v]) s |= static_cast<uint8_t>(1u << v);
        sets[j] = s;
    }
    return SMARTGPU_OK;
}

int smartgpu_iupac_sets(const uint8_t values[4], int nvalues, const char* P, uint32_t m, uint8_t* sets)
{
    return iupac_sets_impl("iupac_sets", 4, values, nvalues, P, m, sets);
}

int smartgpu_iupac_sets8(const uint8_t values[8], int nvalues, const char* P, uint32_t m, uint8_t* sets)
{
    return iupac_sets_impl("iupac_sets8", SMARTGPU_PTEXT_MAXVALUES, values, nvalues, P, m, sets);
}

int smartgpu_iupac_revcomp(const char* P, uint32_t m, char* out)
{
    if (m && (!P || !out)) { set_error("iupac_revcomp: NULL argument"); return SMARTGPU_ERR_ARG; }
    // the complement of every letter smartgpu_iupac_sets accepts; U reads as T
    static const char kPairs[][2] = {{'A', 'T'}, {'T', 'A'}, {'U', 'A'}, {'C', 'G'}, {'G', 'C'}, {'R', 'Y'}, {'Y', 'R'}, {'K', 'M'}, {'M', 'K'},
                                     {'B', 'V'}, {'V', 'B'}, {'D', 'H'}, {'H', 'D'}, {'S', 'S'}, {'W', 'W'}, {'N', 'N'}};
    char comp[256] = {0};
    for (const auto& e : kPairs) {
        comp[(uint8_t)e[0]] = e[1];
        comp[(uint8_t)(e[0] | 0x20)] = static_cast<char>(e[1] | 0x20);  // case is preserved
    }
    for (uint32_t j = 0; j < m; ++j)
        if (!comp[(uint8_t)P[j]]) {
            set_error("iupac_revcomp: position %u: byte 0x%02x is no IUPAC nucleotide letter", j, (unsigned)(uint8_t)P[j]);
            return SMARTGPU_ERR_ARG;
        }
    if (out == P) {  // in place: swap the ends
        for (uint32_t i = 0, j = m; i < j; ++i) {
            --j;
            const char lo = comp[(uint8_t)P[i]], hi = comp[(uint8_t)P[j]];
            out[i] = hi;
            out[j] = lo;
        }
    } else {
        for (uint32_t j = 0; j < m; ++j) out[j] = comp[(uint8_t)P[m - 1 - j]];
    }
    return SMARTGPU_OK;
}

}  // extern "C"
