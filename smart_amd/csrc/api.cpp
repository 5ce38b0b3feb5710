// api.cpp — C ABI of libsmartgpu (include/smartgpu.h): text residency in HBM,
// host-side preprocessing, launches, timing.  Compiled with hipcc as host code.
// The calls on packed texts, the approximate matchers and the align calls are
// match_calls.cpp; what the two units share is host_ctx.hpp, defined here.
//
// There is deliberately no CPU search path in this file or anywhere in the
// library: if HIP is not usable every compute entry point fails.
#include "../../include/smartgpu.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types, enums and prototypes only: the library itself is dlopen'ed on first use

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_ctx.hpp"
#include "kernels.hpp"
#include "multi.hpp"
#include "multi_find.hpp"
#include "multi_find_host.hpp"
#include "plan.hpp"
#include "route.hpp"
#include "sample.hpp"
#include "tables.hpp"
#include "text_rate.hpp"

namespace {

thread_local std::string g_error;
thread_local double g_last_pre_ms = 0.0, g_last_run_ms = 0.0;

}  // namespace

// ---- what host_ctx.hpp declares for match_calls.cpp is defined outside the anonymous namespaces: here, and further down
// device_ctx_flushed, batch_reserve, find_reserve and copy_positions ----

void set_error(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}

// (host_ctx.hpp) what a count call answers, and how match_calls.cpp sets the times smartgpu_last_times reports
int pcount_done(uint64_t c, double pre, double run, uint64_t* count, double* pre_ms, double* run_ms)
{
    g_last_pre_ms = pre;
    g_last_run_ms = run;
    if (count) *count = c;
    if (pre_ms) *pre_ms = pre;
    if (run_ms) *run_ms = run;
    return SMARTGPU_OK;
}

double now_ms()
{
    using clk = std::chrono::steady_clock;  // CLOCK_MONOTONIC, as src/timer.h:43-55
    return std::chrono::duration<double, std::milli>(clk::now().time_since_epoch()).count();
}

// `reps` passes of probe_read over [first, first + bytes) after one warm-up pass, timed by two events of its own: both
// are released on every path
int probe_read_ms(const DeviceCtx* d, const uint8_t* first, uint64_t bytes, unsigned long long* sink, int reps, double* ms_per_pass)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const auto timed = [&]() -> int {
        HIP_TRY(hipEventCreate(&e0), return SMARTGPU_ERR_HIP);
        HIP_TRY(hipEventCreate(&e1), return SMARTGPU_ERR_HIP);
        sg::launch_probe_read(first, bytes, sink, d->num_cus, d->stream);  // warm-up
        hipEventRecord(e0, d->stream);
        for (int i = 0; i < reps; ++i) sg::launch_probe_read(first, bytes, sink, d->num_cus, d->stream);
        hipEventRecord(e1, d->stream);
        HIP_TRY(hipEventSynchronize(e1), return SMARTGPU_ERR_HIP);
        float ms = 0.f;
        hipEventElapsedTime(&ms, e0, e1);
        *ms_per_pass = ms / reps;
        return SMARTGPU_OK;
    };
    const int rc = timed();
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    return rc;
}

namespace {

constexpr int kMaxDevices = 16;

DeviceCtx g_dev[kMaxDevices];

DeviceCtx* device_ctx(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("no HIP device available (hipGetDeviceCount)");
        return nullptr;
    }
    if (device < 0 || device >= n || device >= kMaxDevices) {
        set_error("device %d out of range (have %d)", device, n);
        return nullptr;
    }
    DeviceCtx& d = g_dev[device];
    HIP_TRY(hipSetDevice(device), return nullptr);
    if (!d.ready) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device), return nullptr);
        d.num_cus = prop.multiProcessorCount;
        d.device = device;
        HIP_TRY(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking), return nullptr);
        d.pinned_bytes = sg::kStagingBytes;  // (multi_find.hpp: find_batch_max counts on it)
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&d.pinned), d.pinned_bytes, hipHostMallocDefault),
                return nullptr);
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&d.pinned_count), 64, hipHostMallocDefault),
                return nullptr);
        d.ready = true;
    }
    return &d;
}

// device_ctx without a HIP call where the device has been set up — and WITHOUT making it current: for
// smartgpu_plan_launch, whose launches are mostly queued (below) and touch the device only when a key is sent.  Two HIP
// calls per launch were a visible part of the host's launch loop once a pass took 84 launches: that loop, not the GPU,
// bounds the flagship workload (profiles/coalesce/RESULTS.md).  Whoever sends makes the device current (send_key).
DeviceCtx* device_ctx_ready(int device)
{
    if (device >= 0 && device < kMaxDevices && g_dev[device].ready) return &g_dev[device];
    return device_ctx(device);
}

// hor_flat, bm_scan, bndm_scan and kmp_runs address LDS by absolute offset; a kernel that finds its dynamic segment
// elsewhere than at offset 0 (a static __shared__ crept into it) adds 2^62 to its count and returns.  No text has
// 2^62 start positions: such a count is reported as an error, never as a result.
constexpr unsigned long long kPoisonedCount = 1ull << 62;
bool count_poisoned(unsigned long long c)
{
    if (c < kPoisonedCount) return false;
    set_error("a scan kernel found its LDS segment displaced (static LDS in a kernel that addresses LDS by offset): count poisoned");
    return true;
}

}  // namespace

struct smartgpu_plan {
    int device = 0;
    int algo = 0;
    uint32_t m = 0;
    sg::PlanWords words;  // see plan.hpp
    uint8_t* blob = nullptr;               // device: pattern + tables
    uint8_t tail[sg::kTailRow] = {};       // host: the pattern's end as a shared pass takes it by value (multi.hpp)
    uint8_t head[sg::kSampleRow] = {};     // host: its first 31 bytes as a sampled pass takes them by value (sample.hpp)
    unsigned long long* results = nullptr; // device: kResultSlots counters (library-owned)
    unsigned long long* ext_results = nullptr; // caller-owned device buffer, if set
    int ext_slots = 0;
    unsigned long long* slot_ptr(int slot) const { return ext_results ? ext_results + slot : results + slot; }
    int num_slots() const { return ext_results ? ext_slots : sg::kResultSlots; }
    hipEvent_t ev0[sg::kResultSlots] = {}; // created lazily for timed launches
    hipEvent_t ev1[sg::kResultSlots] = {};
    bool timed[sg::kResultSlots] = {};
    double pre_ms = 0.0;
};

namespace {

smartgpu_text* text_alloc(uint64_t n, int device, DeviceCtx** ctx_out)
{
    DeviceCtx* d = device_ctx(device);
    if (!d) return nullptr;
    smartgpu_text* t = new smartgpu_text;
    t->device = device;
    t->n = n;
    const uint64_t total = sg::kFrontPad + n + sg::kBackPad;
    if (hipMalloc(reinterpret_cast<void**>(&t->base), total) != hipSuccess) {
        set_error("hipMalloc of %llu bytes failed", (unsigned long long)total);
        delete t;
        return nullptr;
    }
    // pads are zero; they are never counted as text, only read by whole-tile loads
    if (hipMemsetAsync(t->base, 0, sg::kFrontPad, d->stream) != hipSuccess ||
        hipMemsetAsync(t->base + sg::kFrontPad + n, 0, sg::kBackPad, d->stream) != hipSuccess) {
        set_error("hipMemsetAsync of the text pads failed");
        hipFree(t->base);
        delete t;
        return nullptr;
    }
    *ctx_out = d;
    return t;
}

// One pass over a text that has just been written (upload, tile fill, generator): which byte values it holds.  A text
// is never written again (ownership), so the answer holds for every later search, of any part of it.
// The 256 bits collect in the text's OWN front pad (bytes 64..95 of the allocation — zeroed with the pad; no scan reads
// below byte 152 of it: the pad is kXSize + 256 bytes and more), not in a per-device buffer: two threads that create
// texts on one device cannot interleave their passes.
constexpr size_t kAlphabetScratchOff = 64;
static_assert(kAlphabetScratchOff + 32 <= sg::kFrontPad - (SMARTGPU_XSIZE + 256), "the scratch must lie below every byte a scan can read");
static_assert(sg::kHitSlotsOff >= kAlphabetScratchOff + 32 && sg::kHitSlotsOff + sg::kHitSlots * 128 <= sg::kFrontPad - (SMARTGPU_XSIZE + 256),
              "flush_hits' staging slots lie between the scratch and the bytes a scan can read");
// The byte histogram of the text's sample (text_rate.hpp) is taken behind it on the same stream and read back before the
// same synchronisation.  Its 2 KB of counters do NOT fit the pad (the asserts above leave the scratch 32 bytes): they
// are a device allocation of this call, released before it returns.
bool text_alphabet(smartgpu_text* t, DeviceCtx* d)
{
    uint32_t* dev = reinterpret_cast<uint32_t*>(t->base + kAlphabetScratchOff);
    uint64_t hist[256] = {};
    unsigned long long* dev_hist = nullptr;
    const bool with_rate = sg::g_text_histogram && sg::rate_sample(t->n).bytes() >= 2;
    hipError_t e = hipMemsetAsync(dev, 0, 32, d->stream);
    if (e == hipSuccess && with_rate) e = hipMalloc(reinterpret_cast<void**>(&dev_hist), sizeof hist);
    if (e == hipSuccess && with_rate) e = hipMemsetAsync(dev_hist, 0, sizeof hist, d->stream);
    if (e == hipSuccess && t->n) e = sg::launch_text_alphabet(t->data(), t->n, dev, d->num_cus, d->stream);
    if (e == hipSuccess && with_rate) e = static_cast<hipError_t>(sg::g_text_histogram(t->data(), t->n, dev_hist, d->num_cus, d->stream));
    if (e == hipSuccess) e = hipMemcpyAsync(t->alphabet, dev, 32, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess && with_rate) e = hipMemcpyAsync(hist, dev_hist, sizeof hist, hipMemcpyDeviceToHost, d->stream);
    const hipError_t synced = hipStreamSynchronize(d->stream);  // (also after a failure: nothing may still write to hist)
    if (e == hipSuccess) e = synced;
    if (dev_hist) (void)hipFree(dev_hist);
    if (e != hipSuccess) { set_error("text_alphabet failed: %s", hipGetErrorString(e)); return false; }
    t->rate = with_rate ? sg::text_repeat_rate(hist) : -1.0;
    if (!sg::four_symbol_codes(t->alphabet, &t->four_shift, &t->four_symtab)) t->four_shift = 7;
    // one-bit codes of a text of at most two byte values: the lowest bit in which they differ (one value: bit 0)
    t->one_bit = 0xFF;
    {
        uint32_t syms[3], ns = 0;
        for (uint32_t c = 0; c < 256 && ns < 3; ++c)
            if (t->alphabet[c >> 5] >> (c & 31) & 1u) syms[ns++] = c;
        if (ns == 1) syms[ns++] = syms[0];
        if (ns == 2) {
            uint32_t bit = 0;
            while (bit < 7 && ((syms[0] ^ syms[1]) >> bit & 1u) == 0) ++bit;
            const uint32_t s0 = (syms[0] >> bit & 1u) ? syms[1] : syms[0], s1 = (syms[0] >> bit & 1u) ? syms[0] : syms[1];
            t->one_bit = bit | (s0 << 8) | (s1 << 16);
        }
    }
    // the kernels' copy: the first three words of the allocation (TextCodes, kernels.hpp)
    const uint32_t words[3] = {t->four_shift, t->four_symtab, t->one_bit};
    if (hipMemcpyAsync(t->base, words, 12, hipMemcpyHostToDevice, d->stream) != hipSuccess ||
        hipMemsetAsync(dev, 0, 32, d->stream) != hipSuccess ||  // the pad is zero again
        hipStreamSynchronize(d->stream) != hipSuccess) {
        set_error("text_alphabet: writing the codes failed");
        return false;
    }
    return true;
}

// A text that is searched ONCE (the int search(P, m, T, n) shims upload it per call): no alphabet pass — a full
// read of the text and two synchronisations for a table form that one search does not pay back.  The runs kernels
// then take their byte-wise forms (shift 7 = "not a four-symbol text"), which are correct on any text.
bool text_no_alphabet(smartgpu_text* t, DeviceCtx* d)
{
    t->four_shift = 7;
    t->four_symtab = 0;
    t->one_bit = 0xFF;
    t->rate = -1.0;  // not measured either: no pattern whose symbols repeat rides in a pass over this text
    for (uint32_t& wv : t->alphabet) wv = 0xFFFFFFFFu;  // unknown: every byte value may occur
    const uint32_t words[3] = {7u, 0u, 0xFFu};
    if (hipMemcpyAsync(t->base, words, 12, hipMemcpyHostToDevice, d->stream) != hipSuccess || hipStreamSynchronize(d->stream) != hipSuccess) {
        set_error("text upload: writing the codes failed");
        return false;
    }
    return true;
}

// The least text, in bytes, that gets a sample when it is created; -1: none does (smartgpu_text_sampling).  The sample
// costs a read of the text when it is made and n / 7 bytes while the text lives (profiles/coalesce/RESULTS.md).
std::atomic<long long> g_text_sampling{64ll << 20};

// The sample of a text that has just been written, built on the text's stream behind the alphabet pass.  Nothing here
// is an error: a text without a sample is searched as before.
void text_sample(smartgpu_text* t, DeviceCtx* d)
{
    const long long least = g_text_sampling.load(std::memory_order_relaxed);
    if (least < 0 || t->n < static_cast<uint64_t>(least) || !sg::g_sample_build) return;
    uint32_t* s = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&s), sg::sample_alloc_dwords(t->n) * 4) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    if (sg::g_sample_build(t->data(), t->n, s, d->num_cus, d->stream) != hipSuccess || hipStreamSynchronize(d->stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(s);
        return;
    }
    t->sample = s;
}

// The pattern checks of every entry point: algorithm id, applicability, length.  length_first: smartgpu_plan_create's order
// (a pattern that is both too short for the algorithm and not a pattern at all — m = 0, P = NULL — is reported as the latter).
int check_pattern(int algo, const uint8_t* P, uint32_t m, bool length_first = false)
{
    if (algo < 0 || algo >= SMARTGPU_NUM_ALGOS) { set_error("unknown algorithm id %d", algo); return SMARTGPU_ERR_ARG; }
    const bool na = m < sg::min_pattern(algo);
    if ((!na || length_first) && (!P || m < 1 || m > SMARTGPU_XSIZE)) { set_error("pattern length %u outside [1,%d]", m, SMARTGPU_XSIZE); return SMARTGPU_ERR_ARG; }
    if (na) { set_error("%s: not applicable for m < %u", sg::kAlgoNames[algo], sg::min_pattern(algo)); return SMARTGPU_NA; }
    return SMARTGPU_OK;
}

int check_search_args(int algo, const uint8_t* P, uint32_t m, const smartgpu_text* text,
                      uint64_t off, uint64_t n)
{
    const int rc = check_pattern(algo, P, m);
    if (rc != SMARTGPU_OK) return rc;
    if (!text) { set_error("text handle is NULL"); return SMARTGPU_ERR_ARG; }
    if (off > text->n || n > text->n - off) { set_error("range [%llu,+%llu) outside the text (%llu bytes)", (unsigned long long)off, (unsigned long long)n, (unsigned long long)text->n); return SMARTGPU_ERR_ARG; }
    return SMARTGPU_OK;
}

// what a scan receives: a plan's words, its tables on the device and its count slot, over n bytes of the text from `off`
sg::ScanArgs make_args(const sg::PlanWords& pw, uint32_t m, const uint8_t* blob, unsigned long long* count, const smartgpu_text* text,
                       uint64_t off, uint64_t n)
{
    const uint64_t s_end = (n >= m) ? off + n - m + 1 : off;  // no window fits: empty range
    return sg::ScanArgs{text->data(), off, s_end, m, pw.halo, /* fp_off: launch_scan */ 0, pw.prefer_packed, pw.sparse, pw.so_off, blob, count};
}

// ---- searches that share a pass over the text (k_horm.hip: hor_multi_scan) -------------------------------------------
// A streaming Horspool scan runs at the rate the text can be read, so what is left to save lies BETWEEN searches: K plans
// launched over the same text read it K times.  smartgpu_plan_launch therefore does not send a launch that would reach
// launch_hor's streaming branch (route {hor, 0}, a sparse pattern); it queues the finished arguments per device under
// (text, range, m, halo).  A key that has collected its width — g_coalesce launches, or what the arguments of a pass of
// its length have room for (sg::pass_width(m), at most kPassMax = 96) if that is less — is sent at once as ONE
// hor_multi_scan — the GPU never waits for a flush while full groups exist, and fewer than a width per key are ever pending.
// (Sending a key that is still gathering whenever it held a multiple of 32 launches and hipStreamQuery found the stream
// idle was tried and left out: on the flagship workload it changed ms_per_step by less than the run-to-run spread —
// profiles/coalesce/RESULTS.md.)  Every
// entry point that waits for, times, orders work on, or frees what is on the device's stream sends what is pending
// first (flush_queue), in arrival order; a launch that is alone by then goes through launch_scan as it always did.
// An untimed launch that cannot share a pass (another algorithm, a pattern whose symbols repeat over a text whose symbols
// repeat as well, or with no key gathering for it) is no such entry point: it is sent at once, ahead of what is pending,
// and a key goes on gathering its launches across it.  A pattern whose symbols repeat over a text where symbols do NOT
// (the text's measured rate, text_rate.hpp) RIDES in the key that is gathering for its text, range and length: the rules
// stand at queue_launch.  Such a launch used to read the whole text for one pattern, a quarter of the flagship's reads
// and nearly all of them at m = 8 and 16 (profiles/coalesce/RESULTS.md).
// The queue holds device pointers of plans and texts: smartgpu_plan_free, _plan_set_result_buffer and _text_free flush.
// The plan's tail row is copied, not pointed to.
// LONG passes.  pass_width(m) is what the kernel's arguments hold BY VALUE, not what the kernel can walk: its LDS has
// room for sg::long_width(m) patterns (152 at m = 32 against 84) when a pass carries pointers only and reads its rows
// from the plans' blobs (multi.hpp).  When launches keep arriving, the read of the text a wider pass saves is worth far
// more than the dependent read its prologue adds; what a wider pass costs is the WAIT until it is full, and that wait
// is free only while the GPU has something to do.  The queue cannot ask the GPU (a HIP call in a launch that is only
// queued was measured and left out, above), so the rule is one it can decide alone: a key that reaches pass_width(m)
// is sent at once, as ever, UNLESS (a) its range is at least g_coalesce_long bytes and (b) the previous pass of the same
// (text, range, m, halo) was sent because it was full — not by a flush — and no flush has happened since.  Then a
// pass of that key is on the stream or was a moment ago, the launches come faster than the GPU reads, and the key goes on
// gathering to long_width(m); it is sent there, or by the next flush, in the long layout if it holds more than
// pass_width(m) entries.  After any flush the GPU is presumably idle, and the first pass of a key leaves at
// pass_width(m) again: waiting longer would only lengthen the lead-in, UNLESS (c) the launches arrive faster than that:
// (b) was chosen when a launch cost the host a microsecond (ctypes) and pass_width(m) of them took longer than a pass.
// Through the native binding (fastcall.cpp) a launch takes 40 ns, 84 of them 3 us, and a first pass sent at 84 only
// makes the second wait behind it: on the flagship 34 + 34 us in two passes against 42 us in one of 200
// (profiles/coalesce/RESULTS.md).  So the key notes the host clock when it is opened, and the launch that fills it to
// pass_width(m) reads it once more: what the GPU would idle while the key gathers on to long_width(m), at the rate its
// launches came so far, against what a pass over the range takes (pass_estimate_ns; a pass estimated below 10 us, 44 MB
// of text or 308 MB under a sample, is sent as ever).  Shorter: the key goes on gathering as under (b).  Two reads of the clock per key, none in any other launch, and still no HIP call.
// (a): below 64 MiB a read of the range takes
// some 10 us, the host's 1.3 us per launch bounds the run and not the GPU, and a second read costs nothing that a longer
// wait would win back.  Long passes exist under the widest setting (kPassMax) only: a narrower one asks for exactly
// that many launches per pass.
// SAMPLED passes.  A key whose text has a sample (sample.hpp) and whose patterns have at least kSampleMinM = 31 bytes is
// sent to hor_sample_scan (k_hors.hip) while smartgpu_coalesce_sample is on: the same arguments in both layouts with the
// patterns' FIRST bytes for rows, 84 by value at every length and 252 in a long pass, and the room a key has follows the
// kernel it will be sent to.  Which launches are eligible, the riders, the rule for long passes and the key of one
// launch are as they were.  An entry carries its text's sample pointer and its plan's head row.
struct QueuedScan { int algo; sg::ScanArgs a; sg::TextCodes codes; uint8_t tail[sg::kTailRow]; uint8_t head[sg::kSampleRow]; const uint32_t* sample; };
bool same_key(const sg::ScanArgs& x, const sg::ScanArgs& a) { return x.text == a.text && x.s_begin == a.s_begin && x.s_end == a.s_end && x.m == a.m && x.halo == a.halo; }
struct QueuedKey {
    sg::ScanArgs key;  // text, s_begin, s_end, m, halo
    uint32_t n = 0;          // entries: streaming launches and riders
    uint32_t streaming = 0;  // the streaming launches among them: what the coalesce setting counts
    int64_t opened_ns = 0;   // the host clock when the key was opened (rule (c) of the long passes)
    bool fast = false;       // (c) held when the key reached pass_width(m): it gathers on to long_width(m)
    QueuedScan scans[sg::kLongMax];
    bool holds(const sg::ScanArgs& a) const { return same_key(key, a); }
    void take(const QueuedKey& o)  // (the entries it holds, not all kLongMax)
    {
        key = o.key;
        n = o.n;
        streaming = o.streaming;
        opened_ns = o.opened_ns;
        fast = o.fast;
        std::memcpy(static_cast<void*>(scans), static_cast<const void*>(o.scans), o.n * sizeof(QueuedScan));
    }
};
static_assert(std::is_trivially_copyable<QueuedScan>::value, "QueuedKey::take copies entries as bytes");
static_assert(SMARTGPU_XSIZE - 1 - sg::kGramCap + sg::kTailRow <= sg::kPatternBytes, "a long pass reads whole rows from a blob's pattern slot");
struct LaunchQueue {
    std::mutex mu;
    static constexpr uint32_t kKeys = 8;  // a ninth key sends the oldest
    uint32_t nkeys = 0;
    QueuedKey keys[kKeys];  // in arrival order
    void drop(uint32_t at) { for (--nkeys; at < nkeys; ++at) keys[at].take(keys[at + 1]); }
    // the keys whose last pass was sent because it was full, since the last flush (a ninth replaces the oldest)
    uint32_t nfull = 0, full_next = 0;
    sg::ScanArgs full[kKeys];
    bool was_full(const sg::ScanArgs& a) const
    {
        for (uint32_t i = 0; i < nfull; ++i)
            if (same_key(full[i], a)) return true;
        return false;
    }
    void note_full(const sg::ScanArgs& a)
    {
        if (was_full(a)) return;
        if (nfull < kKeys) { full[nfull++] = a; return; }
        full[full_next] = a;
        full_next = (full_next + 1) % kKeys;
    }
    bool off = false;             // smartgpu_stream_handle gave the stream out: its holder orders their own work on it
    uint64_t launches = 0, passes = 0;  // eligible launches seen / kernels sent for them
    uint64_t riders = 0;                // launches that rode in a key's pass (not among `launches`)
    uint64_t sampled = 0;               // the passes among `passes` that went to hor_sample_scan
};
LaunchQueue g_queue[kMaxDevices];
// the least range, in bytes of start positions, whose keys gather long passes; -1: none do (smartgpu_coalesce_long)
std::atomic<long long> g_coalesce_long{64ll << 20};
// launches per pass: 0 = off, 2..kPassMax.  ONE number with three calls: smartgpu_coalesce, the first, sets 0 or
// 2..kCoalesceNarrow and reports a wider value as kCoalesceNarrow; smartgpu_coalesce_wide sets 0 or 2..kMultiMax and
// reports a wider value as kMultiMax; smartgpu_coalesce_pass sets and reports all of it.
// The default is the widest pass, clipped per key to sg::pass_width(m): per pattern on 1 GiB of rand128 at m = 32,
// 0.0202 / 0.0055 / 0.0034 / 0.0028 ms in passes of 8 / 32 / 64 / 84, and the widest pass is the fastest at m = 16, 64 and
// 256 as well (profiles/coalesce/RESULTS.md), so no length gets a cap beyond what its rows leave room for.
constexpr int kCoalesceNarrow = 8;
std::atomic<int> g_coalesce{sg::kPassMax};
// sampled passes on / off (smartgpu_coalesce_sample), and the workgroups of one (smartgpu_coalesce_sample_grid; 0: one per CU)
std::atomic<int> g_coalesce_sample{1};
std::atomic<int> g_sample_grid{0};
// does a pass of length m over a text with this sample go to hor_sample_scan?
bool pass_sampled(const uint32_t* sample, uint32_t m)
{
    return sample && m >= sg::kSampleMinM && sg::g_hor_sample && g_coalesce_sample.load(std::memory_order_relaxed) != 0;
}

int64_t host_ns()
{
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// What a pass over `range` start positions takes, for rule (c) of the long passes: the bytes it reads (a sampled pass
// 4 of every 28) at 4.4 TB/s, the rate of hor_sample_scan on 1 GiB (35 us; hor_multi_scan reads 1 GiB in 180 us, 5.9 TB/s:
// the estimate is a third too long there, on the side of gathering).  A rule of thumb for a choice between one pass and
// two, not a model.
// Below 10 us the estimate decides nothing: such a pass is mostly its prologue and the dispatch, which it leaves out.
constexpr int64_t kFastLeastNs = 10000;
int64_t pass_estimate_ns(uint64_t range, bool sampled)
{
    const uint64_t bytes = sampled ? range / (sg::kSampleStride / sg::kSampleGram) : range;
    return static_cast<int64_t>(bytes / 4400u);
}

// send one key's launches (q.mu held); makes the device current
hipError_t send_key(const DeviceCtx* d, LaunchQueue& q, QueuedKey& k)
{
    hipError_t e = k.n ? hipSetDevice(d->device) : hipSuccess;
    if (e != hipSuccess) {
        k.n = 0;
        k.streaming = 0;
        return e;
    }
    if (k.n == 1) {  // (a streaming launch: a rider never opens a key)
        e = sg::launch_scan(k.scans[0].algo, k.scans[0].a, d->num_cus, d->stream, k.scans[0].codes);
    } else if (k.n > 1) {
        sg::MultiArgs ma;  // (not zeroed: 4 KB, and the kernel reads the entries of np patterns only)
        ma.text = k.key.text;
        ma.s_begin = k.key.s_begin;
        ma.s_end = k.key.s_end;
        ma.m = k.key.m;
        ma.halo = k.key.halo & 0xFFu;  // as prepare_scan_args: H without the plan's marks
        ma.np = k.n;
        const uint32_t* sample = k.scans[0].sample;  // (a key has one text)
        if (pass_sampled(sample, k.key.m)) {  // over the sample: the patterns' heads by value, or the pointers alone
            const bool by_value = k.n <= sg::kSampleWidth;
            ma.stride = sg::kSampleRow;
            ma.width = by_value ? sg::kSampleWidth : sg::kSampleLongWidth;
            ma.reserved = by_value ? sg::kMultiByValue : sg::kMultiLong;
            for (uint32_t j = 0; j < k.n; ++j) {
                if (by_value) sg::sample_set(ma, j, k.scans[j].a.blob, k.scans[j].a.count, k.scans[j].head);
                else sg::multi_set_long(ma, j, k.scans[j].a.blob, k.scans[j].a.count);
            }
            e = sg::g_hor_sample(ma, sample, d->num_cus, g_sample_grid.load(std::memory_order_relaxed), d->stream);
            if (e == hipSuccess) ++q.sampled;
        } else {
            ma.stride = sg::tail_stride(k.key.m);
            if (k.n <= sg::pass_width(k.key.m)) {
                ma.width = sg::pass_width(k.key.m);
                ma.reserved = sg::kMultiByValue;
                for (uint32_t j = 0; j < k.n; ++j) sg::multi_set(ma, j, k.scans[j].a.blob, k.scans[j].a.count, k.scans[j].tail);
            } else {  // a long pass: the pointers alone, the rows are read from the blobs
                ma.width = sg::long_width(k.key.m);
                ma.reserved = sg::kMultiLong;
                for (uint32_t j = 0; j < k.n; ++j) sg::multi_set_long(ma, j, k.scans[j].a.blob, k.scans[j].a.count);
            }
            e = sg::g_hor_multi(ma, d->num_cus, d->stream);
        }
    }
    if (k.n && e == hipSuccess) ++q.passes;
    k.n = 0;
    k.streaming = 0;
    return e;
}

// send everything that is pending on the device (which must be current), in arrival order
hipError_t flush_queue(const DeviceCtx* d)
{
    LaunchQueue& q = g_queue[d->device];
    std::lock_guard<std::mutex> lock(q.mu);
    hipError_t err = hipSuccess;
    for (uint32_t i = 0; i < q.nkeys; ++i) {
        const hipError_t e = send_key(d, q, q.keys[i]);
        if (e != hipSuccess && err == hipSuccess) err = e;
    }
    q.nkeys = 0;
    q.nfull = q.full_next = 0;  // whatever comes next finds, presumably, an idle GPU: its first pass leaves at pass_width(m)
    return err;
}

// the same for every device that has been used, whichever is current (smartgpu_tune, smartgpu_coalesce: no device argument)
void flush_all_queues()
{
    int current = -1;
    for (int i = 0; i < kMaxDevices; ++i) {
        if (!g_dev[i].ready) continue;
        {
            std::lock_guard<std::mutex> lock(g_queue[i].mu);
            if (g_queue[i].nkeys == 0) continue;
        }
        if (current < 0 && hipGetDevice(&current) != hipSuccess) return;
        if (hipSetDevice(i) == hipSuccess) (void)flush_queue(&g_dev[i]);
    }
    if (current >= 0) (void)hipSetDevice(current);
}

}  // namespace

// device_ctx for an entry point that waits for the device's stream or puts work of its own on it
DeviceCtx* device_ctx_flushed(int device)
{
    DeviceCtx* d = device_ctx(device);
    if (!d) return nullptr;
    const hipError_t e = flush_queue(d);
    if (e != hipSuccess) { set_error("a queued launch failed: %s", hipGetErrorString(e)); return nullptr; }
    return d;
}

namespace {

// Queue the launch if it is one that can share a pass.  *queued = false: the caller launches it (after flush_queue).
// A RIDER is a launch of the same route whose pattern's own symbols repeat (words.sparse == 0, m >= 8) over a text whose
// measured rate says that they do not repeat THERE (text_rate: at most 1/48): its windows die on their first bytes like
// a streaming pattern's, and hor_multi_scan compares whole windows, so it counts any pattern exactly.  A rider joins a
// key that is already gathering for its (text, range, m, halo) and leaves with that key's pass; it never opens a key —
// with none it is the caller's to launch, as before — so a text whose patterns all repeat never forms a pass of them.
// It counts neither in `launches` nor toward the coalesce setting; it does take one of the pass_width(m) places a key has.
hipError_t queue_launch(const DeviceCtx* d, int algo, const sg::PlanWords& words, const sg::ScanArgs& a, const sg::TextCodes& codes,
                        double text_rate, const uint8_t (&tail)[sg::kTailRow], const uint8_t (&head)[sg::kSampleRow], const uint32_t* sample,
                        bool timed, bool* queued)
{
    *queued = false;
    if (a.s_end <= a.s_begin) return hipSuccess;
    const bool rider = !words.sparse;
    if (rider && (a.m < 8 || !sg::text_rate_streams(text_rate))) return hipSuccess;
    const sg::Route r = sg::route(algo, a.m, words, codes);
    if (r.to != sg::Launcher::hor || r.arg != 0) return hipSuccess;
    LaunchQueue& q = g_queue[d->device];
    std::lock_guard<std::mutex> lock(q.mu);
    if (!rider) ++q.launches;
    const int G = g_coalesce.load(std::memory_order_relaxed);
    if (timed || G < 2 || q.off || !sg::g_hor_multi) {
        if (!rider) ++q.passes;
        return hipSuccess;
    }
    hipError_t err = hipSuccess;
    uint32_t at = 0;
    while (at < q.nkeys && !q.keys[at].holds(a)) ++at;
    if (at == q.nkeys) {
        if (rider) return hipSuccess;  // no key is gathering for it: alone, at once
        if (q.nkeys == LaunchQueue::kKeys) {
            err = send_key(d, q, q.keys[0]);
            q.drop(0);
        }
        at = q.nkeys++;
        q.keys[at].key = a;
        q.keys[at].n = 0;
        q.keys[at].streaming = 0;
        q.keys[at].fast = false;
        q.keys[at].opened_ns = host_ns();
    }
    QueuedKey& k = q.keys[at];  // (has room: a key that reached its width was sent by the launch that filled it)
    QueuedScan& qs = k.scans[k.n++];
    qs.algo = algo;
    qs.a = a;
    qs.codes = codes;
    std::memcpy(qs.tail, tail, sg::kTailRow);
    std::memcpy(qs.head, head, sg::kSampleRow);
    qs.sample = sample;
    if (rider) ++q.riders; else ++k.streaming;
    // the room a key has follows the kernel it will be sent to (at most kPassMax by value)
    const bool sampled = pass_sampled(sample, a.m);
    const uint32_t room = sampled ? sg::kSampleWidth : sg::pass_width(a.m);
    const uint32_t long_room = sampled ? sg::kSampleLongWidth : sg::long_width(a.m);
    const uint32_t width = static_cast<uint32_t>(G) < room ? static_cast<uint32_t>(G) : room;
    // a long pass (the rule stands above the queue): launches and riders together, up to long_width(m)
    const long long least = g_coalesce_long.load(std::memory_order_relaxed);
    const bool may_gather = G == sg::kPassMax && least >= 0 && a.s_end - a.s_begin >= static_cast<uint64_t>(least);
    const bool full = k.streaming >= width || k.n >= room;
    if (may_gather && full && !k.fast && k.n < long_room && !q.was_full(a)) {  // (c), asked once: by the launch that fills the key
        const int64_t waited = host_ns() - k.opened_ns;  // for k.n launches; long_room - k.n more would take about as long each
        const int64_t pass_ns = pass_estimate_ns(a.s_end - a.s_begin, sampled);
        k.fast = pass_ns >= kFastLeastNs && waited >= 0 && waited / k.n * (long_room - k.n) < pass_ns;
    }
    const bool gather_on = may_gather && (k.fast || q.was_full(a));
    if (gather_on ? k.n >= long_room : full) {
        q.note_full(k.key);
        const hipError_t e = send_key(d, q, k);
        if (e != hipSuccess && err == hipSuccess) err = e;
        q.drop(at);
    }
    *queued = true;
    return err;
}

}  // namespace

namespace sg {
hipError_t (*g_hor_multi)(const MultiArgs&, int, hipStream_t) = nullptr;  // multi.hpp: set by k_horm.hip where that unit is linked
hipError_t (*g_hor_multi_find)(const MultiFindArgs&, int, hipStream_t) = nullptr;  // multi_find.hpp: set by k_hormf.hip where that unit is linked
// sample.hpp: set by k_hors.hip where that unit is linked
hipError_t (*g_hor_sample)(const MultiArgs&, const uint32_t*, int, int, hipStream_t) = nullptr;
hipError_t (*g_sample_build)(const uint8_t*, uint64_t, uint32_t*, int, hipStream_t) = nullptr;
hipError_t (*g_hor_preload)() = nullptr;  // launch_common.hpp: set by k_hor.hip where that unit is linked
int (*g_text_histogram)(const uint8_t*, uint64_t, unsigned long long*, int, void*) = nullptr;  // text_rate.hpp: set by k_util.hip where that unit is linked
}

extern "C" {

const char* smartgpu_version(void)
{
#ifdef SMARTGPU_AB
    return "smartgpu 0.2 (gfx950, A/B build)";
#else
    return "smartgpu 0.2 (gfx950)";
#endif
}
const char* smartgpu_last_error(void) { return g_error.c_str(); }

int smartgpu_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { set_error("hipGetDeviceCount failed"); return SMARTGPU_ERR_HIP; }
    return n;
}

int smartgpu_algo_id(const char* name)
{
    if (!name) return -1;
    std::string s(name);
    for (auto& ch : s) ch = static_cast<char>(std::tolower(static_cast<unsigned char>(ch)));
    for (int i = 0; i < SMARTGPU_NUM_ALGOS; ++i)
        if (s == sg::kAlgoNames[i]) return i;
    return -1;
}

const char* smartgpu_algo_name(int algo)
{
    return (algo >= 0 && algo < SMARTGPU_NUM_ALGOS) ? sg::kAlgoNames[algo] : nullptr;
}

int smartgpu_device_sync(int device)
{
    DeviceCtx* d = device_ctx_flushed(device);
    if (!d) return SMARTGPU_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(d->stream), return SMARTGPU_ERR_HIP);
    return SMARTGPU_OK;
}

/* ---- text ------------------------------------------------------------- */
static smartgpu_text* text_upload_impl(const void* host, uint64_t n, int device, bool alphabet)
{
    if (!host && n) { set_error("host pointer is NULL"); return nullptr; }
    DeviceCtx* d = nullptr;
    smartgpu_text* t = text_alloc(n, device, &d);
    if (!t) return nullptr;
    const uint8_t* src = static_cast<const uint8_t*>(host);
    uint8_t* dst = t->base + sg::kFrontPad;
    for (uint64_t done = 0; done < n;) {  // pinned staging -> HBM
        const size_t chunk = static_cast<size_t>(std::min<uint64_t>(d->pinned_bytes, n - done));
        std::memcpy(d->pinned, src + done, chunk);
        if (hipMemcpyAsync(dst + done, d->pinned, chunk, hipMemcpyHostToDevice, d->stream) != hipSuccess ||
            hipStreamSynchronize(d->stream) != hipSuccess) {
            set_error("text upload failed at byte %llu", (unsigned long long)done);
            smartgpu_text_free(t);
            return nullptr;
        }
        done += chunk;
    }
    hipStreamSynchronize(d->stream);
    if (!(alphabet ? text_alphabet(t, d) : text_no_alphabet(t, d))) { smartgpu_text_free(t); return nullptr; }
    if (alphabet) text_sample(t, d);
    return t;
}

smartgpu_text* smartgpu_text_upload(const void* host, uint64_t n, int device) { return text_upload_impl(host, n, device, true); }

smartgpu_text* smartgpu_text_upload_tiled(const void* unit, uint64_t unit_len, uint64_t phase,
                                          uint64_t n, int device)
{
    if (!unit || unit_len == 0) { set_error("empty unit"); return nullptr; }
    smartgpu_text* u = smartgpu_text_upload(unit, unit_len, device);
    if (!u) return nullptr;
    DeviceCtx* d = nullptr;
    smartgpu_text* t = text_alloc(n, device, &d);
    if (!t) { smartgpu_text_free(u); return nullptr; }
    hipError_t e = sg::launch_tile_fill(t->base + sg::kFrontPad, u->data(), unit_len, phase % unit_len, n, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    smartgpu_text_free(u);
    if (e != hipSuccess) {
        set_error("tile_fill failed: %s", hipGetErrorString(e));
        smartgpu_text_free(t);
        return nullptr;
    }
    if (!text_alphabet(t, d)) { smartgpu_text_free(t); return nullptr; }
    text_sample(t, d);
    return t;
}

smartgpu_text* smartgpu_text_generate(uint64_t seed, int sigma, uint64_t off, uint64_t n, int device)
{
    if (sigma < 2 || sigma > 256) { set_error("sigma %d outside [2,256]", sigma); return nullptr; }
    DeviceCtx* d = nullptr;
    smartgpu_text* t = text_alloc(n, device, &d);
    if (!t) return nullptr;
    hipError_t e = sg::launch_generate(t->base + sg::kFrontPad, seed, sigma, off, n, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) {
        set_error("generate_text failed: %s", hipGetErrorString(e));
        smartgpu_text_free(t);
        return nullptr;
    }
    if (!text_alphabet(t, d)) { smartgpu_text_free(t); return nullptr; }
    text_sample(t, d);
    return t;
}

void smartgpu_text_free(smartgpu_text* t)
{
    if (!t) return;
    if (t->base) {
        hipSetDevice(t->device);
        if (t->device >= 0 && t->device < kMaxDevices && g_dev[t->device].ready) {  // launches over this text may be pending
            const hipError_t e = flush_queue(&g_dev[t->device]);
            if (e != hipSuccess) set_error("text_free: a queued launch failed: %s", hipGetErrorString(e));
        }
        hipFree(t->base);
        if (t->sample) hipFree(t->sample);
    }
    delete t;
}

uint64_t smartgpu_text_length(const smartgpu_text* t) { return t ? t->n : 0; }
int smartgpu_text_device(const smartgpu_text* t) { return t ? t->device : -1; }

int smartgpu_text_alphabet(const smartgpu_text* t, uint32_t bits[8])
{
    if (!t || !bits) { set_error("bad alphabet arguments"); return SMARTGPU_ERR_ARG; }
    std::memcpy(bits, t->alphabet, 32);
    return SMARTGPU_OK;
}

int smartgpu_text_repeat_rate(const smartgpu_text* t, double* rate)
{
    if (!t || !rate) { set_error("bad repeat_rate arguments"); return SMARTGPU_ERR_ARG; }
    *rate = t->rate;
    return SMARTGPU_OK;
}

int smartgpu_text_read(const smartgpu_text* t, uint64_t off, uint64_t len, void* host)
{
    if (!t || !host || off > t->n || len > t->n - off) { set_error("bad text_read range"); return SMARTGPU_ERR_ARG; }
    DeviceCtx* d = device_ctx_flushed(t->device);
    if (!d) return SMARTGPU_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(d->stream), return SMARTGPU_ERR_HIP);
    HIP_TRY(hipMemcpy(host, t->data() + off, len, hipMemcpyDeviceToHost), return SMARTGPU_ERR_HIP);
    return SMARTGPU_OK;
}

/* ---- plans ------------------------------------------------------------ */
smartgpu_plan* smartgpu_plan_create(int algo, const uint8_t* P, uint32_t m, int device)
{
    if (check_pattern(algo, P, m, true) != SMARTGPU_OK) return nullptr;
    DeviceCtx* d = device_ctx(device);
    if (!d) return nullptr;
    const double t0 = now_ms();
    smartgpu_plan* p = new smartgpu_plan;
    p->device = device;
    p->algo = algo;
    p->m = m;
    std::vector<uint8_t> blob;
    p->words = sg::build_blob(blob, algo, P, m);
    sg::tail_fill(p->tail, P, m);
    sg::sample_head_fill(p->head, P, m);
    if ((algo == SMARTGPU_HOR || algo == SMARTGPU_TUNEDBM) && sg::g_hor_preload && !d->hor_preloaded) {
        // hor_scan's code object and kernels now, not at the first launch that cannot share a pass (k_hor.hip)
        d->hor_preloaded = true;
        if (sg::g_hor_preload() != hipSuccess) (void)hipGetLastError();  // (a launch will report what is wrong)
    }
    bool ok = hipMalloc(reinterpret_cast<void**>(&p->blob), blob.size()) == hipSuccess &&
              hipMalloc(reinterpret_cast<void**>(&p->results), sizeof(unsigned long long) * sg::kResultSlots) == hipSuccess;
    if (ok) {
        std::memcpy(d->pinned, blob.data(), blob.size());
        ok = hipMemcpyAsync(p->blob, d->pinned, blob.size(), hipMemcpyHostToDevice, d->stream) == hipSuccess &&
             hipMemsetAsync(p->results, 0, sizeof(unsigned long long) * sg::kResultSlots, d->stream) == hipSuccess &&
             hipStreamSynchronize(d->stream) == hipSuccess;
    }
    if (!ok) {
        set_error("plan_create: device allocation or table upload failed (%s)", hipGetErrorString(hipGetLastError()));
        smartgpu_plan_free(p);
        return nullptr;
    }
    p->pre_ms = now_ms() - t0;
    return p;
}

void smartgpu_plan_free(smartgpu_plan* p)
{
    if (!p) return;
    hipSetDevice(p->device);
    if (p->device >= 0 && p->device < kMaxDevices && g_dev[p->device].ready) {  // launches of this plan may be pending
        const hipError_t e = flush_queue(&g_dev[p->device]);
        if (e != hipSuccess) set_error("plan_free: a queued launch failed: %s", hipGetErrorString(e));
    }
    for (int i = 0; i < sg::kResultSlots; ++i) {
        if (p->ev0[i]) hipEventDestroy(p->ev0[i]);
        if (p->ev1[i]) hipEventDestroy(p->ev1[i]);
    }
    if (p->blob) hipFree(p->blob);
    if (p->results) hipFree(p->results);
    delete p;
}

int smartgpu_plan_launch(smartgpu_plan* p, const smartgpu_text* text, uint64_t off, uint64_t n,
                         int slot, int timed)
{
    if (!p || !text) { set_error("plan or text is NULL"); return SMARTGPU_ERR_ARG; }
    if (slot < 0 || slot >= p->num_slots()) { set_error("slot %d out of range", slot); return SMARTGPU_ERR_ARG; }
    if (text->device != p->device) { set_error("plan is on device %d, text on %d", p->device, text->device); return SMARTGPU_ERR_ARG; }
    if (off > text->n || n > text->n - off) { set_error("range outside the text"); return SMARTGPU_ERR_ARG; }
    DeviceCtx* d = device_ctx_ready(p->device);  // (not current yet: a queued launch makes no HIP call)
    if (!d) return SMARTGPU_ERR_HIP;
    const sg::ScanArgs a = make_args(p->words, p->m, p->blob, p->slot_ptr(slot), text, off, n);
    bool queued = false;
    HIP_TRY(queue_launch(d, p->algo, p->words, a, text->codes(), text->rate, p->tail, p->head, text->sample, timed != 0, &queued), return SMARTGPU_ERR_HIP);
    if (queued) { p->timed[slot] = false; return SMARTGPU_OK; }
    HIP_TRY(hipSetDevice(p->device), return SMARTGPU_ERR_HIP);
    // A timed launch keeps its place behind what was queued before it: its events bracket this kernel alone.  Any other
    // launch that cannot share a pass goes ahead of what is pending: counts are ADDED to their slots, in any order, and
    // sending a half-filled key here costs its launches a pass of their own over the text.  (One m = 32 pattern in the
    // 250 of bench.py repeats its symbols: it used to turn the 25 passes of the 200 timed launches into 26 and a solo scan;
    // on that text it now rides in the pass that is gathering — queue_launch — and only without one comes here.)
    if (timed) HIP_TRY(flush_queue(d), return SMARTGPU_ERR_HIP);
    p->timed[slot] = timed != 0;
    if (timed) {
        if (!p->ev0[slot]) {
            HIP_TRY(hipEventCreate(&p->ev0[slot]), return SMARTGPU_ERR_HIP);
            HIP_TRY(hipEventCreate(&p->ev1[slot]), return SMARTGPU_ERR_HIP);
        }
        HIP_TRY(hipEventRecord(p->ev0[slot], d->stream), return SMARTGPU_ERR_HIP);
    }
    HIP_TRY(sg::launch_scan(p->algo, a, d->num_cus, d->stream, text->codes()), return SMARTGPU_ERR_HIP);
    if (timed) HIP_TRY(hipEventRecord(p->ev1[slot], d->stream), return SMARTGPU_ERR_HIP);
    return SMARTGPU_OK;
}

int smartgpu_plan_result(smartgpu_plan* p, int slot, uint64_t* count, double* kernel_ms)
{
    if (!p || slot < 0 || slot >= p->num_slots()) { set_error("bad plan/slot"); return SMARTGPU_ERR_ARG; }
    DeviceCtx* d = device_ctx_flushed(p->device);
    if (!d) return SMARTGPU_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(d->pinned_count, p->slot_ptr(slot), sizeof(unsigned long long), hipMemcpyDeviceToHost, d->stream),
            return SMARTGPU_ERR_HIP);
    HIP_TRY(hipStreamSynchronize(d->stream), return SMARTGPU_ERR_HIP);
    if (count_poisoned(*d->pinned_count)) return SMARTGPU_ERR_HIP;
    if (count) *count = *d->pinned_count;
    if (kernel_ms) {
        *kernel_ms = -1.0;
        if (p->timed[slot]) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, p->ev0[slot], p->ev1[slot]), return SMARTGPU_ERR_HIP);
            *kernel_ms = ms;
        }
    }
    return SMARTGPU_OK;
}

const char* smartgpu_plan_kernel_name(const smartgpu_plan* p)
{
    return p ? sg::scan_kernel_name(p->algo, p->m, p->words.prefer_packed != 0, p->words.so_off != 0, p->words.halo) : nullptr;
}

const char* smartgpu_kernel_for(int algo, const uint8_t* P, uint32_t m)
{
    if (check_pattern(algo, P, m) != SMARTGPU_OK) {
        set_error("kernel_for: algorithm %d / pattern length %u not applicable", algo, m);
        return nullptr;
    }
    std::vector<uint8_t> blob;
    const sg::PlanWords pw = sg::build_blob(blob, algo, P, m);
    return sg::scan_kernel_name(algo, m, pw.prefer_packed != 0, pw.so_off != 0, pw.halo);
}

void* smartgpu_plan_result_device_ptr(smartgpu_plan* p) { return p ? p->slot_ptr(0) : nullptr; }

int smartgpu_plan_reset(smartgpu_plan* p)
{
    if (!p) { set_error("plan is NULL"); return SMARTGPU_ERR_ARG; }
    DeviceCtx* d = device_ctx_flushed(p->device);
    if (!d) return SMARTGPU_ERR_HIP;
    HIP_TRY(hipMemsetAsync(p->slot_ptr(0), 0, sizeof(unsigned long long) * p->num_slots(), d->stream),
            return SMARTGPU_ERR_HIP);
    return SMARTGPU_OK;
}

int smartgpu_plan_set_result_buffer(smartgpu_plan* p, void* device_u64, int nslots)
{
    if (!p || (device_u64 && (nslots < 1 || nslots > sg::kResultSlots))) { set_error("bad result buffer"); return SMARTGPU_ERR_ARG; }
    if (!device_ctx_flushed(p->device)) return SMARTGPU_ERR_HIP;  // pending launches of this plan count into the buffer they were given
    p->ext_results = static_cast<unsigned long long*>(device_u64);
    p->ext_slots = device_u64 ? nslots : 0;
    return SMARTGPU_OK;
}

int smartgpu_stream_mark(int device, int which)
{
    DeviceCtx* d = device_ctx_flushed(device);
    if (!d || which < 0 || which > 1) return SMARTGPU_ERR_ARG;
    if (!d->mark[which]) HIP_TRY(hipEventCreate(&d->mark[which]), return SMARTGPU_ERR_HIP);
    HIP_TRY(hipEventRecord(d->mark[which], d->stream), return SMARTGPU_ERR_HIP);
    return SMARTGPU_OK;
}

int smartgpu_stream_elapsed_ms(int device, double* ms)
{
    DeviceCtx* d = device_ctx_flushed(device);
    if (!d || !ms || !d->mark[0] || !d->mark[1]) { set_error("stream marks not set"); return SMARTGPU_ERR_ARG; }
    HIP_TRY(hipEventSynchronize(d->mark[1]), return SMARTGPU_ERR_HIP);
    float f = 0.f;
    HIP_TRY(hipEventElapsedTime(&f, d->mark[0], d->mark[1]), return SMARTGPU_ERR_HIP);
    *ms = f;
    return SMARTGPU_OK;
}

int smartgpu_probe_read_ms(const smartgpu_text* t, int reps, double* ms_per_pass)
{
    if (!t || reps < 1 || !ms_per_pass) { set_error("bad probe arguments"); return SMARTGPU_ERR_ARG; }
    DeviceCtx* d = device_ctx_flushed(t->device);
    if (!d) return SMARTGPU_ERR_HIP;
    unsigned long long* sink = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&sink), 8), return SMARTGPU_ERR_HIP);
    const int rc = probe_read_ms(d, t->data(), t->n, sink, reps, ms_per_pass);
    hipFree(sink);
    return rc;
}

int smartgpu_tune(int key, int value)
{
    if (key < 0 || key >= 8) { set_error("tune key %d out of range", key); return SMARTGPU_ERR_ARG; }
    if (!sg::tune_supported(key, value)) {
        set_error("tune(%d,%d) selects a superseded kernel: only in the A/B build (make -C smart_amd/csrc AB=1 -> libsmartgpu_ab.so)", key, value);
        return SMARTGPU_ERR_ARG;
    }
    flush_all_queues();  // what is pending was launched under the settings of its time
    sg::g_tune[key] = value;
    return SMARTGPU_OK;
}

// the one setting behind smartgpu_coalesce (most = kCoalesceNarrow), smartgpu_coalesce_wide (most = kMultiMax) and
// smartgpu_coalesce_pass (most = kPassMax)
static int set_coalesce(int max_group, int most)
{
    if (max_group != 0 && (max_group < 2 || max_group > most)) { set_error("coalesce: a pass takes 2..%d launches (0: off), not %d", most, max_group); return SMARTGPU_ERR_ARG; }
    flush_all_queues();
    return g_coalesce.exchange(max_group);
}

int smartgpu_coalesce(int max_group)
{
    const int prev = set_coalesce(max_group, kCoalesceNarrow);
    return prev > kCoalesceNarrow ? kCoalesceNarrow : prev;
}

int smartgpu_coalesce_wide(int max_group)
{
    const int prev = set_coalesce(max_group, sg::kMultiMax);
    return prev > sg::kMultiMax ? sg::kMultiMax : prev;
}

int smartgpu_coalesce_pass(int max_group)
{
    return set_coalesce(max_group, sg::kPassMax);
}

long long smartgpu_coalesce_long(long long min_range_bytes)
{
    if (min_range_bytes < -1) { set_error("coalesce_long: the least range of a long pass is 0 or more bytes (-1: no long passes), not %lld", min_range_bytes); return SMARTGPU_ERR_ARG; }
    flush_all_queues();
    return g_coalesce_long.exchange(min_range_bytes);
}

int smartgpu_coalesce_stats(int device, uint64_t* launches, uint64_t* passes)
{
    if (device < 0 || device >= kMaxDevices) { set_error("device %d out of range", device); return SMARTGPU_ERR_ARG; }
    std::lock_guard<std::mutex> lock(g_queue[device].mu);
    if (launches) *launches = g_queue[device].launches;
    if (passes) *passes = g_queue[device].passes;
    return SMARTGPU_OK;
}

int smartgpu_coalesce_sample(int on)
{
    flush_all_queues();
    return g_coalesce_sample.exchange(on != 0 ? 1 : 0);
}

int smartgpu_coalesce_sample_grid(int workgroups)
{
    if (workgroups < 0 || workgroups > 65536) { set_error("coalesce_sample_grid: 1..65536 workgroups (0: one per compute unit), not %d", workgroups); return SMARTGPU_ERR_ARG; }
    flush_all_queues();
    return g_sample_grid.exchange(workgroups);
}

int smartgpu_coalesce_sampled(int device, uint64_t* passes)
{
    if (device < 0 || device >= kMaxDevices || !passes) { set_error("bad coalesce_sampled arguments (device %d)", device); return SMARTGPU_ERR_ARG; }
    std::lock_guard<std::mutex> lock(g_queue[device].mu);
    *passes = g_queue[device].sampled;
    return SMARTGPU_OK;
}

long long smartgpu_text_sampling(long long min_bytes)
{
    if (min_bytes < -1) { set_error("text_sampling: the least text that gets a sample has 0 or more bytes (-1: none gets one), not %lld", min_bytes); return SMARTGPU_ERR_ARG; }
    return g_text_sampling.exchange(min_bytes);
}

int smartgpu_text_has_sample(const smartgpu_text* t) { return t && t->sample ? 1 : 0; }

int smartgpu_coalesce_riders(int device, uint64_t* riders)
{
    if (device < 0 || device >= kMaxDevices || !riders) { set_error("bad coalesce_riders arguments (device %d)", device); return SMARTGPU_ERR_ARG; }
    std::lock_guard<std::mutex> lock(g_queue[device].mu);
    *riders = g_queue[device].riders;
    return SMARTGPU_OK;
}

void* smartgpu_stream_handle(int device)
{
    DeviceCtx* d = device_ctx_flushed(device);
    if (!d) return nullptr;
    {   // whoever holds the stream orders their own work on it: from here on every launch on this device is sent at once
        std::lock_guard<std::mutex> lock(g_queue[d->device].mu);
        g_queue[d->device].off = true;
    }
    return static_cast<void*>(d->stream);
}

/* ---- one-shot searches ------------------------------------------------- */
int smartgpu_search64(int algo, const uint8_t* P, uint32_t m, const smartgpu_text* text,
                      uint64_t off, uint64_t n, uint64_t* count, double* pre_ms, double* run_ms)
{
    const int rc = check_search_args(algo, P, m, text, off, n);
    if (rc != SMARTGPU_OK) return rc;
    // a pattern set of one: tables through the device's arena and staging buffer (no allocation per call — a plan's
    // two hipMalloc and its memset were most of the 25-30 us a call cost around a 3 us kernel), one launch, one read-back
    const uint8_t* set[1] = {P};
    uint64_t c = 0;
    double pre = 0.0, wall = 0.0;
    const int r = smartgpu_search_batch64(algo, set, m, 1, text, off, n, &c, &pre, nullptr, &wall);
    if (r != SMARTGPU_OK) return r;
    g_last_pre_ms = pre;
    g_last_run_ms = wall;  // launch -> count on host, the run_time analogue (main.h:29,31)
    if (count) *count = c;
    if (pre_ms) *pre_ms = pre;
    if (run_ms) *run_ms = wall;
    return SMARTGPU_OK;
}

/* ---- a whole pattern set per call (the harness loop, src/smart.c:312-345) ------------- */
}  // extern "C"

// (host_ctx.hpp) make sure the device's batch arena holds `blob_bytes` of tables and `k` counts
bool batch_reserve(DeviceCtx* d, size_t blob_bytes, size_t k)
{
    if (blob_bytes > d->arena_bytes) {
        if (d->arena) (void)hipFree(d->arena);
        d->arena = nullptr;
        d->arena_bytes = 0;
        const size_t want = std::max(blob_bytes + blob_bytes / 4, size_t(8) << 20);
        if (hipMalloc(reinterpret_cast<void**>(&d->arena), want) != hipSuccess) { set_error("batch arena: hipMalloc of %zu bytes failed", want); return false; }
        d->arena_bytes = want;
    }
    if (k > d->batch_slots) {
        if (d->batch_counts) (void)hipFree(d->batch_counts);
        if (d->pinned_counts) (void)hipHostFree(d->pinned_counts);
        d->batch_counts = nullptr;
        d->pinned_counts = nullptr;
        d->batch_slots = 0;
        const size_t want = std::max<size_t>(k, 1024);
        if (hipMalloc(reinterpret_cast<void**>(&d->batch_counts), want * 8) != hipSuccess ||
            hipHostMalloc(reinterpret_cast<void**>(&d->pinned_counts), want * 8, hipHostMallocDefault) != hipSuccess) {
            set_error("batch counts: allocation of %zu slots failed", want);
            return false;
        }
        d->batch_slots = want;
    }
    return true;
}

// (host_ctx.hpp) the device buffer of `cap` positions for a find
unsigned long long* find_reserve(DeviceCtx* d, uint64_t cap, bool* own)
{
    *own = false;
    if (cap <= d->find_out_cap) return d->find_out;
    unsigned long long* out = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&out), cap * sizeof(unsigned long long)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("pfind: cannot allocate %llu positions on the device", (unsigned long long)cap);
        return nullptr;
    }
    if (cap > kFindKeep) {
        *own = true;
        return out;
    }
    if (d->find_out) (void)hipFree(d->find_out);  // (idle: every find ends with a synchronisation of the device's stream)
    d->find_out = out;
    d->find_out_cap = static_cast<size_t>(cap);
    return out;
}

// (host_ctx.hpp) positions from the device to the caller's memory through the pinned staging buffer
bool copy_positions(DeviceCtx* d, uint64_t* dst, const unsigned long long* src, uint64_t count)
{
    for (uint64_t done = 0; done < count;) {
        const uint64_t part = std::min<uint64_t>(count - done, d->pinned_bytes / 8);
        if (hipMemcpyAsync(d->pinned, src + done, part * 8, hipMemcpyDeviceToHost, d->stream) != hipSuccess ||
            hipStreamSynchronize(d->stream) != hipSuccess)
            return false;
        std::memcpy(dst + done, d->pinned, part * 8);
        done += part;
    }
    return true;
}

namespace {

struct BatchPlan { sg::PlanWords words; size_t off; };  // off: the blob inside the arena
// the staging buffer of a set of K patterns: [table blobs ...][K argument records][K launch-order indices]
size_t batch_tail_offset(const DeviceCtx* d, uint32_t K)
{
    return (d->pinned_bytes - static_cast<size_t>(K) * (4 + sizeof(sg::BatchItem))) & ~size_t(63);
}
constexpr uint64_t kOneGridMaxText = 32ull << 20;  // pattern sets over texts up to this size run as ONE grid per kernel
constexpr uint32_t kOneGridMaxY = 65535;            // HIP's limit on gridDim.y: patterns per grid of the one-grid form
constexpr uint32_t kBatchMaxPatterns = 1u << 18;    // per call (argument records and launch order of a set sit in the staging buffer's tail: 9 of its 32 MB)

// Build the K blobs on the host ONCE and place them in the arena of every device of `ds` (one device: a plain pattern
// set; several: the shards of a multi-GPU text — VERDICT r3: the tables of a set were rebuilt per device, 8x the
// preprocessing at 8 GPUs).  pre_ms[k] = host table construction of pattern k + its share of the uploads.
// plans[k].off = offset of blob k in the arenas (the same in each).  The blobs are staged in ds[0]'s pinned buffer and
// copied from there to every arena, each copy on its device's own stream.
int batch_upload(const std::vector<DeviceCtx*>& ds, int algo, const uint8_t* const* P, uint32_t m, uint32_t K, std::vector<BatchPlan>& plans,
                 double* pre_ms)
{
    static thread_local std::vector<uint8_t> blob;  // one buffer for every pattern of every set
    DeviceCtx* const d0 = ds[0];
    std::vector<double> host_ms(K, 0.0);
    plans.resize(K);
    // the blobs of one algorithm and one length are equally long (multiples of 256): size the arena from the first
    if (!P[0]) { set_error("pattern 0 is NULL"); return SMARTGPU_ERR_ARG; }
    plans[0].words = sg::build_blob(blob, algo, P[0], m);
    const size_t room = batch_tail_offset(d0, K);  // the tail of the staging buffer holds the set's argument records and launch order
    if (blob.size() > room) { set_error("a table blob of %zu bytes exceeds the staging buffer", blob.size()); return SMARTGPU_ERR_NOMEM; }
    size_t arena_min = 0;
    for (DeviceCtx* d : ds) {
        if (d->device != d0->device) HIP_TRY(hipSetDevice(d->device), return SMARTGPU_ERR_HIP);
        if (!batch_reserve(d, (blob.size() + 4096) * K + 256 + K * sizeof(sg::BatchItem), K)) return SMARTGPU_ERR_NOMEM;
        arena_min = arena_min ? std::min(arena_min, d->arena_bytes) : d->arena_bytes;
    }
    double up_total = 0.0;
    size_t total = 0, fill = 0, fill_off = 0;  // staging holds `fill` bytes that belong at arena offset fill_off
    // the copy is waited for only where the staging buffer is filled again in this call: the launches that follow are
    // ordered behind it on each device's stream, and every caller ends with a synchronisation before the buffer is reused
    auto flush = [&](bool more) -> bool {
        if (!fill) return true;
        const double t_up = now_ms();
        bool ok = true;
        for (DeviceCtx* d : ds) {
            if (ds.size() > 1) ok = ok && hipSetDevice(d->device) == hipSuccess;
            ok = ok && hipMemcpyAsync(d->arena + fill_off, d0->pinned, fill, hipMemcpyHostToDevice, d->stream) == hipSuccess;
        }
        if (more || ds.size() > 1)  // several devices read ONE staging buffer: all done before the caller's own use of it
            for (DeviceCtx* d : ds) ok = ok && hipStreamSynchronize(d->stream) == hipSuccess;
        up_total += now_ms() - t_up;
        fill_off += fill;
        fill = 0;
        return ok;
    };
    for (uint32_t k = 0; k < K; ++k) {
        if (!P[k]) { set_error("pattern %u is NULL", k); return SMARTGPU_ERR_ARG; }
        const double t0 = now_ms();
        if (k) plans[k].words = sg::build_blob(blob, algo, P[k], m);
        if (total + blob.size() + 256 + K * sizeof(sg::BatchItem) > arena_min) {  // rerouted patterns carry masks the first did not
            set_error("batch: the table arena (%zu bytes) is too small for this pattern set", arena_min);
            return SMARTGPU_ERR_NOMEM;
        }
        if (fill + blob.size() > room && !flush(true)) { set_error("batch: table upload failed (%s)", hipGetErrorString(hipGetLastError())); return SMARTGPU_ERR_HIP; }
        std::memcpy(d0->pinned + fill, blob.data(), blob.size());  // straight into the staging buffer
        fill += blob.size();
        plans[k].off = total;
        total += blob.size();  // multiples of 256
        host_ms[k] = now_ms() - t0;
    }
    if (!flush(false)) { set_error("batch: table upload failed (%s)", hipGetErrorString(hipGetLastError())); return SMARTGPU_ERR_HIP; }
    if (ds.size() > 1) HIP_TRY(hipSetDevice(d0->device), return SMARTGPU_ERR_HIP);
    const double up_ms = up_total / K;
    if (pre_ms)
        for (uint32_t k = 0; k < K; ++k) pre_ms[k] = host_ms[k] + up_ms;
    return SMARTGPU_OK;
}

// Enqueue the searches of a pattern set on the device's stream; counts go to d->batch_counts[0..K).
// Small texts (SMART's stock 1 MiB: a search is 64 workgroups and 3 us, less than its launch costs the host):
// the set runs as ONE grid per kernel, gridDim.y = patterns (sg::launch_scan_set) — the per-pattern arguments
// go up as one array behind the tables; patterns are grouped by the kernel and grid their plans choose.
// Larger texts: K launches back to back (each fills the chip on its own), with one HIP event per pattern
// if per-pattern device times are wanted.  run_ms (or NULL): device time per pattern; in the one-grid form
// a group's time divided by its patterns.
int batch_enqueue(DeviceCtx* d, int algo, const std::vector<BatchPlan>& plans, uint32_t m, const smartgpu_text* text,
                  uint64_t off, uint64_t n, uint32_t K, bool timed, std::vector<std::pair<uint32_t, uint32_t>>* groups_out,
                  bool each = false)  // each: one launch per pattern whatever the text's size (smartgpu_search_batch64_each)
{
    HIP_TRY(hipMemsetAsync(d->batch_counts, 0, static_cast<size_t>(K) * 8, d->stream), return SMARTGPU_ERR_HIP);
    if (timed)
        while (d->batch_events.size() < static_cast<size_t>(K) + 1) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e), return SMARTGPU_ERR_HIP);
            d->batch_events.push_back(e);
        }
    if (groups_out) groups_out->clear();
    if (n > kOneGridMaxText || K == 1 || each) {
        if (timed) HIP_TRY(hipEventRecord(d->batch_events[0], d->stream), return SMARTGPU_ERR_HIP);
        for (uint32_t k = 0; k < K; ++k) {
            const sg::ScanArgs a = make_args(plans[k].words, m, d->arena + plans[k].off, d->batch_counts + k, text, off, n);
            HIP_TRY(sg::launch_scan(algo, a, d->num_cus, d->stream, text->codes()), return SMARTGPU_ERR_HIP);
            if (timed) HIP_TRY(hipEventRecord(d->batch_events[k + 1], d->stream), return SMARTGPU_ERR_HIP);
            if (groups_out) groups_out->push_back({k, 1u});
        }
        return SMARTGPU_OK;
    }
    // one grid per group of patterns whose plans lead to the same kernel, template arguments and grid: sg::group_key (launch.hip)
    std::vector<uint64_t> key(K);
    std::vector<uint32_t> order(K);
    for (uint32_t k = 0; k < K; ++k) {
        key[k] = sg::group_key(algo, m, plans[k].words, text->codes());
        order[k] = k;
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
    // (in the staging buffer's tail: its front may still be on its way to the arena — batch_upload does not wait)
    sg::BatchItem* host_items = reinterpret_cast<sg::BatchItem*>(d->pinned + batch_tail_offset(d, K));
    for (uint32_t i = 0; i < K; ++i) {
        const BatchPlan& bp = plans[order[i]];
        const sg::ScanArgs pa = sg::prepare_scan_args(algo, make_args(bp.words, m, d->arena, d->batch_counts, text, off, n));
        host_items[i] = sg::BatchItem{bp.off, order[i], pa.halo, pa.fp_off, pa.prefer_packed, pa.sparse, pa.so_off};
    }
    sg::BatchItem* dev_items = reinterpret_cast<sg::BatchItem*>(d->arena + d->arena_bytes - ((static_cast<size_t>(K) * sizeof(sg::BatchItem) + 255) & ~size_t(255)));
    HIP_TRY(hipMemcpyAsync(dev_items, host_items, static_cast<size_t>(K) * sizeof(sg::BatchItem), hipMemcpyHostToDevice, d->stream),
            return SMARTGPU_ERR_HIP);
    uint32_t ev = 0;
    if (timed) HIP_TRY(hipEventRecord(d->batch_events[ev++], d->stream), return SMARTGPU_ERR_HIP);
    for (uint32_t i = 0; i < K;) {
        uint32_t j = i;
        while (j < K && key[order[j]] == key[order[i]]) ++j;
        // the set's common arguments: blob = arena base, count = first slot (the items add their own), and the
        // group's plan fields, which choose kernel and grid
        const sg::ScanArgs first = make_args(plans[order[i]].words, m, d->arena, d->batch_counts, text, off, n);
        // gridDim.y holds at most 65535: a larger group goes as several grids over slices of its items
        for (uint32_t lo = i; lo < j; lo += kOneGridMaxY)
            HIP_TRY(sg::launch_scan_set(algo, first, dev_items + lo, std::min(kOneGridMaxY, j - lo), d->num_cus, d->stream, text->codes()), return SMARTGPU_ERR_HIP);
        if (timed) HIP_TRY(hipEventRecord(d->batch_events[ev++], d->stream), return SMARTGPU_ERR_HIP);
        if (groups_out) groups_out->push_back({i, j - i});
        i = j;
    }
    // groups_out indexes the sorted order; remember it for the caller through the pinned array's tail
    if (groups_out) {
        uint32_t* ord = reinterpret_cast<uint32_t*>(d->pinned + d->pinned_bytes - static_cast<size_t>(K) * 4);
        for (uint32_t i = 0; i < K; ++i) ord[i] = order[i];
    }
    return SMARTGPU_OK;
}

}  // namespace

extern "C" {

static int search_batch_impl(int algo, const uint8_t* const* P, uint32_t m, uint32_t K, const smartgpu_text* text,
                             uint64_t off, uint64_t n, uint64_t* counts, double* pre_ms, double* run_ms, double* batch_ms, bool each)
{
    if (!P || K < 1 || !counts) { set_error("batch: P/counts NULL or K = 0"); return SMARTGPU_ERR_ARG; }
    if (K > kBatchMaxPatterns) { set_error("batch: %u patterns in one set (at most %u)", K, kBatchMaxPatterns); return SMARTGPU_ERR_ARG; }
    const int rc = check_search_args(algo, P[0], m, text, off, n);
    if (rc != SMARTGPU_OK) return rc;
    DeviceCtx* d = device_ctx_flushed(text->device);
    if (!d) return SMARTGPU_ERR_HIP;
    std::vector<BatchPlan> plans;
    const int up = batch_upload({d}, algo, P, m, K, plans, pre_ms);  // preprocessing phase
    if (up != SMARTGPU_OK) return up;
    const bool timed = run_ms != nullptr;
    // searching phase: the set's launches, one read-back
    std::vector<std::pair<uint32_t, uint32_t>> groups;
    const double t0 = now_ms();
    const int eq = batch_enqueue(d, algo, plans, m, text, off, n, K, timed, &groups, each);
    if (eq != SMARTGPU_OK) return eq;
    HIP_TRY(hipMemcpyAsync(d->pinned_counts, d->batch_counts, static_cast<size_t>(K) * 8, hipMemcpyDeviceToHost, d->stream),
            return SMARTGPU_ERR_HIP);
    HIP_TRY(hipStreamSynchronize(d->stream), return SMARTGPU_ERR_HIP);
    const double wall = now_ms() - t0;
    for (uint32_t k = 0; k < K; ++k) {
        if (count_poisoned(d->pinned_counts[k])) return SMARTGPU_ERR_HIP;
        counts[k] = d->pinned_counts[k];
    }
    if (timed) {
        const bool one_grid = !(n > kOneGridMaxText || K == 1 || each);
        const uint32_t* ord = reinterpret_cast<const uint32_t*>(d->pinned + d->pinned_bytes - static_cast<size_t>(K) * 4);
        for (size_t g = 0; g < groups.size(); ++g) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, d->batch_events[g], d->batch_events[g + 1]), return SMARTGPU_ERR_HIP);
            for (uint32_t i = groups[g].first; i < groups[g].first + groups[g].second; ++i)
                run_ms[one_grid ? ord[i] : i] = ms / groups[g].second;
        }
    }
    if (batch_ms) *batch_ms = wall;
    g_last_pre_ms = pre_ms ? pre_ms[K - 1] : 0.0;
    g_last_run_ms = wall / K;
    return SMARTGPU_OK;
}

int smartgpu_search_batch64(int algo, const uint8_t* const* P, uint32_t m, uint32_t K, const smartgpu_text* text,
                            uint64_t off, uint64_t n, uint64_t* counts, double* pre_ms, double* run_ms, double* batch_ms)
{
    return search_batch_impl(algo, P, m, K, text, off, n, counts, pre_ms, run_ms, batch_ms, false);
}

int smartgpu_search_batch64_each(int algo, const uint8_t* const* P, uint32_t m, uint32_t K, const smartgpu_text* text,
                                 uint64_t off, uint64_t n, uint64_t* counts, double* pre_ms, double* run_ms, double* batch_ms)
{
    return search_batch_impl(algo, P, m, K, text, off, n, counts, pre_ms, run_ms, batch_ms, true);
}

/* ---- occurrence positions ------------------------------------------------- */
int smartgpu_find64(const uint8_t* P, uint32_t m, const smartgpu_text* text, uint64_t off, uint64_t n,
                    uint64_t* positions, uint64_t cap, uint64_t* count)
{
    const int rc = check_search_args(SMARTGPU_EPSM, P, m, text, off, n);
    if (rc != SMARTGPU_OK) return rc;
    if (!count || (cap && !positions)) { set_error("find64: count/positions must not be NULL"); return SMARTGPU_ERR_ARG; }
    DeviceCtx* d = device_ctx_flushed(text->device);
    if (!d) return SMARTGPU_ERR_HIP;
    smartgpu_plan* p = smartgpu_plan_create(SMARTGPU_EPSM, P, m, text->device);
    if (!p) return SMARTGPU_ERR_HIP;
    unsigned long long* out = nullptr;
    int r = SMARTGPU_OK;
    if (cap && hipMalloc(reinterpret_cast<void**>(&out), cap * sizeof(unsigned long long)) != hipSuccess) {
        set_error("find64: cannot allocate %llu positions on the device", (unsigned long long)cap);
        r = SMARTGPU_ERR_NOMEM;
    }
    unsigned long long total = 0;
    if (r == SMARTGPU_OK) {
        sg::ScanArgs a = make_args(p->words, p->m, p->blob, p->slot_ptr(0), text, off, n);
        a.fp_off = sg::kTableOff;  // EPSM blob: the fingerprint follows the pattern slot
        bool ok = hipMemsetAsync(a.count, 0, sizeof(unsigned long long), d->stream) == hipSuccess &&
                  sg::launch_find(a, out, cap, d->num_cus, d->stream) == hipSuccess &&
                  hipMemcpyAsync(d->pinned_count, a.count, sizeof(unsigned long long), hipMemcpyDeviceToHost, d->stream) == hipSuccess &&
                  hipStreamSynchronize(d->stream) == hipSuccess;
        if (ok) {
            total = *d->pinned_count;
            const unsigned long long have = total < cap ? total : cap;
            if (have) ok = hipMemcpy(positions, out, have * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess;
            if (ok && have) std::sort(positions, positions + have);  // waves append in no particular order
        }
        if (!ok) {
            set_error("find64: %s", hipGetErrorString(hipGetLastError()));
            r = SMARTGPU_ERR_HIP;
        }
    }
    if (out) (void)hipFree(out);
    smartgpu_plan_free(p);
    if (r != SMARTGPU_OK) return r;
    *count = total;
    if (total > cap) { set_error("find64: %llu occurrences, room for %llu", total, (unsigned long long)cap); return SMARTGPU_ERR_NOMEM; }
    return SMARTGPU_OK;
}

void smartgpu_last_times(double* pre_ms, double* run_ms)
{
    if (pre_ms) *pre_ms = g_last_pre_ms;
    if (run_ms) *run_ms = g_last_run_ms;
}

static int search_host(int algo, const unsigned char* P, int m, const unsigned char* T, int n)
{
    if (!P || !T || m < 1 || n < 0) return SMARTGPU_NA;
    if (m > SMARTGPU_XSIZE) return SMARTGPU_NA;
    smartgpu_text* t = text_upload_impl(T, static_cast<uint64_t>(n), 0, false);  // searched once: no alphabet pass
    if (!t) return SMARTGPU_NA;
    uint64_t c = 0;
    const int rc = smartgpu_search64(algo, P, static_cast<uint32_t>(m), t, 0, static_cast<uint64_t>(n), &c, nullptr, nullptr);
    smartgpu_text_free(t);
    if (rc != SMARTGPU_OK || c > 0x7FFFFFFFull) return SMARTGPU_NA;
    return static_cast<int>(c);
}

int smartgpu_hor_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_HOR, P, m, T, n); }
int smartgpu_bm_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_BM, P, m, T, n); }
int smartgpu_kmp_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_KMP, P, m, T, n); }
int smartgpu_so_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_SO, P, m, T, n); }
int smartgpu_bndm_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_BNDM, P, m, T, n); }
int smartgpu_epsm_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_EPSM, P, m, T, n); }
int smartgpu_sa_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_SA, P, m, T, n); }
int smartgpu_qs_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_QS, P, m, T, n); }
int smartgpu_tunedbm_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_TUNEDBM, P, m, T, n); }
int smartgpu_raita_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_RAITA, P, m, T, n); }
int smartgpu_hash3_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_HASH3, P, m, T, n); }
int smartgpu_hash5_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_HASH5, P, m, T, n); }
int smartgpu_hash8_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_HASH8, P, m, T, n); }
int smartgpu_sbndm_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_SBNDM, P, m, T, n); }
int smartgpu_kr_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_KR, P, m, T, n); }
int smartgpu_bndml_search(const unsigned char* P, int m, const unsigned char* T, int n) { return search_host(SMARTGPU_BNDML, P, m, T, n); }

/* ---- one process, several GPUs ------------------------------------------ */
}  // extern "C"

namespace {

// RCCL is loaded on first use (dlopen), so the library itself has no link-time
// dependency on it; only the multi-GPU reduce needs it.  Signatures, ncclUint64 and ncclSum
// come from <rccl/rccl.h>: an ABI change there is a compile error here, not a silent miscount.
struct Rccl {
    void* lib = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    bool load()
    {
        if (lib) return true;
        // (HSA_ENABLE_IPC_MODE_LEGACY=0 — dmabuf IPC, the only mode this pool's driver supports — is an HSA runtime
        // flag read at hsa_init: set by this library's constructor below, before any HIP call of the process can be ours)
        lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!lib) { set_error("cannot load librccl.so: %s", dlerror()); return false; }
        CommInitAll = reinterpret_cast<decltype(CommInitAll)>(dlsym(lib, "ncclCommInitAll"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
        AllReduce = reinterpret_cast<decltype(AllReduce)>(dlsym(lib, "ncclAllReduce"));
        GroupStart = reinterpret_cast<decltype(GroupStart)>(dlsym(lib, "ncclGroupStart"));
        GroupEnd = reinterpret_cast<decltype(GroupEnd)>(dlsym(lib, "ncclGroupEnd"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
        if (!CommInitAll || !CommDestroy || !AllReduce || !GroupStart || !GroupEnd || !GetErrorString) {
            set_error("librccl.so lacks an expected symbol");
            return false;
        }
        return true;
    }
};
Rccl g_rccl;

// Runs when the library is loaded, i.e. before its first HIP call: ROCr reads the flag when it initialises (hsa_init,
// on the process's first HIP call).  A process that initialised HIP before loading this library has to set it itself
// (bench.py and host/smart.c do so at entry); an explicit setting in the environment is never overridden.
__attribute__((constructor)) void smartgpu_set_ipc_mode() { setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0); }

}  // namespace

struct smartgpu_mtext {
    uint64_t n = 0;
    std::vector<int> devices;
    std::vector<smartgpu_text*> shards;   // shard g = bytes [begin[g], begin[g+1] + overlap)
    std::vector<uint64_t> begin;          // k+1 entries, start-position ownership
    std::vector<ncclComm_t> comms;        // RCCL communicators, created on first RCCL reduce
};

namespace {

// first byte shard g of k owns (the shards' sizes differ by at most one byte; g = k: n)
uint64_t shard_begin(uint64_t n, int k, int g) { return n / k * g + std::min<uint64_t>(g, n % k); }

smartgpu_mtext* mtext_new(uint64_t n, int ngpus, const int* devices)
{
    if (ngpus < 1 || ngpus > kMaxDevices) { set_error("ngpus %d outside [1,%d]", ngpus, kMaxDevices); return nullptr; }
    smartgpu_mtext* t = new smartgpu_mtext;
    t->n = n;
    for (int g = 0; g < ngpus; ++g) t->devices.push_back(devices ? devices[g] : g);
    for (int g = 0; g <= ngpus; ++g) t->begin.push_back(shard_begin(n, ngpus, g));
    return t;
}

// bytes shard g has to hold: its own starts plus XSIZE-1 bytes of the next shards
void shard_span(const smartgpu_mtext* t, int g, uint64_t* off, uint64_t* len)
{
    uint64_t own = 0;
    (void)smartgpu_mtext_partition(t->n, static_cast<int>(t->devices.size()), g, off, &own, len);
}

// k-1 parked host threads, one per further device of a multi-GPU search: the caller enqueues device 0's shard itself
// while worker g enqueues device g's (one host thread enqueued the k devices' launches one after the other —
// with one pattern on 128 MiB shards, a 28 us kernel, the launch latency of eight devices in a row was the bound).
// The threads are created on the first multi-GPU search and parked on a condition variable between calls.
class LaunchPool {
public:
    // fn(g) for g = 0 .. k-1: g = 0 on the calling thread, the others on the workers; returns when all are done
    void run(int k, const std::function<void(int)>& fn)
    {
        if (k <= 1) { if (k == 1) fn(0); return; }
        {
            std::unique_lock<std::mutex> lk(mu_);
            while (static_cast<int>(workers_.size()) < k - 1) {
                const int idx = static_cast<int>(workers_.size()) + 1;
                workers_.emplace_back([this, idx] { loop(idx); });
            }
            job_ = &fn;
            active_ = k;
            pending_ = k - 1;
            ++gen_;
        }
        go_.notify_all();
        fn(0);
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return pending_ == 0; });
        job_ = nullptr;
    }
    ~LaunchPool()
    {
        {
            std::unique_lock<std::mutex> lk(mu_);
            stop_ = true;
        }
        go_.notify_all();
        for (std::thread& t : workers_) t.join();
    }

private:
    void loop(int idx)
    {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int)>* job = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu_);
                go_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                if (idx < active_) job = job_;
            }
            if (!job) continue;  // this call uses fewer devices than there are workers
            (*job)(idx);
            std::unique_lock<std::mutex> lk(mu_);
            if (--pending_ == 0) done_.notify_one();
        }
    }
    std::mutex mu_;
    std::condition_variable go_, done_;
    std::vector<std::thread> workers_;
    const std::function<void(int)>* job_ = nullptr;
    uint64_t gen_ = 0;
    int active_ = 0, pending_ = 0;
    bool stop_ = false;
};
LaunchPool g_pool;

}  // namespace

extern "C" {

smartgpu_mtext* smartgpu_mtext_upload(const void* host, uint64_t n, int ngpus, const int* devices)
{
    if (!host && n) { set_error("host pointer is NULL"); return nullptr; }
    smartgpu_mtext* t = mtext_new(n, ngpus, devices);
    if (!t) return nullptr;
    for (int g = 0; g < ngpus; ++g) {
        uint64_t off, len;
        shard_span(t, g, &off, &len);
        smartgpu_text* s = smartgpu_text_upload(static_cast<const uint8_t*>(host) + off, len, t->devices[g]);
        if (!s) { smartgpu_mtext_free(t); return nullptr; }
        t->shards.push_back(s);
    }
    return t;
}

smartgpu_mtext* smartgpu_mtext_generate(uint64_t seed, int sigma, uint64_t n, int ngpus, const int* devices)
{
    smartgpu_mtext* t = mtext_new(n, ngpus, devices);
    if (!t) return nullptr;
    for (int g = 0; g < ngpus; ++g) {
        uint64_t off, len;
        shard_span(t, g, &off, &len);
        smartgpu_text* s = smartgpu_text_generate(seed, sigma, off, len, t->devices[g]);
        if (!s) { smartgpu_mtext_free(t); return nullptr; }
        t->shards.push_back(s);
    }
    return t;
}

void smartgpu_mtext_free(smartgpu_mtext* t)
{
    if (!t) return;
    for (smartgpu_text* s : t->shards) smartgpu_text_free(s);
    for (ncclComm_t c : t->comms)
        if (c && g_rccl.CommDestroy) g_rccl.CommDestroy(c);
    delete t;
}

uint64_t smartgpu_mtext_length(const smartgpu_mtext* t) { return t ? t->n : 0; }
int smartgpu_mtext_ngpus(const smartgpu_mtext* t) { return t ? static_cast<int>(t->devices.size()) : 0; }

int smartgpu_mtext_partition(uint64_t n, int ngpus, int g, uint64_t* begin, uint64_t* own, uint64_t* held)
{
    if (ngpus < 1 || ngpus > kMaxDevices || g < 0 || g >= ngpus) { set_error("partition: shard %d of %d", g, ngpus); return SMARTGPU_ERR_ARG; }
    const uint64_t b = shard_begin(n, ngpus, g), e = shard_begin(n, ngpus, g + 1);
    if (begin) *begin = b;
    if (own) *own = e - b;
    if (held) *held = std::min<uint64_t>(n, e + SMARTGPU_XSIZE - 1) - b;
    return SMARTGPU_OK;
}

int smartgpu_selftest_launch_pool(int k, int rounds)
{
    // every round: fn(g) adds g + 1 into a slot of its own and into a shared atomic; checks that each g in 0..k-1 ran
    // exactly once per round, whatever k was in the round before (the pool keeps its workers between calls)
    if (k < 1 || k > kMaxDevices || rounds < 1) { set_error("selftest: k %d, rounds %d", k, rounds); return SMARTGPU_ERR_ARG; }
    for (int r = 0; r < rounds; ++r) {
        const int kk = 1 + (r * 7 + k - 1) % k;  // varies between 1 and k
        std::vector<int> ran(kk, 0);
        std::atomic<long> sum{0};
        g_pool.run(kk, [&](int g) { ++ran[g]; sum += g + 1; });
        long want = 0;
        for (int g = 0; g < kk; ++g) {
            want += g + 1;
            if (ran[g] != 1) { set_error("selftest: job %d of %d ran %d times in round %d", g, kk, ran[g], r); return SMARTGPU_ERR_HIP; }
        }
        if (sum != want) { set_error("selftest: sum %ld, want %ld", sum.load(), want); return SMARTGPU_ERR_HIP; }
    }
    return SMARTGPU_OK;
}

int smartgpu_msearch_batch64(int algo, const uint8_t* const* P, uint32_t m, uint32_t K, smartgpu_mtext* text, int reduce,
                             uint64_t* counts, double* pre_ms, double* batch_ms)
{
    if (!text) { set_error("text handle is NULL"); return SMARTGPU_ERR_ARG; }
    if (!P || K < 1 || !counts || !P[0]) { set_error("batch: P/counts NULL or K = 0"); return SMARTGPU_ERR_ARG; }
    if (K > kBatchMaxPatterns) { set_error("batch: %u patterns in one set (at most %u)", K, kBatchMaxPatterns); return SMARTGPU_ERR_ARG; }
    const int rc_p = check_pattern(algo, P[0], m);
    if (rc_p != SMARTGPU_OK) return rc_p;
    const int k = static_cast<int>(text->devices.size());
    // preprocessing: the K tables are built ONCE on the host and copied to the arena of every (distinct) device
    std::vector<BatchPlan> plans;
    std::vector<DeviceCtx*> ctx(k, nullptr), uniq;
    for (int g = 0; g < k; ++g) {
        ctx[g] = device_ctx_flushed(text->devices[g]);
        if (!ctx[g]) return SMARTGPU_ERR_HIP;
        if (std::find(uniq.begin(), uniq.end(), ctx[g]) == uniq.end()) uniq.push_back(ctx[g]);
    }
    const int up = batch_upload(uniq, algo, P, m, K, plans, pre_ms);
    if (up != SMARTGPU_OK) return up;
    const bool distinct = reduce == SMARTGPU_REDUCE_RCCL;
    if (distinct && static_cast<int>(uniq.size()) != k) { set_error("RCCL reduce: the %d devices of the text must be distinct", k); return SMARTGPU_ERR_ARG; }
    if (distinct && text->comms.empty()) {
        if (!g_rccl.load()) return SMARTGPU_ERR_HIP;
        text->comms.assign(k, nullptr);
        const ncclResult_t st = g_rccl.CommInitAll(text->comms.data(), k, text->devices.data());
        if (st != ncclSuccess) {
            set_error("ncclCommInitAll over %d devices failed: %s (devices must be distinct)", k, g_rccl.GetErrorString(st));
            text->comms.clear();
            return SMARTGPU_ERR_HIP;
        }
    }
    // searching: every shard on its own device / stream, concurrently; the same device listed twice (host reduce,
    // the one-GPU test of the shard arithmetic) shares one arena, so its shards take turns
    const double t_run = now_ms();
    std::vector<uint64_t> total(K, 0);
    auto launch_shard = [&](int g) -> int {
        DeviceCtx* d = ctx[g];
        HIP_TRY(hipSetDevice(text->devices[g]), return SMARTGPU_ERR_HIP);
        // shard g counts the starts it owns: its first (begin[g+1]-begin[g]) positions
        const uint64_t own = text->begin[g + 1] - text->begin[g];
        const uint64_t have = smartgpu_text_length(text->shards[g]);
        const uint64_t span = std::min<uint64_t>(have, own + m - 1);
        return batch_enqueue(d, algo, plans, m, text->shards[g], 0, span, K, false, nullptr);
    };
    int rc = SMARTGPU_OK;
    if (distinct) {
        // the k devices' launches are enqueued by k host threads at once (LaunchPool): each sets its device, enqueues the
        // memset and the kernel(s) of its shard; an error text travels back from the worker's thread-local slot
        std::vector<int> rcs(k, SMARTGPU_OK);
        std::vector<std::string> errs(k);
        g_pool.run(k, [&](int g) {
            rcs[g] = launch_shard(g);
            if (rcs[g] != SMARTGPU_OK) errs[g] = g_error;
        });
        for (int g = 0; g < k; ++g)
            if (rcs[g] != SMARTGPU_OK) { g_error = errs[g]; return rcs[g]; }
        // ONE collective for the whole pattern set: the K counts of every device, summed in place
        ncclResult_t st = g_rccl.GroupStart();
        for (int g = 0; g < k && st == ncclSuccess; ++g)
            st = g_rccl.AllReduce(ctx[g]->batch_counts, ctx[g]->batch_counts, K, ncclUint64, ncclSum, text->comms[g], ctx[g]->stream);
        const ncclResult_t end = g_rccl.GroupEnd();
        if (st == ncclSuccess) st = end;
        if (st != ncclSuccess) { set_error("RCCL all-reduce of %u counts over %d devices failed: %s", K, k, g_rccl.GetErrorString(st)); return SMARTGPU_ERR_HIP; }
        HIP_TRY(hipSetDevice(text->devices[0]), return SMARTGPU_ERR_HIP);
        HIP_TRY(hipMemcpyAsync(ctx[0]->pinned_counts, ctx[0]->batch_counts, static_cast<size_t>(K) * 8, hipMemcpyDeviceToHost, ctx[0]->stream),
                return SMARTGPU_ERR_HIP);
        HIP_TRY(hipStreamSynchronize(ctx[0]->stream), return SMARTGPU_ERR_HIP);
        for (uint32_t j = 0; j < K; ++j) total[j] = ctx[0]->pinned_counts[j];
        for (int g = 1; g < k; ++g) smartgpu_device_sync(text->devices[g]);
        for (uint32_t j = 0; j < K; ++j)
            if (count_poisoned(total[j])) return SMARTGPU_ERR_HIP;  // (a sum of at most 16 shards: still below 2^63)
    } else {
        for (int g = 0; g < k; ++g) {  // K-count read-backs added on the host
            rc = launch_shard(g);
            if (rc != SMARTGPU_OK) return rc;
            DeviceCtx* d = ctx[g];
            HIP_TRY(hipMemcpyAsync(d->pinned_counts, d->batch_counts, static_cast<size_t>(K) * 8, hipMemcpyDeviceToHost, d->stream),
                    return SMARTGPU_ERR_HIP);
            HIP_TRY(hipStreamSynchronize(d->stream), return SMARTGPU_ERR_HIP);
            for (uint32_t j = 0; j < K; ++j) {
                if (count_poisoned(d->pinned_counts[j])) return SMARTGPU_ERR_HIP;
                total[j] += d->pinned_counts[j];
            }
        }
    }
    const double run = now_ms() - t_run;
    for (uint32_t j = 0; j < K; ++j) counts[j] = total[j];
    if (batch_ms) *batch_ms = run;
    g_last_pre_ms = pre_ms ? pre_ms[K - 1] : 0.0;
    g_last_run_ms = run / K;
    return SMARTGPU_OK;
}

int smartgpu_msearch64(int algo, const uint8_t* P, uint32_t m, smartgpu_mtext* text, int reduce,
                       uint64_t* count, double* pre_ms, double* run_ms)
{
    if (!P) { set_error("pattern is NULL"); return SMARTGPU_ERR_ARG; }
    const uint8_t* one[1] = {P};
    uint64_t c = 0;
    double pre = 0.0, run = 0.0;
    const int rc = smartgpu_msearch_batch64(algo, one, m, 1, text, reduce, &c, &pre, &run);
    if (rc != SMARTGPU_OK) return rc;
    // (the per-device shards of the host-reduce path prepare their tables in turn: pre covers the last device)
    if (count) *count = c;
    if (pre_ms) *pre_ms = pre;
    if (run_ms) *run_ms = run;
    return SMARTGPU_OK;
}

/* ---- table export (tests) ---------------------------------------------- */
int smartgpu_build_table(int which, const uint8_t* P, uint32_t m, int32_t* out, uint32_t cap)
{
    if (!P || !out || m < 1 || m > SMARTGPU_XSIZE) { set_error("bad build_table arguments"); return SMARTGPU_ERR_ARG; }
    std::vector<int32_t> v;
    switch (which) {
        case 0: v = sg::bad_char(P, m); break;
        case 1: v = sg::good_suffix(P, m); break;
        case 2: v = sg::kmp_next(P, m); break;
        case 3: { auto s = sg::shift_or_masks(P, m); v.assign(s.begin(), s.end()); break; }
        case 4: { auto b = sg::bndm_masks(P, m); v.assign(b.begin(), b.end()); break; }
        case 5: {  // KMP transition table, (m+1)*256 entries (m <= 255)
            if (m > 255) { set_error("the KMP transition table needs m <= 255"); return SMARTGPU_ERR_ARG; }
            auto d = sg::kmp_dfa(P, m);
            v.assign(d.begin(), d.end());
            break;
        }
        case 6: {  // compressed form: [k1][colmap 256][table (m+1)*k1]
            if (m > 255) { set_error("the KMP transition table needs m <= 255"); return SMARTGPU_ERR_ARG; }
            uint32_t k1 = 0;
            auto d = sg::kmp_dfa_compressed(P, m, &k1);
            v.push_back(static_cast<int32_t>(k1));
            v.insert(v.end(), d.begin(), d.end());
            break;
        }
        case 7: { auto sa = sg::shift_and_masks(P, m); v.assign(sa.begin(), sa.end()); break; }
        case 9: {  // kmp_runs' tables as the kernel holds them in LDS (bytes; the last 272: Q and thr)
            const uint32_t w = sg::kmp_window(m);
            std::vector<uint8_t> t;
            sg::kmp_runs_tables(P, w, t);
            if (w < 63) {  // the blob stores the rows of the states one after the other: spread them out as the kernel does
                const uint32_t Z = 4 * w + 1;
                std::vector<uint8_t> lds((Z + 1) * 256 + 272, 0);
                for (uint32_t st = 0; st <= w; ++st) std::memcpy(&lds[4 * st * 256], &t[st * 256], 256);
                std::memset(&lds[Z * 256], static_cast<int>(Z), 256);
                std::memcpy(&lds[(Z + 1) * 256], &t[(w + 1) * 256], 272);
                t.swap(lds);
            }
            v.assign(t.begin(), t.end());
            break;
        }
        case 11: {  // kmp_runs' COMPACT tables as the kernel holds them in LDS: rows 0..w, row Z = 4(w+1), then Q and thr (272 bytes)
            const uint32_t w = sg::kmp_compact_window(m);
            std::vector<uint8_t> t;
            sg::kmp_runs_tables(P, w, t, true);
            const uint32_t Z = 4 * w + 4;
            std::vector<uint8_t> lds((w + 2) * 256 + 272, 0);
            std::memcpy(lds.data(), t.data(), (w + 1) * 256);
            std::memset(&lds[(w + 1) * 256], static_cast<int>(Z), 256);
            std::memcpy(&lds[(w + 2) * 256], &t[(w + 1) * 256], 272);
            v.assign(lds.begin(), lds.end());
            break;
        }
        case 10: {  // the two-bit codes of the byte values in P[0..m) taken as a SET (a text's alphabet): shift, symtab; no entries: none
            uint32_t set[8] = {0, 0, 0, 0, 0, 0, 0, 0}, shift = 7, symtab = 0;
            for (uint32_t i = 0; i < m; ++i) set[P[i] >> 5] |= 1u << (P[i] & 31);
            if (sg::four_symbol_codes(set, &shift, &symtab)) {
                v.push_back(static_cast<int32_t>(shift));
                v.push_back(static_cast<int32_t>(symtab));
            }
            break;
        }
        case 8: v = sg::quick_search_shifts(P, m); break;
        case 13: case 15: case 18: {  // HASHq: 256 shifts + the shift after a candidate
            const uint32_t q = static_cast<uint32_t>(which - 10);
            if (m < q) { set_error("HASH%u needs m >= %u", q, q); return SMARTGPU_ERR_ARG; }
            int32_t after = 1;
            v = sg::qgram_hash_shifts(P, m, q, &after);
            v.push_back(after);
            break;
        }
        default: set_error("unknown table %d", which); return SMARTGPU_ERR_ARG;
    }
    if (v.size() > cap) { set_error("table needs %zu entries, cap %u", v.size(), cap); return SMARTGPU_ERR_ARG; }
    std::memcpy(out, v.data(), v.size() * sizeof(int32_t));
    return static_cast<int>(v.size());
}

/* ---- occurrence positions of a pattern set on a BYTE text (k_hormf.hip: hor_multi_find) ----------------------------- */
// smartgpu_pfind_batch64's contract, asked of a smartgpu_text.  The set goes through the staging buffer into the arena
// once (rows, and whole patterns where a window is completed in memory); its passes, find_width(m) patterns each, run
// back to back on the device's stream into ONE entry buffer behind ONE cursor, counting and listing in the same read of
// the text; one synchronisation, one copy_positions, and multi_find_host.hpp's order_find_batch sorts the entries into
// the patterns' slices.  What the device wrote is refused, never reported, where its two tallies disagree.
static_assert(sg::kFindBatchIndexBits == sg::kFindBatchShift, "order_find_batch strips what hor_multi_find adds");
static_assert(sg::kStagingBytes == SMARTGPU_FIND_BATCH_STAGING, "the bound the header documents");

int smartgpu_find_batch64(const uint8_t* const* P, uint32_t m, uint32_t K, const smartgpu_text* text, uint64_t off, uint64_t n,
                          uint64_t* positions, uint64_t cap, uint64_t* starts)
{
    if (!P || K < 1 || !starts) { set_error("find_batch: P/starts NULL or K = 0"); return SMARTGPU_ERR_ARG; }
    if (K > sg::kFindBatchMaxK) { set_error("find_batch: %u patterns in one set (at most %u: an entry keeps 18 bits for the pattern)", K, sg::kFindBatchMaxK); return SMARTGPU_ERR_ARG; }
    const int rc = check_search_args(SMARTGPU_EPSM, P[0], m, text, off, n);
    if (rc != SMARTGPU_OK) return rc;
    if (cap && !positions) { set_error("find_batch: positions NULL with cap > 0"); return SMARTGPU_ERR_ARG; }
    for (uint32_t k = 0; k < K; ++k)
        if (!P[k]) { set_error("find_batch: pattern %u is NULL", k); return SMARTGPU_ERR_ARG; }
    if (K > sg::find_batch_max(m)) {
        set_error("find_batch: %u patterns of length %u, at most %u per call (%u bytes per pattern in the staging buffer of %zu)", K, m, sg::find_batch_max(m),
                  sg::find_batch_bytes(m), sg::kStagingBytes);
        return SMARTGPU_ERR_ARG;
    }
    if (off + n >= sg::kFindBatchMaxEnd) {
        set_error("find_batch: the range ends at byte %llu, it must end below %llu (an entry keeps 46 bits for the position)", (unsigned long long)(off + n),
                  (unsigned long long)sg::kFindBatchMaxEnd);
        return SMARTGPU_ERR_ARG;
    }
    for (uint32_t k = 0; k <= K; ++k) starts[k] = 0;
    if (m > n) return SMARTGPU_OK;  // no window fits: no launch
    if (m < 3) {
        // no gram, no previous byte: K runs of the single-pattern find into consecutive slices; past the room they only count
        for (uint32_t k = 0; k < K; ++k) {
            const uint64_t room = cap > starts[k] ? cap - starts[k] : 0;
            uint64_t c = 0;
            const int r = smartgpu_find64(P[k], m, text, off, n, room ? positions + starts[k] : nullptr, room, &c);
            if (r != SMARTGPU_OK && r != SMARTGPU_ERR_NOMEM) return r;
            if (r == SMARTGPU_ERR_NOMEM && c <= room) return r;  // the device's memory, not the caller's room
            starts[k + 1] = starts[k] + c;
        }
        if (starts[K] > cap) { set_error("find_batch: %llu occurrences, room for %llu", (unsigned long long)starts[K], (unsigned long long)cap); return SMARTGPU_ERR_NOMEM; }
        return SMARTGPU_OK;
    }
    if (!sg::g_hor_multi_find) { set_error("find_batch: this program holds no hor_multi_find kernel (k_hormf.hip is not linked)"); return SMARTGPU_ERR_HIP; }
    DeviceCtx* d = device_ctx_flushed(text->device);
    if (!d) return SMARTGPU_ERR_HIP;
    const uint32_t stride = sg::tail_stride(m), pitch = sg::find_pitch(m);
    const bool in_memory = sg::find_in_memory(m);
    const size_t rows_bytes = static_cast<size_t>(K) * stride, staged = static_cast<size_t>(K) * sg::find_batch_bytes(m);
    if (staged > d->pinned_bytes) { set_error("find_batch: %u patterns exceed the staging buffer", K); return SMARTGPU_ERR_ARG; }
    if (!batch_reserve(d, staged, static_cast<size_t>(K) + 1)) return SMARTGPU_ERR_NOMEM;
    // (the staging buffer is free: every call that fills it ends with a synchronisation of the device's stream)
    for (uint32_t k = 0; k < K; ++k) {
        uint8_t row[sg::kTailRow];
        sg::tail_fill(row, P[k], m);
        std::memcpy(d->pinned + static_cast<size_t>(k) * stride, row, stride);
        if (in_memory) {
            uint8_t* whole = d->pinned + rows_bytes + static_cast<size_t>(k) * pitch;
            std::memcpy(whole, P[k], m);
            std::memset(whole + m, 0, pitch - m);
        }
    }
    const uint64_t per = n - m + 1, bound = per * K;  // (K <= 2^18 and n < 2^46)
    const uint64_t room = cap < bound ? cap : bound;
    bool own = false;
    unsigned long long* out = nullptr;
    uint64_t room_got = room;
    if (room && !(out = find_reserve(d, room, &own))) room_got = 0;  // no device room: the call still counts
    unsigned long long* const cursor = d->batch_counts + K;
    bool ok = hipMemcpyAsync(d->arena, d->pinned, staged, hipMemcpyHostToDevice, d->stream) == hipSuccess &&
              hipMemsetAsync(d->batch_counts, 0, (static_cast<size_t>(K) + 1) * 8, d->stream) == hipSuccess;
    sg::MultiFindArgs a;
    a.text = text->data();
    a.s_begin = off;
    a.s_end = off + per;
    a.m = m;
    a.halo = m - 1 < sg::kHaloMax ? m - 1 : sg::kHaloMax;
    a.counts = d->batch_counts;
    a.out = out;
    a.cap = room_got;
    a.cursor = cursor;
    const uint32_t width = sg::find_width(m);
    for (uint32_t base = 0; base < K && ok; base += width) {
        a.base = base;
        a.np = K - base < width ? K - base : width;
        a.rows = d->arena + static_cast<size_t>(base) * stride;
        a.pats = d->arena + rows_bytes + static_cast<size_t>(base) * pitch;
        ok = sg::g_hor_multi_find(a, d->num_cus, d->stream) == hipSuccess;
    }
    ok = ok && hipMemcpyAsync(d->pinned_counts, d->batch_counts, (static_cast<size_t>(K) + 1) * 8, hipMemcpyDeviceToHost, d->stream) == hipSuccess;
    const bool synced = hipStreamSynchronize(d->stream) == hipSuccess;  // (also after a failure: nothing may still write to the buffers)
    int r = SMARTGPU_OK;
    uint64_t total = 0;
    std::vector<uint64_t> counts(K);
    if (!ok || !synced) {
        set_error("find_batch: %s", hipGetErrorString(hipGetLastError()));
        r = SMARTGPU_ERR_HIP;
    } else {
        // the two tallies of the kernel: every count within the start positions, and the cursor their sum
        for (uint32_t k = 0; k < K && r == SMARTGPU_OK; ++k) {
            counts[k] = d->pinned_counts[k];
            if (counts[k] > per) { set_error("hor_multi_find: pattern %u: count %llu exceeds the %llu start positions", k, (unsigned long long)counts[k], (unsigned long long)per); r = SMARTGPU_ERR_HIP; }
            total += counts[k];
        }
        if (r == SMARTGPU_OK && d->pinned_counts[K] != total) {
            set_error("hor_multi_find: cursor %llu, the patterns' counts add up to %llu", d->pinned_counts[K], (unsigned long long)total);
            r = SMARTGPU_ERR_HIP;
        }
    }
    if (r == SMARTGPU_OK) {
        for (uint32_t k = 0; k < K; ++k) starts[k + 1] = starts[k] + counts[k];
        if (total > cap) {
            set_error("find_batch: %llu occurrences, room for %llu", (unsigned long long)total, (unsigned long long)cap);
            r = SMARTGPU_ERR_NOMEM;
        } else if (total > room_got) {
            set_error("find_batch: %llu occurrences, room for %llu, but the device has no memory for %llu entries", (unsigned long long)total, (unsigned long long)cap, (unsigned long long)room);
            r = SMARTGPU_ERR_NOMEM;
        } else if (total && !copy_positions(d, positions, out, total)) {
            set_error("find_batch: %s", hipGetErrorString(hipGetLastError()));
            r = SMARTGPU_ERR_HIP;
        } else if (total && !sg::order_find_batch(positions, total, K, counts.data(), off, off + n - m, starts)) {
            set_error("hor_multi_find: the entries are not the counted occurrences of %u patterns at distinct starts in [%llu, %llu]", K, (unsigned long long)off, (unsigned long long)(off + n - m));
            r = SMARTGPU_ERR_HIP;
        }
    }
    if (own) (void)hipFree(out);
    return r;
}

}  // extern "C"
