// api.cpp — C ABI of libsmartgpu (include/smartgpu.h): text residency in HBM,
// host-side preprocessing, launches, timing.  Compiled with hipcc as host code.
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

#include "kernels.hpp"
#include "multi.hpp"
#include "multi_find.hpp"
#include "multi_find_host.hpp"
#include "pedit.hpp"
#include "peditl.hpp"
#include "tedit.hpp"
#include "teditl.hpp"
#include "tmis.hpp"
#include "palign.hpp"
#include "talign.hpp"
#include "planes.hpp"
#include "planes_host.hpp"
#include "planes3.hpp"
#include "planes3_host.hpp"
#include "plan.hpp"
#include "route.hpp"
#include "sample.hpp"
#include "tables.hpp"
#include "text_rate.hpp"

namespace {

thread_local std::string g_error;
thread_local double g_last_pre_ms = 0.0, g_last_run_ms = 0.0;

void set_error(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}

#define HIP_TRY(expr, fail)                                                          \
    do {                                                                             \
        hipError_t e_ = (expr);                                                      \
        if (e_ != hipSuccess) {                                                      \
            set_error("%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            fail;                                                                    \
        }                                                                            \
    } while (0)

constexpr int kMaxDevices = 16;

struct DeviceCtx {
    bool ready = false;
    int device = 0;
    hipStream_t stream = nullptr;
    int num_cus = 0;
    uint8_t* pinned = nullptr;      // staging for uploads
    size_t pinned_bytes = 0;
    unsigned long long* pinned_count = nullptr;  // 8-byte readback slot
    hipEvent_t mark[2] = {nullptr, nullptr};     // smartgpu_stream_mark()
    bool hor_preloaded = false;                  // sg::g_hor_preload has run on this device (smartgpu_plan_create)
    // smartgpu_search_batch64(): one arena for the K pattern blobs and the K counts, grown when a
    // batch needs more, never per pattern; K+1 events for the per-pattern device times
    uint8_t* arena = nullptr;
    size_t arena_bytes = 0;
    unsigned long long* batch_counts = nullptr;
    size_t batch_slots = 0;
    unsigned long long* pinned_counts = nullptr;  // host side of the one read-back
    std::vector<hipEvent_t> batch_events;
    // smartgpu_pfind64(): the positions' device buffer, kept between calls while it is small (find_reserve)
    unsigned long long* find_out = nullptr;
    size_t find_out_cap = 0;  // entries
};
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

}  // namespace

struct smartgpu_text {
    int device = 0;
    uint64_t n = 0;
    uint8_t* base = nullptr;  // allocation start; text byte 0 at base + kFrontPad
    const uint8_t* data() const { return base + sg::kFrontPad; }
    // what the text consists of, taken once when it is created (text_alphabet below): the byte values that occur, and
    // — for at most four of them — their two-bit codes (ScanArgs.four_shift, four_symtab; 7: none)
    uint32_t alphabet[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t four_shift = 7, four_symtab = 0, one_bit = 0xFF;
    sg::TextCodes codes() const { sg::TextCodes c; c.shift = four_shift; c.symtab = four_symtab; c.one = one_bit; return c; }
    // how often two of its symbols are equal, from a byte histogram of a sample taken in the same pass (text_rate.hpp);
    // -1: none (text_no_alphabet, a text of fewer than two bytes).  What queue_launch asks before a pattern whose own
    // symbols repeat may ride in a shared pass.
    double rate = -1.0;
    // the 4 bytes at every 28th position (sample.hpp), written once behind the alphabet pass; null: the text has none
    // (smartgpu_text_sampling, a one-search upload, or no memory for it) and its passes read the text itself
    uint32_t* sample = nullptr;
};

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

// device_ctx for an entry point that waits for the device's stream or puts work of its own on it
DeviceCtx* device_ctx_flushed(int device)
{
    DeviceCtx* d = device_ctx(device);
    if (!d) return nullptr;
    const hipError_t e = flush_queue(d);
    if (e != hipSuccess) { set_error("a queued launch failed: %s", hipGetErrorString(e)); return nullptr; }
    return d;
}

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
// pedit.hpp: set by k_pedit.hip where that unit is linked
hipError_t (*g_planes_edit_scan)(const PlaneEditArgs&, int, int, hipStream_t) = nullptr;
hipError_t (*g_planes_edit_find)(const PlaneEditArgs&, unsigned long long*, unsigned long long, int, int, hipStream_t) = nullptr;
// peditl.hpp: set by k_peditl.hip where that unit is linked
hipError_t (*g_planes_editl_scan)(const PlaneEditlArgs&, int, int, hipStream_t) = nullptr;
hipError_t (*g_planes_editl_find)(const PlaneEditlArgs&, unsigned long long*, unsigned long long, int, int, hipStream_t) = nullptr;
// tedit.hpp: set by k_tedit.hip where that unit is linked
hipError_t (*g_text_edit_scan)(const TextEditArgs&, int, hipStream_t) = nullptr;
hipError_t (*g_text_edit_find)(const TextEditArgs&, unsigned long long*, unsigned long long, int, hipStream_t) = nullptr;
// teditl.hpp: set by k_teditl.hip where that unit is linked
hipError_t (*g_text_editl_scan)(const TextEditlArgs&, int, hipStream_t) = nullptr;
hipError_t (*g_text_editl_find)(const TextEditlArgs&, unsigned long long*, unsigned long long, int, hipStream_t) = nullptr;
// tmis.hpp: set by k_tmis.hip where that unit is linked
hipError_t (*g_text_mis_scan)(const TextMisArgs&, int, hipStream_t) = nullptr;
hipError_t (*g_text_mis_find)(const TextMisArgs&, unsigned long long*, unsigned long long, int, hipStream_t) = nullptr;
// palign.hpp: set by k_palign.hip where that unit is linked
hipError_t (*g_planes_edit_align)(const PlaneAlignArgs&, int, hipStream_t) = nullptr;
// talign.hpp: set by k_talign.hip where that unit is linked
hipError_t (*g_text_edit_align)(const TextAlignArgs&, hipStream_t) = nullptr;
// planes3.hpp: set by k_planes3.hip where that unit is linked
hipError_t (*g_planes3_pack)(const uint8_t*, uint64_t, uint32_t*, uint32_t*, uint32_t*, const uint8_t[7], hipStream_t) = nullptr;
hipError_t (*g_planes3_scan)(const Plane3Args&, int, int, hipStream_t) = nullptr;
hipError_t (*g_planes3_find)(const Plane3Args&, unsigned long long*, unsigned long long, int, int, hipStream_t) = nullptr;
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

namespace {

// make sure the device's batch arena holds `blob_bytes` of tables and `k` counts
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

}  // extern "C"

/* ---- packed texts: at most four byte values as bit planes (planes.hpp, k_planes.hip), five to eight on three
 * (planes3.hpp, k_planes3.hip) ------------------------------------------------------------------------------------- */
struct smartgpu_ptext {
    int device = 0;
    uint64_t n = 0;            // symbols
    int planes = 1;            // 1: at most two values, 2: three or four, 3: five to eight
    int nvalues = 0;
    uint8_t values[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // values[code], ascending
    uint8_t* base = nullptr;   // allocation start; plane b at base + kFrontPad + b * plane_stride(n)
    uint32_t* plane(int b) const { return reinterpret_cast<uint32_t*>(base + sg::kFrontPad + static_cast<uint64_t>(b) * sg::plane_stride(n)); }
    uint64_t alloc_bytes() const { return sg::kFrontPad + static_cast<uint64_t>(planes) * sg::plane_stride(n); }
};

namespace {

int check_psearch_args(const uint8_t* P, uint32_t m, const smartgpu_ptext* text, uint64_t off, uint64_t n)
{
    if (!P || m < 1 || m > SMARTGPU_XSIZE) { set_error("pattern length %u outside [1,%d]", m, SMARTGPU_XSIZE); return SMARTGPU_ERR_ARG; }
    if (!text) { set_error("packed text handle is NULL"); return SMARTGPU_ERR_ARG; }
    if (off > text->n || n > text->n - off) { set_error("range [%llu,+%llu) outside the packed text (%llu symbols)", (unsigned long long)off, (unsigned long long)n, (unsigned long long)text->n); return SMARTGPU_ERR_ARG; }
    return SMARTGPU_OK;
}

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
    a.p0 = text->plane(0);
    a.p1 = text->plane(1);
    a.p2 = text->plane(2);
    a.s_begin = off;
    a.s_end = off + n - m + 1;
    a.m = m;
    a.pat = reinterpret_cast<const uint32_t*>(d->arena);
    a.count = d->batch_counts + k;
}

// a.y of Plane3Args: the first dword of each of the eight membership planes at Y
void set_words8(sg::Plane3Args& a, const uint32_t* Y)
{
    for (uint32_t c = 0; c < 8; ++c) a.y[c] = Y[c * sg::kPatWords];
}

// The calls on a three-plane text need k_planes3.hip in the program: a missing kernel is an error, never a fall-back.
bool planes3_linked(const char* call)
{
    if (sg::g_planes3_scan && sg::g_planes3_find) return true;
    set_error("%s: this program holds no planes3_scan / planes3_find kernel (k_planes3.hip is not linked)", call);
    return false;
}

// What the kernels receive for pattern k of a set staged at host_pat (encode_pattern, 2 * kPatWords dwords per pattern)
// and, for m > 32, at the same stride in the device's arena.
sg::PlaneArgs plane_args(const DeviceCtx* d, const smartgpu_ptext* text, const uint32_t* host_pat, uint32_t k, uint32_t m, uint64_t off, uint64_t n)
{
    sg::PlaneArgs a;
    plane_head(a, d, text, m, off, n, k);
    a.x0 = host_pat[2 * sg::kPatWords * k];
    a.x1 = host_pat[2 * sg::kPatWords * k + sg::kPatWords];
    a.pat += 2 * sg::kPatWords * k;
    return a;
}

// What planes3_scan / planes3_find receive for pattern k of a set staged at host_pat (encode_pattern8, kSet8Words dwords per
// pattern) and, for m > 32, at the same stride in the device's arena: an exact pattern, singleton sets, budget 0.
sg::Plane3Args plane3_args(const DeviceCtx* d, const smartgpu_ptext* text, const uint32_t* host_pat, uint32_t k, uint32_t m, uint64_t off, uint64_t n)
{
    sg::Plane3Args a;
    plane_head(a, d, text, m, off, n, k);
    set_words8(a, host_pat + sg::kSet8Words * k);
    a.budget = a.foreign = a.shift = 0;
    a.pat += sg::kSet8Words * k;
    return a;
}

// psearch_impl on a three-plane text (K <= kBatch3Max: checked by the callers before any HIP call): eight membership planes
// per pattern in place of two code planes.
int psearch3_impl(const uint8_t* const* P, uint32_t m, uint32_t K, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                  uint64_t* counts, double* pre_ms, double* run_ms)
{
    if (!planes3_linked("psearch64")) return SMARTGPU_ERR_HIP;
    DeviceCtx* d = device_ctx_flushed(text->device);
    if (!d) return SMARTGPU_ERR_HIP;
    const double t_pre = now_ms();
    constexpr size_t kPatBytes = 4 * sg::kSet8Words;
    if (static_cast<size_t>(K) * kPatBytes > d->pinned_bytes) { set_error("psearch_batch: %u patterns exceed the staging buffer", K); return SMARTGPU_ERR_ARG; }
    if (!batch_reserve(d, static_cast<size_t>(K) * kPatBytes, K)) return SMARTGPU_ERR_NOMEM;
    // (the staging buffer is free: every call that fills it ends with a synchronisation of the device's stream)
    uint32_t* host_pat = reinterpret_cast<uint32_t*>(d->pinned);
    std::vector<uint8_t> present(K, 0);
    for (uint32_t k = 0; k < K; ++k) {
        if (!P[k]) { set_error("pattern %u is NULL", k); return SMARTGPU_ERR_ARG; }
        present[k] = sg::encode_pattern8(text->values, text->nvalues, P[k], m, false, host_pat + sg::kSet8Words * k) == 0;
    }
    const bool fits = n >= m;  // m > n: no window fits, count 0
    if (m > 32 && fits)
        HIP_TRY(hipMemcpyAsync(d->arena, host_pat, static_cast<size_t>(K) * kPatBytes, hipMemcpyHostToDevice, d->stream), return SMARTGPU_ERR_HIP);
    if (pre_ms) *pre_ms = now_ms() - t_pre;
    const double t0 = now_ms();
    HIP_TRY(hipMemsetAsync(d->batch_counts, 0, static_cast<size_t>(K) * 8, d->stream), return SMARTGPU_ERR_HIP);
    for (uint32_t k = 0; k < K && fits; ++k) {
        if (!present[k]) continue;
        const sg::Plane3Args a = plane3_args(d, text, host_pat, k, m, off, n);
        HIP_TRY(sg::g_planes3_scan(a, text->planes, d->num_cus, d->stream), return SMARTGPU_ERR_HIP);
    }
    HIP_TRY(hipMemcpyAsync(d->pinned_counts, d->batch_counts, static_cast<size_t>(K) * 8, hipMemcpyDeviceToHost, d->stream), return SMARTGPU_ERR_HIP);
    HIP_TRY(hipStreamSynchronize(d->stream), return SMARTGPU_ERR_HIP);
    if (run_ms) *run_ms = now_ms() - t0;
    for (uint32_t k = 0; k < K; ++k) {
        // more occurrences than start positions: refused like a poisoned count, never reported
        if (d->pinned_counts[k] > (fits ? n - m + 1 : 0)) { set_error("planes3_scan: count %llu exceeds the %llu start positions", (unsigned long long)d->pinned_counts[k], (unsigned long long)(fits ? n - m + 1 : 0)); return SMARTGPU_ERR_HIP; }
        counts[k] = d->pinned_counts[k];
    }
    return SMARTGPU_OK;
}

// The batch calls' bound on a three-plane text (planes3.hpp: kBatch3Max), decided before any HIP call.
int check_batch3(const char* call, const smartgpu_ptext* text, uint32_t K)
{
    if (text->planes != 3 || K <= sg::kBatch3Max) return SMARTGPU_OK;
    set_error("%s: %u patterns on a three-plane text, at most %u per call (eight membership planes per pattern in the staging buffer)", call, K, sg::kBatch3Max);
    return SMARTGPU_ERR_ARG;
}

// K patterns of m symbols: their planes to the device's arena (m > 32 only: shorter patterns travel as kernel arguments),
// K launches back to back on the device's stream, ONE read-back.  A pattern with a byte the text does not hold: no launch.
int psearch_impl(const uint8_t* const* P, uint32_t m, uint32_t K, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                 uint64_t* counts, double* pre_ms, double* run_ms)
{
    if (text->planes == 3) return psearch3_impl(P, m, K, text, off, n, counts, pre_ms, run_ms);
    DeviceCtx* d = device_ctx_flushed(text->device);
    if (!d) return SMARTGPU_ERR_HIP;
    const double t_pre = now_ms();
    constexpr size_t kPatBytes = 2 * 4 * sg::kPatWords;  // one pattern's two planes
    if (static_cast<size_t>(K) * kPatBytes > d->pinned_bytes) { set_error("psearch_batch: %u patterns exceed the staging buffer", K); return SMARTGPU_ERR_ARG; }
    if (!batch_reserve(d, static_cast<size_t>(K) * kPatBytes, K)) return SMARTGPU_ERR_NOMEM;
    // (the staging buffer is free: every call that fills it ends with a synchronisation of the device's stream)
    uint32_t* host_pat = reinterpret_cast<uint32_t*>(d->pinned);
    std::vector<uint8_t> present(K, 0);
    for (uint32_t k = 0; k < K; ++k) {
        if (!P[k]) { set_error("pattern %u is NULL", k); return SMARTGPU_ERR_ARG; }
        uint32_t* X = host_pat + 2 * sg::kPatWords * k;
        present[k] = sg::encode_pattern(text->values, text->nvalues, P[k], m, X, X + sg::kPatWords, nullptr) == 0;
    }
    const bool fits = n >= m;  // m > n: no window fits, count 0
    if (m > 32 && fits)
        HIP_TRY(hipMemcpyAsync(d->arena, host_pat, static_cast<size_t>(K) * kPatBytes, hipMemcpyHostToDevice, d->stream), return SMARTGPU_ERR_HIP);
    if (pre_ms) *pre_ms = now_ms() - t_pre;
    const double t0 = now_ms();
    HIP_TRY(hipMemsetAsync(d->batch_counts, 0, static_cast<size_t>(K) * 8, d->stream), return SMARTGPU_ERR_HIP);
    for (uint32_t k = 0; k < K && fits; ++k) {
        if (!present[k]) continue;
        const sg::PlaneArgs a = plane_args(d, text, host_pat, k, m, off, n);
        HIP_TRY(sg::launch_planes_scan(a, text->planes, d->num_cus, d->stream), return SMARTGPU_ERR_HIP);
    }
    HIP_TRY(hipMemcpyAsync(d->pinned_counts, d->batch_counts, static_cast<size_t>(K) * 8, hipMemcpyDeviceToHost, d->stream), return SMARTGPU_ERR_HIP);
    HIP_TRY(hipStreamSynchronize(d->stream), return SMARTGPU_ERR_HIP);
    if (run_ms) *run_ms = now_ms() - t0;
    for (uint32_t k = 0; k < K; ++k) {
        // more occurrences than start positions: refused like a poisoned count, never reported
        if (d->pinned_counts[k] > (fits ? n - m + 1 : 0)) { set_error("planes_scan: count %llu exceeds the %llu start positions", (unsigned long long)d->pinned_counts[k], (unsigned long long)(fits ? n - m + 1 : 0)); return SMARTGPU_ERR_HIP; }
        counts[k] = d->pinned_counts[k];
    }
    return SMARTGPU_OK;
}

// The device buffer of `cap` positions for a find.  Up to kFindKeep entries it is the device's own, grown when a call needs
// more and kept (no hipMalloc per call: a find on a packed text takes less time than an allocation); a larger one is the
// call's (*own, to be freed by the caller).
constexpr size_t kFindKeep = size_t(8) << 20;  // entries: 64 MiB
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

// Positions from the device to the caller's (pageable) memory through the device's pinned staging buffer, part by part
// (no overlap of copy and memcpy): a hipMemcpy into pageable memory stages as well, through buffers it sets up per call.
// The staging buffer is free: the patterns it held have been launched and the stream is synchronised.
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

// ---- ONE host path for every single-pattern count and find on a packed text and for the edit-distance calls on a byte
// text: count_run and find_run.  The skeleton fixes the order of the steps — the device's context with nothing queued, the
// arena (batch_reserve), for a find the entries' device buffer (find_reserve; none: the call still counts), the family's
// staging, the slot's memset, the kernel, the read-back, the synchronisation —, the refusal of a count or cursor beyond
// the bound, what *count receives, the find's outcomes (planes_host.hpp: find_outcome) with their return codes and texts,
// and the times (pre: arena and staging; run: memset to synchronisation; counts only).  A family supplies its names
// (RunNames), its bound — n - m + 1 start positions, or n end positions whatever m is —, the bytes it stages into the
// arena, and two lambdas: `stage` (may do nothing; false is a HIP error) and `launch` (fills what its arguments need of the
// device — the result slot is d->batch_counts — and launches).  A find adds a third, `order`: the entries in ascending
// order, or set_error and false for what its kernel cannot have written.  So a family is: checks, masks, args, two
// lambdas; what needs no launch it answers before it comes here. ----
struct RunNames {
    const char* call;     // the entry point: "<call>: ..." for what the caller can mend
    const char* kernel;   // the kernel, for refusals of what the device wrote
    const char* bound;    // what the bound counts: "start positions", "end positions"
    const char* entries;  // what a find lists: "positions", "entries"
};

// What a count call answers: the times for smartgpu_last_times, the count and the times for the caller.
int pcount_done(uint64_t c, double pre, double run, uint64_t* count, double* pre_ms, double* run_ms)
{
    g_last_pre_ms = pre;
    g_last_run_ms = run;
    if (count) *count = c;
    if (pre_ms) *pre_ms = pre;
    if (run_ms) *run_ms = run;
    return SMARTGPU_OK;
}

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

// A find whose every start position is an occurrence (full sets): no launch
int find_every_start(const char* call, uint64_t off, uint64_t total, uint64_t* positions, uint64_t cap, uint64_t* count)
{
    *count = total;
    if (total > cap) { set_error("%s: %llu occurrences, room for %llu", call, (unsigned long long)total, (unsigned long long)cap); return SMARTGPU_ERR_NOMEM; }
    for (uint64_t i = 0; i < total; ++i) positions[i] = off + i;
    return SMARTGPU_OK;
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

// count_run / find_run for the kernels of planes.hpp and planes3.hpp, n >= m: start positions, the pattern's planes at
// `words` staged when m > 32, `a` holds the kind's own fields.  shift: order_spans'.
template <typename Args>
int pcount_run(const char* call, const char* kernel, hipError_t (*launch)(const Args&, int, int, hipStream_t), Args a, const smartgpu_ptext* text,
               const uint32_t* words, size_t bytes, uint32_t m, uint64_t off, uint64_t n, uint64_t* count, double* pre_ms, double* run_ms)
{
    return count_run({call, kernel, "start positions", "positions"}, text->device, bytes, n - m + 1,
                     [&](DeviceCtx* d) { return stage_pattern(d, words, bytes, m); },
                     [&](DeviceCtx* d) { plane_head(a, d, text, m, off, n); return launch(a, text->planes, d->num_cus, d->stream); },
                     count, pre_ms, run_ms);
}

template <typename Args>
int pfind_run(const char* call, const char* kernel, hipError_t (*launch)(const Args&, unsigned long long*, unsigned long long, int, int, hipStream_t),
              Args a, const smartgpu_ptext* text, const uint32_t* words, size_t bytes, uint32_t m, uint64_t off, uint64_t n, uint64_t* positions,
              uint64_t cap, uint64_t* count, uint32_t shift = 0)
{
    const RunNames w = {call, kernel, "start positions", "positions"};
    return find_run(w, text->device, bytes, n - m + 1,
                    [&](DeviceCtx* d) { return stage_pattern(d, words, bytes, m); },
                    [&](DeviceCtx* d, unsigned long long* out, uint64_t room) { plane_head(a, d, text, m, off, n); return launch(a, out, room, text->planes, d->num_cus, d->stream); },
                    [&](uint64_t* e, uint64_t total) { return spans_in_order(w, e, total, off, off + n - m, shift); },
                    positions, cap, count);
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

// The checks of the set, mis and sets-mis calls that need no device; `what` names the pattern argument, k = 0 without mismatches.
int check_pext_args(const char* call, const char* what, const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off,
                    uint64_t n, const uint64_t* count)
{
    if (!P) { set_error("%s: %s is NULL", call, what); return SMARTGPU_ERR_ARG; }
    if (k > SMARTGPU_PMIS_MAX) { set_error("%s: k = %u mismatches, at most %d", call, k, SMARTGPU_PMIS_MAX); return SMARTGPU_ERR_ARG; }
    const int rc = check_psearch_args(P, m, text, off, n);
    if (rc != SMARTGPU_OK) return rc;
    if (!count) { set_error("%s: count must not be NULL", call); return SMARTGPU_ERR_ARG; }
    return SMARTGPU_OK;
}

// encode_sets for a checked call.  SMARTGPU_ERR_ARG: a set names a code the text does not hold.
int sets_planes(const smartgpu_ptext* t, const uint8_t* sets, uint32_t m, bool fill_empty, uint32_t* Y, uint32_t* empty, bool* full)
{
    const int bad = sg::encode_sets(t->nvalues, sets, m, fill_empty, Y, empty, full);
    if (bad < 0) return SMARTGPU_OK;
    set_error("set pattern: position %d: set 0x%02x names a code >= %d, the number of values the text holds", bad, sets[bad], t->nvalues);
    return SMARTGPU_ERR_ARG;
}

// a.y of PlaneSetArgs and PlaneSetMisArgs: the first dword of each membership plane
template <typename Args>
void set_words(Args& a, const uint32_t* Y)
{
    for (uint32_t c = 0; c < 4; ++c) a.y[c] = Y[c * sg::kPatWords];
}

constexpr size_t kMisWords = 3 * sg::kPatWords;  // a pattern's two code planes and its skip plane

// The pattern as X0, X1, SKIP in X[kMisWords] and a.x0, a.x1, a.skip.  Returns the number of foreign positions.
uint32_t mis_planes(const smartgpu_ptext* t, const uint8_t* P, uint32_t m, uint32_t* X, sg::PlaneMisArgs* a)
{
    const uint32_t foreign = sg::encode_pattern(t->values, t->nvalues, P, m, X, X + sg::kPatWords, X + 2 * sg::kPatWords);
    a->x0 = X[0];
    a->x1 = X[sg::kPatWords];
    a->skip = X[2 * sg::kPatWords];
    return foreign;
}

// ---- three-plane texts (planes3.hpp): the exact, set, mismatch and set-with-mismatch calls, count and find, through ONE
// kernel pair.  The callers have made their own checks (check_psearch_args / check_pext_args) ----

// The pattern — bytes, or sets when `sets` — as eight membership planes at Y[kSet8Words] and as a.y, a.foreign, a.budget for
// k mismatches.  *none: more positions that accept nothing (empty sets, foreign bytes) than k, no start position is an
// occurrence; *full: every position accepts every value.  SMARTGPU_ERR_ARG: a set names a code the text does not hold.
int plane3_pattern(const smartgpu_ptext* t, const uint8_t* pat, bool sets, uint32_t m, uint32_t k, uint32_t* Y, sg::Plane3Args* a, bool* none,
                   bool* full)
{
    uint32_t empty = 0;
    *full = false;
    if (sets) {
        const int bad = sg::encode_sets8(t->nvalues, pat, m, true, Y, &empty, full);
        if (bad >= 0) {
            set_error("set pattern: position %d: set 0x%02x names a code >= %d, the number of values the text holds", bad, pat[bad], t->nvalues);
            return SMARTGPU_ERR_ARG;
        }
    } else {
        empty = sg::encode_pattern8(t->values, t->nvalues, pat, m, true, Y);
    }
    *none = empty > k;
    a->foreign = empty;
    a->budget = *none ? 0 : k - empty;
    a->shift = 0;
    set_words8(*a, Y);
    return SMARTGPU_OK;
}

// mis: the call takes k and reports distances (its no-launch cases are those of the two-plane mismatch calls: a pattern of
// full sets is launched there, and answered without a launch by the set calls).
int p3_count(const char* call, const uint8_t* pat, bool sets, bool mis, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
             uint64_t* count, double* pre_ms, double* run_ms)
{
    uint32_t Y[sg::kSet8Words];
    sg::Plane3Args a;
    bool none = false, full = false;
    const int rc = plane3_pattern(text, pat, sets, m, k, Y, &a, &none, &full);
    if (rc != SMARTGPU_OK) return rc;
    if (none || m > n) return pcount_done(0, 0.0, 0.0, count, pre_ms, run_ms);
    if (full && !mis) return pcount_done(n - m + 1, 0.0, 0.0, count, pre_ms, run_ms);
    if (!planes3_linked(call)) return SMARTGPU_ERR_HIP;
    return pcount_run(call, "planes3_scan", sg::g_planes3_scan, a, text, Y, sizeof Y, m, off, n, count, pre_ms, run_ms);
}

int p3_find(const char* call, const uint8_t* pat, bool sets, bool mis, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
            uint64_t* positions, uint8_t* mismatches, uint64_t cap, uint64_t* count)
{
    uint32_t Y[sg::kSet8Words];
    sg::Plane3Args a;
    bool none = false, full = false;
    const int rc = plane3_pattern(text, pat, sets, m, k, Y, &a, &none, &full);
    if (rc != SMARTGPU_OK) return rc;
    if (none || m > n) {
        *count = 0;
        return SMARTGPU_OK;
    }
    if (full && !mis) return find_every_start(call, off, n - m + 1, positions, cap, count);
    if (!planes3_linked(call)) return SMARTGPU_ERR_HIP;
    a.shift = mis ? sg::kMisShift : 0u;
    const int r = pfind_run(call, "planes3_find", sg::g_planes3_find, a, text, Y, sizeof Y, m, off, n, positions, cap, count, a.shift);
    if (mis && r == SMARTGPU_OK) unpack_mis(positions, mismatches, *count);
    return r;
}

// The edit-distance and alignment calls do not read a third plane.
int refuse_planes3(const char* call, const smartgpu_ptext* text)
{
    if (text->planes != 3) return SMARTGPU_OK;
    set_error("%s: three-plane texts (five to eight values) are not offered here: edit distance and alignments read one or two planes", call);
    return SMARTGPU_ERR_ARG;
}

// The edit-distance families below count and list END positions, n of them whatever m is, and m > n is legal; their
// entries are end << shift | distance.  None of them stages planes: `stage` does nothing, or (byte texts) sends the masks.
constexpr auto no_stage = [](DeviceCtx*) { return true; };

// The checks of the edit, editl and align calls that need no device; `what` names the pattern argument, max_m and max_k are
// the family's, flags is 0 for a call that takes none.
int check_pedit_args(const char* call, const char* what, const uint8_t* P, uint32_t m, uint32_t max_m, uint32_t k, uint32_t max_k, uint32_t flags,
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

// The fields that PlaneEditArgs, PlaneEditlArgs and PlaneAlignArgs share
template <typename Args>
void edit_head(Args& a, const smartgpu_ptext* text, uint32_t m, uint32_t k, uint64_t off, uint64_t n)
{
    a.p0 = text->plane(0);
    a.p1 = text->plane(text->planes - 1);
    a.e_begin = off;
    a.e_end = off + n;
    a.m = m;
    a.k = k;
}

// Edit distance, m <= 64 and k <= 7 (pedit.hpp).  The pattern's masks for a checked call, kernel arguments: from bytes
// (sets == false) or from sets.  SMARTGPU_ERR_ARG: a set names a code the text does not hold.
int edit_masks(const smartgpu_ptext* t, const uint8_t* pat, uint32_t m, bool sets, sg::PlaneEditArgs* a)
{
    if (!sets) {
        sg::edit_peq_pattern(t->values, t->nvalues, pat, m, a->peq);
        return SMARTGPU_OK;
    }
    const int bad = sg::edit_peq_sets(t->nvalues, pat, m, a->peq);
    if (bad < 0) return SMARTGPU_OK;
    set_error("set pattern: position %d: set 0x%02x names a code >= %d, the number of values the text holds", bad, pat[bad], t->nvalues);
    return SMARTGPU_ERR_ARG;
}

int pedit_count(const char* call, const uint8_t* pat, bool sets, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                uint64_t* count, double* pre_ms, double* run_ms)
{
    int rc = check_pedit_args(call, sets ? "sets" : "P", pat, m, SMARTGPU_PEDIT_MAXM, k, SMARTGPU_PMIS_MAX, 0, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    sg::PlaneEditArgs a;
    if ((rc = edit_masks(text, pat, m, sets, &a)) != SMARTGPU_OK) return rc;
    if (n + k < m) return pcount_done(0, 0.0, 0.0, count, pre_ms, run_ms);  // not even with k deletions: no launch
    if (!sg::g_planes_edit_scan) { set_error("%s: this program holds no planes_edit_scan kernel (k_pedit.hip is not linked)", call); return SMARTGPU_ERR_HIP; }
    edit_head(a, text, m, k, off, n);
    return count_run({call, "planes_edit_scan", "end positions", "entries"}, text->device, 0, n, no_stage,
                     [&](DeviceCtx* d) { a.count = d->batch_counts; return sg::g_planes_edit_scan(a, text->planes, d->num_cus, d->stream); },
                     count, pre_ms, run_ms);
}

int pedit_find(const char* call, const uint8_t* pat, bool sets, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
               uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    if (cap && !ends) { set_error("%s: ends NULL with cap > 0", call); return SMARTGPU_ERR_ARG; }
    int rc = check_pedit_args(call, sets ? "sets" : "P", pat, m, SMARTGPU_PEDIT_MAXM, k, SMARTGPU_PMIS_MAX, 0, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    sg::PlaneEditArgs a;
    if ((rc = edit_masks(text, pat, m, sets, &a)) != SMARTGPU_OK) return rc;
    if (n + k < m) {
        *count = 0;
        return SMARTGPU_OK;
    }
    if (!sg::g_planes_edit_find) { set_error("%s: this program holds no planes_edit_find kernel (k_pedit.hip is not linked)", call); return SMARTGPU_ERR_HIP; }
    edit_head(a, text, m, k, off, n);
    const RunNames w = {call, "planes_edit_find", "end positions", "entries"};
    rc = find_run(w, text->device, 0, n, no_stage,
                  [&](DeviceCtx* d, unsigned long long* out, uint64_t room) { a.count = d->batch_counts; return sg::g_planes_edit_find(a, out, room, text->planes, d->num_cus, d->stream); },
                  [&](uint64_t* e, uint64_t total) { return spans_in_order(w, e, total, off, off + n - 1, sg::kMisShift); },
                  ends, cap, count);
    if (rc == SMARTGPU_OK) unpack_mis(ends, distances, *count);
    return rc;
}

// BYTE texts: edit distance (tedit.hpp) and mismatches (tmis.hpp), the contracts of the packed calls above with a
// smartgpu_text in place of the planes.  The checks of their calls that need no device; `what` names the pattern argument,
// `noun` what k counts.
int check_text_args(const char* call, const char* what, int max_m, const char* noun, const uint8_t* P, uint32_t m, uint32_t k,
                    const smartgpu_text* text, uint64_t off, uint64_t n, const uint64_t* count)
{
    if (!P) { set_error("%s: %s is NULL", call, what); return SMARTGPU_ERR_ARG; }
    if (m < 1 || m > (uint32_t)max_m) { set_error("%s: pattern length %u outside [1,%d]", call, m, max_m); return SMARTGPU_ERR_ARG; }
    if (k > SMARTGPU_PMIS_MAX) { set_error("%s: k = %u %s, at most %d", call, k, noun, SMARTGPU_PMIS_MAX); return SMARTGPU_ERR_ARG; }
    if (!text) { set_error("%s: text handle is NULL", call); return SMARTGPU_ERR_ARG; }
    if (off > text->n || n > text->n - off) { set_error("%s: range [%llu,+%llu) outside the text (%llu bytes)", call, (unsigned long long)off, (unsigned long long)n, (unsigned long long)text->n); return SMARTGPU_ERR_ARG; }
    if (!count) { set_error("%s: count must not be NULL", call); return SMARTGPU_ERR_ARG; }
    return SMARTGPU_OK;
}

// The pattern is 256 masks (tedit_host.hpp), too many for kernel arguments: bytes or classes as the kernel's table in the
// staging buffer, on their way to the arena (kTEditArena bytes of it), as psearch_impl's patterns travel.  The staging
// buffer is free: every call that fills it ends with a synchronisation.
constexpr size_t kTEditArena = sizeof(uint32_t) * 256 * sg::kTEditWords;
bool text_table_stage(DeviceCtx* d, const uint32_t (&table)[256][sg::kTEditWords], uint32_t words, const uint32_t** dev)
{
    sg::edit_peq_table(table, words, reinterpret_cast<uint32_t*>(d->pinned));
    *dev = reinterpret_cast<const uint32_t*>(d->arena);
    return hipMemcpyAsync(d->arena, d->pinned, 256 * 4 * words, hipMemcpyHostToDevice, d->stream) == hipSuccess;
}

bool tedit_stage(DeviceCtx* d, const uint8_t* pat, bool classes, uint32_t m, const uint32_t** dev)
{
    uint32_t peq[256][sg::kTEditWords];
    if (classes) sg::edit_peq_classes(pat, m, peq); else sg::edit_peq_bytes(pat, m, peq);
    return text_table_stage(d, peq, m <= 32 ? 1u : 2u, dev);
}

// what TextEditArgs, TextMisArgs and TextAlignArgs share: the text and the range, the pattern's length and k
template <class Args>
void text_head(Args& a, const smartgpu_text* text, uint32_t m, uint32_t k, uint64_t off, uint64_t n)
{
    a.text = text->data();
    a.e_begin = off;
    a.e_end = off + n;
    a.m = m;
    a.k = k;
}

int tedit_count(const char* call, const uint8_t* pat, bool classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                uint64_t* count, double* pre_ms, double* run_ms)
{
    const int rc = check_text_args(call, classes ? "classes" : "P", SMARTGPU_EDIT_MAXM, "edits", pat, m, k, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    if (n + k < m) return pcount_done(0, 0.0, 0.0, count, pre_ms, run_ms);  // not even with k deletions: no launch
    if (!sg::g_text_edit_scan) { set_error("%s: this program holds no text_edit_scan kernel (k_tedit.hip is not linked)", call); return SMARTGPU_ERR_HIP; }
    sg::TextEditArgs a;
    text_head(a, text, m, k, off, n);
    return count_run({call, "text_edit_scan", "end positions", "entries"}, text->device, kTEditArena, n,
                     [&](DeviceCtx* d) { return tedit_stage(d, pat, classes, m, &a.peq); },
                     [&](DeviceCtx* d) { a.count = d->batch_counts; return sg::g_text_edit_scan(a, d->num_cus, d->stream); },
                     count, pre_ms, run_ms);
}

int tedit_find(const char* call, const uint8_t* pat, bool classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
               uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    if (cap && !ends) { set_error("%s: ends NULL with cap > 0", call); return SMARTGPU_ERR_ARG; }
    int rc = check_text_args(call, classes ? "classes" : "P", SMARTGPU_EDIT_MAXM, "edits", pat, m, k, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    if (n + k < m) {
        *count = 0;
        return SMARTGPU_OK;
    }
    if (!sg::g_text_edit_find) { set_error("%s: this program holds no text_edit_find kernel (k_tedit.hip is not linked)", call); return SMARTGPU_ERR_HIP; }
    sg::TextEditArgs a;
    text_head(a, text, m, k, off, n);
    const RunNames w = {call, "text_edit_find", "end positions", "entries"};
    rc = find_run(w, text->device, kTEditArena, n,
                  [&](DeviceCtx* d) { return tedit_stage(d, pat, classes, m, &a.peq); },
                  [&](DeviceCtx* d, unsigned long long* out, uint64_t room) { a.count = d->batch_counts; return sg::g_text_edit_find(a, out, room, d->num_cus, d->stream); },
                  [&](uint64_t* e, uint64_t total) { return spans_in_order(w, e, total, off, off + n - 1, sg::kMisShift); },
                  ends, cap, count);
    if (rc == SMARTGPU_OK) unpack_mis(ends, distances, *count);
    return rc;
}

// Mismatches on BYTE texts (tmis.hpp).  The 256 masks "position j does NOT accept this byte" (tmis_host.hpp) travel as
// tedit_stage's: the same table, the same arena.
bool tmis_stage(DeviceCtx* d, const uint8_t* pat, bool classes, uint32_t m, const uint32_t** dev)
{
    uint32_t neq[256][sg::kTEditWords];
    if (classes) sg::mis_neq_classes(pat, m, neq); else sg::mis_neq_bytes(pat, m, neq);
    return text_table_stage(d, neq, static_cast<uint32_t>(sg::mis_words(m)), dev);
}

int tmis_count(const char* call, const uint8_t* pat, bool classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
               uint64_t* count, double* pre_ms, double* run_ms)
{
    const int rc = check_text_args(call, classes ? "classes" : "P", SMARTGPU_MIS_MAXM, "mismatches", pat, m, k, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    if (m > n) return pcount_done(0, 0.0, 0.0, count, pre_ms, run_ms);  // no window fits: no launch
    if (!sg::g_text_mis_scan) { set_error("%s: this program holds no text_mis_scan kernel (k_tmis.hip is not linked)", call); return SMARTGPU_ERR_HIP; }
    sg::TextMisArgs a;
    text_head(a, text, m, k, off, n);
    return count_run({call, "text_mis_scan", "start positions", "positions"}, text->device, kTEditArena, n - m + 1,
                     [&](DeviceCtx* d) { return tmis_stage(d, pat, classes, m, &a.neq); },
                     [&](DeviceCtx* d) { a.count = d->batch_counts; return sg::g_text_mis_scan(a, d->num_cus, d->stream); },
                     count, pre_ms, run_ms);
}

int tmis_find(const char* call, const uint8_t* pat, bool classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
              uint64_t* positions, uint8_t* mismatches, uint64_t cap, uint64_t* count)
{
    if (cap && !positions) { set_error("%s: positions NULL with cap > 0", call); return SMARTGPU_ERR_ARG; }
    int rc = check_text_args(call, classes ? "classes" : "P", SMARTGPU_MIS_MAXM, "mismatches", pat, m, k, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    if (m > n) {
        *count = 0;
        return SMARTGPU_OK;
    }
    if (!sg::g_text_mis_find) { set_error("%s: this program holds no text_mis_find kernel (k_tmis.hip is not linked)", call); return SMARTGPU_ERR_HIP; }
    sg::TextMisArgs a;
    text_head(a, text, m, k, off, n);
    const RunNames w = {call, "text_mis_find", "start positions", "positions"};
    // the kernel's entries hold END positions, the spans order_spans knows (tmis.hpp); a window's start is m - 1 below its end
    rc = find_run(w, text->device, kTEditArena, n - m + 1,
                  [&](DeviceCtx* d) { return tmis_stage(d, pat, classes, m, &a.neq); },
                  [&](DeviceCtx* d, unsigned long long* out, uint64_t room) { a.count = d->batch_counts; return sg::g_text_mis_find(a, out, room, d->num_cus, d->stream); },
                  [&](uint64_t* e, uint64_t total) { return spans_in_order(w, e, total, off, off + n - 1, sg::kMisShift); },
                  positions, cap, count);
    if (rc == SMARTGPU_OK) {
        unpack_mis(positions, mismatches, *count);
        for (uint64_t i = 0; i < *count; ++i) positions[i] -= m - 1;
    }
    return rc;
}

// Edit distance, long patterns (peditl.hpp): m <= 256 and k <= 31, a switch that travels with the call, and entries that
// the kernel writes in no order (order_editl sorts them).  edit_masks, eight dwords wide:
int editl_masks(const smartgpu_ptext* t, const uint8_t* pat, uint32_t m, bool sets, sg::PlaneEditlArgs* a)
{
    if (!sets) {
        sg::editl_peq_pattern(t->values, t->nvalues, pat, m, a->peq);
        return SMARTGPU_OK;
    }
    const int bad = sg::editl_peq_sets(t->nvalues, pat, m, a->peq);
    if (bad < 0) return SMARTGPU_OK;
    set_error("set pattern: position %d: set 0x%02x names a code >= %d, the number of values the text holds", bad, pat[bad], t->nvalues);
    return SMARTGPU_ERR_ARG;
}

int peditl_count(const char* call, const uint8_t* pat, bool sets, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_ptext* text, uint64_t off,
                 uint64_t n, uint64_t* count, double* pre_ms, double* run_ms)
{
    int rc = check_pedit_args(call, sets ? "sets" : "P", pat, m, SMARTGPU_PEDITL_MAXM, k, SMARTGPU_PEDITL_MAXK, flags, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    sg::PlaneEditlArgs a;
    if ((rc = editl_masks(text, pat, m, sets, &a)) != SMARTGPU_OK) return rc;
    if (n + k < m) return pcount_done(0, 0.0, 0.0, count, pre_ms, run_ms);  // not even with k deletions: no launch
    if (!sg::g_planes_editl_scan) { set_error("%s: this program holds no planes_editl_scan kernel (k_peditl.hip is not linked)", call); return SMARTGPU_ERR_HIP; }
    edit_head(a, text, m, k, off, n);
    a.all_blocks = flags & SMARTGPU_PEDITL_ALL_BLOCKS;
    return count_run({call, "planes_editl_scan", "end positions", "entries"}, text->device, 0, n, no_stage,
                     [&](DeviceCtx* d) { a.count = d->batch_counts; return sg::g_planes_editl_scan(a, text->planes, d->num_cus, d->stream); },
                     count, pre_ms, run_ms);
}

int peditl_find(const char* call, const uint8_t* pat, bool sets, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_ptext* text, uint64_t off,
                uint64_t n, uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    if (cap && !ends) { set_error("%s: ends NULL with cap > 0", call); return SMARTGPU_ERR_ARG; }
    int rc = check_pedit_args(call, sets ? "sets" : "P", pat, m, SMARTGPU_PEDITL_MAXM, k, SMARTGPU_PEDITL_MAXK, flags, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    sg::PlaneEditlArgs a;
    if ((rc = editl_masks(text, pat, m, sets, &a)) != SMARTGPU_OK) return rc;
    if (n + k < m) {
        *count = 0;
        return SMARTGPU_OK;
    }
    if (!sg::g_planes_editl_find) { set_error("%s: this program holds no planes_editl_find kernel (k_peditl.hip is not linked)", call); return SMARTGPU_ERR_HIP; }
    edit_head(a, text, m, k, off, n);
    a.all_blocks = flags & SMARTGPU_PEDITL_ALL_BLOCKS;
    rc = find_run({call, "planes_editl_find", "end positions", "entries"}, text->device, 0, n, no_stage,
                  [&](DeviceCtx* d, unsigned long long* out, uint64_t room) { a.count = d->batch_counts; return sg::g_planes_editl_find(a, out, room, text->planes, d->num_cus, d->stream); },
                  [&](uint64_t* e, uint64_t total) {
                      if (sg::order_editl(e, total, off, off + n - 1, k, sg::kEditlShift)) return true;
                      set_error("planes_editl_find: the entries are not distinct end positions of the range with distances <= %u", k);
                      return false;
                  },
                  ends, cap, count);
    if (rc == SMARTGPU_OK) unpack_mis(ends, distances, *count, sg::kEditlShift);
    return rc;
}

// Edit distance on BYTE texts, long patterns (teditl.hpp): tedit_count / tedit_find with peditl's bounds, its switch and its
// unordered entries.  check_text_args' checks, in its order and style, with the wider bounds and the flags check.
int check_teditl_args(const char* call, const char* what, const uint8_t* P, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_text* text,
                      uint64_t off, uint64_t n, const uint64_t* count)
{
    if (!P) { set_error("%s: %s is NULL", call, what); return SMARTGPU_ERR_ARG; }
    if (m < 1 || m > SMARTGPU_EDITL_MAXM) { set_error("%s: pattern length %u outside [1,%d]", call, m, SMARTGPU_EDITL_MAXM); return SMARTGPU_ERR_ARG; }
    if (k > SMARTGPU_EDITL_MAXK) { set_error("%s: k = %u edits, at most %d", call, k, SMARTGPU_EDITL_MAXK); return SMARTGPU_ERR_ARG; }
    if (flags & ~SMARTGPU_EDITL_ALL_BLOCKS) { set_error("%s: flags 0x%x: only SMARTGPU_EDITL_ALL_BLOCKS (0x%x) is defined", call, flags, SMARTGPU_EDITL_ALL_BLOCKS); return SMARTGPU_ERR_ARG; }
    if (!text) { set_error("%s: text handle is NULL", call); return SMARTGPU_ERR_ARG; }
    if (off > text->n || n > text->n - off) { set_error("%s: range [%llu,+%llu) outside the text (%llu bytes)", call, (unsigned long long)off, (unsigned long long)n, (unsigned long long)text->n); return SMARTGPU_ERR_ARG; }
    if (!count) { set_error("%s: count must not be NULL", call); return SMARTGPU_ERR_ARG; }
    return SMARTGPU_OK;
}

// The 256 masks, word-major (teditl_host.hpp: 2, 4 or 8 KiB), through the staging buffer into the arena, as text_table_stage
// sends the short patterns' table.
constexpr size_t kTEditlArena = sizeof(uint32_t) * 256 * sg::kTEditlWords;
bool teditl_stage(DeviceCtx* d, const uint8_t* pat, bool classes, uint32_t m, const uint32_t** dev)
{
    uint32_t peq[256][sg::kTEditlWords];
    if (classes) sg::editl_peq_classes(pat, m, peq); else sg::editl_peq_bytes(pat, m, peq);
    const uint32_t words = m <= 64 ? 2u : m <= 128 ? 4u : 8u;  // the kernels' WORDS (k_teditl.hip)
    sg::editl_peq_table(peq, words, reinterpret_cast<uint32_t*>(d->pinned));
    *dev = reinterpret_cast<const uint32_t*>(d->arena);
    return hipMemcpyAsync(d->arena, d->pinned, 256 * 4 * words, hipMemcpyHostToDevice, d->stream) == hipSuccess;
}

int teditl_count(const char* call, const uint8_t* pat, bool classes, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_text* text, uint64_t off,
                 uint64_t n, uint64_t* count, double* pre_ms, double* run_ms)
{
    const int rc = check_teditl_args(call, classes ? "classes" : "P", pat, m, k, flags, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    if (n + k < m) return pcount_done(0, 0.0, 0.0, count, pre_ms, run_ms);  // not even with k deletions: no launch
    if (!sg::g_text_editl_scan) { set_error("%s: this program holds no text_editl_scan kernel (k_teditl.hip is not linked)", call); return SMARTGPU_ERR_HIP; }
    sg::TextEditlArgs a;
    text_head(a, text, m, k, off, n);
    a.all_blocks = flags & SMARTGPU_EDITL_ALL_BLOCKS;
    return count_run({call, "text_editl_scan", "end positions", "entries"}, text->device, kTEditlArena, n,
                     [&](DeviceCtx* d) { return teditl_stage(d, pat, classes, m, &a.peq); },
                     [&](DeviceCtx* d) { a.count = d->batch_counts; return sg::g_text_editl_scan(a, d->num_cus, d->stream); },
                     count, pre_ms, run_ms);
}

int teditl_find(const char* call, const uint8_t* pat, bool classes, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_text* text, uint64_t off,
                uint64_t n, uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    if (cap && !ends) { set_error("%s: ends NULL with cap > 0", call); return SMARTGPU_ERR_ARG; }
    int rc = check_teditl_args(call, classes ? "classes" : "P", pat, m, k, flags, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    if (n + k < m) {
        *count = 0;
        return SMARTGPU_OK;
    }
    if (!sg::g_text_editl_find) { set_error("%s: this program holds no text_editl_find kernel (k_teditl.hip is not linked)", call); return SMARTGPU_ERR_HIP; }
    sg::TextEditlArgs a;
    text_head(a, text, m, k, off, n);
    a.all_blocks = flags & SMARTGPU_EDITL_ALL_BLOCKS;
    rc = find_run({call, "text_editl_find", "end positions", "entries"}, text->device, kTEditlArena, n,
                  [&](DeviceCtx* d) { return teditl_stage(d, pat, classes, m, &a.peq); },
                  [&](DeviceCtx* d, unsigned long long* out, uint64_t room) { a.count = d->batch_counts; return sg::g_text_editl_find(a, out, room, d->num_cus, d->stream); },
                  [&](uint64_t* e, uint64_t total) {
                      if (sg::order_editl(e, total, off, off + n - 1, k, sg::kTEditlShift)) return true;
                      set_error("text_editl_find: the entries are not distinct end positions of the range with distances <= %u", k);
                      return false;
                  },
                  ends, cap, count);
    if (rc == SMARTGPU_OK) unpack_mis(ends, distances, *count, sg::kTEditlShift);
    return rc;
}

// ---- starts and alignments of edit-distance occurrences (palign.hpp): a list of END positions in, one lane each ----

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

// The refusal of a listed end outside the range [off, off+n), shared by the align calls: the message names i and the value
bool ends_in_range(const char* call, const uint64_t* ends, uint64_t count, uint64_t off, uint64_t n)
{
    for (uint64_t i = 0; i < count; ++i)
        if (ends[i] < off || ends[i] - off >= n) {
            set_error("%s: ends[%llu] = %llu outside the range [%llu,+%llu)", call, (unsigned long long)i, (unsigned long long)ends[i], (unsigned long long)off, (unsigned long long)n);
            return false;
        }
    return true;
}

// Every align call.  The device works in the find's own buffer (find_reserve, at most kFindKeep entries, so never an
// allocation per call beyond the first): a piece of `part` occurrences is [io: part entries | ops: 3 * part words], so a piece
// is kFindKeep occurrences without ops and kFindKeep / 4 with them; longer lists go through piece after piece.
// `launch(io, ops, part)` starts the family's kernel on d->stream over one piece.
template <typename Launch>
int align_pieces(const char* call, DeviceCtx* d, Launch launch, const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances,
                 uint64_t* ops)
{
    const uint64_t piece = ops ? kFindKeep / 4 : kFindKeep;
    for (uint64_t done = 0; done < count;) {
        const uint64_t part = std::min<uint64_t>(count - done, piece);
        bool own = false;
        unsigned long long* buf = find_reserve(d, part * (ops ? 4 : 1), &own);
        if (!buf) return SMARTGPU_ERR_NOMEM;
        unsigned long long* const dev_ops = ops ? buf + part : nullptr;
        const bool ok = upload_positions(d, buf, ends + done, part) &&
                        launch(buf, dev_ops, part) == hipSuccess &&
                        hipStreamSynchronize(d->stream) == hipSuccess &&
                        copy_positions(d, starts + done, buf, part) &&
                        (!ops || copy_positions(d, ops + 3 * done, dev_ops, 3 * part));
        if (!ok) set_error("%s: %s", call, hipGetErrorString(hipGetLastError()));
        if (own) (void)hipFree(buf);
        if (!ok) return SMARTGPU_ERR_HIP;
        for (uint64_t i = done; i < done + part; ++i) {
            const uint64_t v = starts[i];
            const bool none = v == sg::kAlignNone;
            starts[i] = none ? UINT64_MAX : v >> sg::kMisShift;
            if (distances) distances[i] = none ? 255 : static_cast<uint8_t>(v & ((1u << sg::kMisShift) - 1u));
        }
        done += part;
    }
    return SMARTGPU_OK;
}

int palign_run(const char* call, const uint8_t* pat, bool sets, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
               const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    if (count && !ends) { set_error("%s: ends NULL with count > 0", call); return SMARTGPU_ERR_ARG; }
    if (count && !starts) { set_error("%s: starts NULL with count > 0", call); return SMARTGPU_ERR_ARG; }
    int rc = check_pedit_args(call, sets ? "sets" : "P", pat, m, SMARTGPU_PEDIT_MAXM, k, SMARTGPU_PMIS_MAX, 0, text, off, n, &count);
    if (rc != SMARTGPU_OK) return rc;
    sg::PlaneEditArgs masks;
    if ((rc = edit_masks(text, pat, m, sets, &masks)) != SMARTGPU_OK) return rc;  // (the pattern as given: the message names ITS position)
    if (!ends_in_range(call, ends, count, off, n)) return SMARTGPU_ERR_ARG;
    if (count == 0) return SMARTGPU_OK;
    if (!sg::g_planes_edit_align) { set_error("%s: this program holds no planes_edit_align kernel (k_palign.hip is not linked)", call); return SMARTGPU_ERR_HIP; }
    uint8_t rev[SMARTGPU_PEDIT_MAXM];
    for (uint32_t j = 0; j < m; ++j) rev[j] = pat[m - 1 - j];
    (void)edit_masks(text, rev, m, sets, &masks);  // the kernel walks backward: the masks of the REVERSED pattern
    DeviceCtx* d = device_ctx_flushed(text->device);
    if (!d) return SMARTGPU_ERR_HIP;
    sg::PlaneAlignArgs a;
    edit_head(a, text, m, k, off, n);
    std::memcpy(a.peq, masks.peq, sizeof a.peq);
    return align_pieces(call, d,
                        [&](unsigned long long* io, unsigned long long* dev_ops, uint64_t part) {
                            a.io = io;
                            a.ops = dev_ops;
                            a.count = part;
                            return sg::g_planes_edit_align(a, text->planes, d->stream);
                        },
                        ends, count, starts, distances, ops);
}

// The same on a BYTE text (talign.hpp).  The 256 masks of the REVERSED pattern travel to the arena as tedit_stage sends them;
// the staging buffer they leave from is the one upload_positions fills next, so the stream is synchronised in between.
int talign_run(const char* call, const uint8_t* pat, bool classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
               const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    if (count && !ends) { set_error("%s: ends NULL with count > 0", call); return SMARTGPU_ERR_ARG; }
    if (count && !starts) { set_error("%s: starts NULL with count > 0", call); return SMARTGPU_ERR_ARG; }
    const int rc = check_text_args(call, classes ? "classes" : "P", SMARTGPU_EDIT_MAXM, "edits", pat, m, k, text, off, n, &count);
    if (rc != SMARTGPU_OK) return rc;
    if (!ends_in_range(call, ends, count, off, n)) return SMARTGPU_ERR_ARG;
    if (count == 0) return SMARTGPU_OK;
    if (!sg::g_text_edit_align) { set_error("%s: this program holds no text_edit_align kernel (k_talign.hip is not linked)", call); return SMARTGPU_ERR_HIP; }
    uint8_t rev[32 * SMARTGPU_EDIT_MAXM];
    if (classes) sg::talign_reverse_classes(pat, m, rev); else sg::talign_reverse_bytes(pat, m, rev);
    DeviceCtx* d = device_ctx_flushed(text->device);
    if (!d) return SMARTGPU_ERR_HIP;
    if (!batch_reserve(d, kTEditArena, 1)) return SMARTGPU_ERR_NOMEM;
    sg::TextAlignArgs a;
    if (!tedit_stage(d, rev, classes, m, &a.peq) || hipStreamSynchronize(d->stream) != hipSuccess) {
        set_error("%s: %s", call, hipGetErrorString(hipGetLastError()));
        return SMARTGPU_ERR_HIP;
    }
    static_assert(sg::kTextAlignNone == sg::kAlignNone, "align_pieces unpacks both kernels' entries");
    text_head(a, text, m, k, off, n);
    return align_pieces(call, d,
                        [&](unsigned long long* io, unsigned long long* dev_ops, uint64_t part) {
                            a.io = io;
                            a.ops = dev_ops;
                            a.count = part;
                            return sg::g_text_edit_align(a, d->stream);
                        },
                        ends, count, starts, distances, ops);
}

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
    if (k > 4 && !sg::g_planes3_pack) { set_error("ptext_pack8: this program holds no planes3_pack kernel (k_planes3.hip is not linked)"); return nullptr; }
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

int smartgpu_psearch64(const uint8_t* P, uint32_t m, const smartgpu_ptext* text, uint64_t off, uint64_t n, uint64_t* count,
                       double* pre_ms, double* run_ms)
{
    const int rc = check_psearch_args(P, m, text, off, n);
    if (rc != SMARTGPU_OK) return rc;
    const uint8_t* set[1] = {P};
    uint64_t c = 0;
    double pre = 0.0, run = 0.0;
    const int r = psearch_impl(set, m, 1, text, off, n, &c, &pre, &run);
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
    const int r = psearch_impl(P, m, K, text, off, n, counts, &pre, &run);
    if (r != SMARTGPU_OK) return r;
    if (batch_ms) *batch_ms = run;
    g_last_pre_ms = pre / K;
    g_last_run_ms = run / K;
    return SMARTGPU_OK;
}

/* ---- occurrence positions on a packed text (planes_find) ---------------------------------------------------------- */
int smartgpu_pfind64(const uint8_t* P, uint32_t m, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                     uint64_t* positions, uint64_t cap, uint64_t* count)
{
    const int rc = check_psearch_args(P, m, text, off, n);
    if (rc != SMARTGPU_OK) return rc;
    if (!count || (cap && !positions)) { set_error("pfind64: count must not be NULL, positions only with cap = 0"); return SMARTGPU_ERR_ARG; }
    if (text->planes == 3) return p3_find("pfind64", P, false, false, m, 0, text, off, n, positions, nullptr, cap, count);
    uint32_t X[2 * sg::kPatWords];
    if (sg::encode_pattern(text->values, text->nvalues, P, m, X, X + sg::kPatWords, nullptr) || m > n) {
        *count = 0;  // a byte the text does not hold, or no window fits: no launch
        return SMARTGPU_OK;
    }
    sg::PlaneArgs a;
    a.x0 = X[0];
    a.x1 = X[sg::kPatWords];
    return pfind_run("pfind64","planes_find", sg::launch_planes_find, a, text, X, sizeof X, m, off, n, positions, cap, count);
}

int smartgpu_pfind_batch64(const uint8_t* const* P, uint32_t m, uint32_t K, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                           uint64_t* positions, uint64_t cap, uint64_t* starts)
{
    if (!P || K < 1 || !starts) { set_error("pfind_batch: P/starts NULL or K = 0"); return SMARTGPU_ERR_ARG; }
    int rc = check_psearch_args(P[0], m, text, off, n);
    if (rc != SMARTGPU_OK) return rc;
    if (cap && !positions) { set_error("pfind_batch: positions NULL with cap > 0"); return SMARTGPU_ERR_ARG; }
    if ((rc = check_batch3("pfind_batch", text, K)) != SMARTGPU_OK) return rc;
    // pass 1: the K counts (the planes are read twice: a one-pass ordered batch is not built)
    std::vector<uint64_t> counts(K);
    const int r1 = psearch_impl(P, m, K, text, off, n, counts.data(), nullptr, nullptr);
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
        if (text->planes == 3) {  // (linked: psearch3_impl has counted)
            const sg::Plane3Args a = plane3_args(d, text, host_pat, k, m, off, n);
            ok = sg::g_planes3_find(a, out + starts[k], counts[k], text->planes, d->num_cus, d->stream) == hipSuccess;
            continue;
        }
        const sg::PlaneArgs a = plane_args(d, text, host_pat, k, m, off, n);
        ok = sg::launch_planes_find(a, out + starts[k], counts[k], text->planes, d->num_cus, d->stream) == hipSuccess;
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

/* ---- set patterns: every pattern position accepts a set of the text's values ---------------------------------------- */
int smartgpu_psearch_sets64(const uint8_t* sets, uint32_t m, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                            uint64_t* count, double* pre_ms, double* run_ms)
{
    int rc = check_pext_args("psearch_sets64", "sets", sets, m, 0, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    if (text->planes == 3) return p3_count("psearch_sets64", sets, true, false, m, 0, text, off, n, count, pre_ms, run_ms);
    uint32_t Y[sg::kSetWords], empty = 0;
    bool full = false;
    if ((rc = sets_planes(text, sets, m, false, Y, &empty, &full)) != SMARTGPU_OK) return rc;
    if (empty || m > n) return pcount_done(0, 0.0, 0.0, count, pre_ms, run_ms);  // a position that accepts nothing, or no window fits: no launch
    if (full) return pcount_done(n - m + 1, 0.0, 0.0, count, pre_ms, run_ms);    // every start position of the range: no launch
    sg::PlaneSetArgs a;
    set_words(a, Y);
    return pcount_run("psearch_sets64", "planes_sets_scan", sg::launch_planes_sets_scan, a, text, Y, sizeof Y, m, off, n, count, pre_ms, run_ms);
}

int smartgpu_pfind_sets64(const uint8_t* sets, uint32_t m, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                          uint64_t* positions, uint64_t cap, uint64_t* count)
{
    if (cap && !positions) { set_error("pfind_sets64: positions NULL with cap > 0"); return SMARTGPU_ERR_ARG; }
    int rc = check_pext_args("pfind_sets64", "sets", sets, m, 0, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    if (text->planes == 3) return p3_find("pfind_sets64", sets, true, false, m, 0, text, off, n, positions, nullptr, cap, count);
    uint32_t Y[sg::kSetWords], empty = 0;
    bool full = false;
    if ((rc = sets_planes(text, sets, m, false, Y, &empty, &full)) != SMARTGPU_OK) return rc;
    if (empty || m > n) {
        *count = 0;
        return SMARTGPU_OK;
    }
    if (full) return find_every_start("pfind_sets64", off, n - m + 1, positions, cap, count);
    sg::PlaneSetArgs a;
    set_words(a, Y);
    return pfind_run("pfind_sets64", "planes_sets_find", sg::launch_planes_sets_find, a, text, Y, sizeof Y, m, off, n, positions, cap, count);
}

/* ---- mismatches: occurrences within Hamming distance k ---------------------------------------------------------------- */
int smartgpu_psearch_mis64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                           uint64_t* count, double* pre_ms, double* run_ms)
{
    const int rc = check_pext_args("psearch_mis64", "P", P, m, k, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    if (text->planes == 3) return p3_count("psearch_mis64", P, false, true, m, k, text, off, n, count, pre_ms, run_ms);
    uint32_t X[kMisWords];
    sg::PlaneMisArgs a;
    a.foreign = mis_planes(text, P, m, X, &a);
    // more foreign bytes than mismatches allowed, or no window fits: no launch
    if (a.foreign > k || m > n) return pcount_done(0, 0.0, 0.0, count, pre_ms, run_ms);
    a.budget = k - a.foreign;
    return pcount_run("psearch_mis64", "planes_mis_scan", sg::launch_planes_mis_scan, a, text, X, sizeof X, m, off, n, count, pre_ms, run_ms);
}

int smartgpu_pfind_mis64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                         uint64_t* positions, uint8_t* mismatches, uint64_t cap, uint64_t* count)
{
    if (cap && !positions) { set_error("pfind_mis64: positions NULL with cap > 0"); return SMARTGPU_ERR_ARG; }
    const int rc = check_pext_args("pfind_mis64", "P", P, m, k, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    if (text->planes == 3) return p3_find("pfind_mis64", P, false, true, m, k, text, off, n, positions, mismatches, cap, count);
    uint32_t X[kMisWords];
    sg::PlaneMisArgs a;
    a.foreign = mis_planes(text, P, m, X, &a);
    if (a.foreign > k || m > n) {
        *count = 0;
        return SMARTGPU_OK;
    }
    a.budget = k - a.foreign;
    const int r = pfind_run("pfind_mis64", "planes_mis_find", sg::launch_planes_mis_find, a, text, X, sizeof X, m, off, n, positions, cap, count,
                            sg::kMisShift);
    if (r == SMARTGPU_OK) unpack_mis(positions, mismatches, *count);
    return r;
}

/* ---- set patterns with mismatches: at most k positions whose symbol is no member of the position's set ---------------- */
int smartgpu_psearch_sets_mis64(const uint8_t* sets, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                                uint64_t* count, double* pre_ms, double* run_ms)
{
    int rc = check_pext_args("psearch_sets_mis64", "sets", sets, m, k, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    if (text->planes == 3) return p3_count("psearch_sets_mis64", sets, true, true, m, k, text, off, n, count, pre_ms, run_ms);
    uint32_t Y[sg::kSetWords];
    bool full = false;
    sg::PlaneSetMisArgs a;
    if ((rc = sets_planes(text, sets, m, true, Y, &a.foreign, &full)) != SMARTGPU_OK) return rc;
    // more empty sets than mismatches allowed, or no window fits: no launch
    if (a.foreign > k || m > n) return pcount_done(0, 0.0, 0.0, count, pre_ms, run_ms);
    a.budget = k - a.foreign;
    set_words(a, Y);
    return pcount_run("psearch_sets_mis64", "planes_sets_mis_scan", sg::launch_planes_sets_mis_scan, a, text, Y, sizeof Y, m, off, n, count, pre_ms, run_ms);
}

int smartgpu_pfind_sets_mis64(const uint8_t* sets, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                              uint64_t* positions, uint8_t* mismatches, uint64_t cap, uint64_t* count)
{
    if (cap && !positions) { set_error("pfind_sets_mis64: positions NULL with cap > 0"); return SMARTGPU_ERR_ARG; }
    int rc = check_pext_args("pfind_sets_mis64", "sets", sets, m, k, text, off, n, count);
    if (rc != SMARTGPU_OK) return rc;
    if (text->planes == 3) return p3_find("pfind_sets_mis64", sets, true, true, m, k, text, off, n, positions, mismatches, cap, count);
    uint32_t Y[sg::kSetWords];
    bool full = false;
    sg::PlaneSetMisArgs a;
    if ((rc = sets_planes(text, sets, m, true, Y, &a.foreign, &full)) != SMARTGPU_OK) return rc;
    if (a.foreign > k || m > n) {
        *count = 0;
        return SMARTGPU_OK;
    }
    a.budget = k - a.foreign;
    set_words(a, Y);
    const int r = pfind_run("pfind_sets_mis64", "planes_sets_mis_find", sg::launch_planes_sets_mis_find, a, text, Y, sizeof Y, m, off, n, positions,
                            cap, count, sg::kMisShift);
    if (r == SMARTGPU_OK) unpack_mis(positions, mismatches, *count);
    return r;
}

/* ---- edit distance: end positions within k substitutions, insertions and deletions (pedit.hpp, k_pedit.hip) ------------ */
int smartgpu_psearch_edit64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                            uint64_t* count, double* pre_ms, double* run_ms)
{
    return pedit_count("psearch_edit64", P, false, m, k, text, off, n, count, pre_ms, run_ms);
}

int smartgpu_pfind_edit64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                          uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return pedit_find("pfind_edit64", P, false, m, k, text, off, n, ends, distances, cap, count);
}

int smartgpu_psearch_sets_edit64(const uint8_t* sets, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                                 uint64_t* count, double* pre_ms, double* run_ms)
{
    return pedit_count("psearch_sets_edit64", sets, true, m, k, text, off, n, count, pre_ms, run_ms);
}

int smartgpu_pfind_sets_edit64(const uint8_t* sets, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                               uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return pedit_find("pfind_sets_edit64", sets, true, m, k, text, off, n, ends, distances, cap, count);
}

/* ---- edit distance on byte texts: the same question of a smartgpu_text (tedit.hpp, k_tedit.hip) ------------------------- */
int smartgpu_search_edit64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                           uint64_t* count, double* pre_ms, double* run_ms)
{
    return tedit_count("search_edit64", P, false, m, k, text, off, n, count, pre_ms, run_ms);
}

int smartgpu_find_edit64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                         uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return tedit_find("find_edit64", P, false, m, k, text, off, n, ends, distances, cap, count);
}

int smartgpu_search_edit_classes64(const uint8_t* classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                                   uint64_t* count, double* pre_ms, double* run_ms)
{
    return tedit_count("search_edit_classes64", classes, true, m, k, text, off, n, count, pre_ms, run_ms);
}

int smartgpu_find_edit_classes64(const uint8_t* classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                                 uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return tedit_find("find_edit_classes64", classes, true, m, k, text, off, n, ends, distances, cap, count);
}

/* ---- edit distance on byte texts, long patterns: m <= 256, k <= 31 (teditl.hpp, k_teditl.hip) --------------------------- */
int smartgpu_search_editl64(const uint8_t* P, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_text* text, uint64_t off, uint64_t n,
                            uint64_t* count, double* pre_ms, double* run_ms)
{
    return teditl_count("search_editl64", P, false, m, k, flags, text, off, n, count, pre_ms, run_ms);
}

int smartgpu_find_editl64(const uint8_t* P, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_text* text, uint64_t off, uint64_t n,
                          uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return teditl_find("find_editl64", P, false, m, k, flags, text, off, n, ends, distances, cap, count);
}

int smartgpu_search_editl_classes64(const uint8_t* classes, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_text* text, uint64_t off,
                                    uint64_t n, uint64_t* count, double* pre_ms, double* run_ms)
{
    return teditl_count("search_editl_classes64", classes, true, m, k, flags, text, off, n, count, pre_ms, run_ms);
}

int smartgpu_find_editl_classes64(const uint8_t* classes, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_text* text, uint64_t off,
                                  uint64_t n, uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return teditl_find("find_editl_classes64", classes, true, m, k, flags, text, off, n, ends, distances, cap, count);
}

/* ---- mismatches on byte texts: smartgpu_psearch_mis64's question of a smartgpu_text (tmis.hpp, k_tmis.hip) --------------- */
int smartgpu_search_mis64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                          uint64_t* count, double* pre_ms, double* run_ms)
{
    return tmis_count("search_mis64", P, false, m, k, text, off, n, count, pre_ms, run_ms);
}

int smartgpu_find_mis64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                        uint64_t* positions, uint8_t* mismatches, uint64_t cap, uint64_t* count)
{
    return tmis_find("find_mis64", P, false, m, k, text, off, n, positions, mismatches, cap, count);
}

int smartgpu_search_mis_classes64(const uint8_t* classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                                  uint64_t* count, double* pre_ms, double* run_ms)
{
    return tmis_count("search_mis_classes64", classes, true, m, k, text, off, n, count, pre_ms, run_ms);
}

int smartgpu_find_mis_classes64(const uint8_t* classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                                uint64_t* positions, uint8_t* mismatches, uint64_t cap, uint64_t* count)
{
    return tmis_find("find_mis_classes64", classes, true, m, k, text, off, n, positions, mismatches, cap, count);
}

/* ---- edit distance, long patterns: m <= 256, k <= 31 (peditl.hpp, k_peditl.hip) ---------------------------------------- */
int smartgpu_psearch_editl64(const uint8_t* P, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                             uint64_t* count, double* pre_ms, double* run_ms)
{
    return peditl_count("psearch_editl64", P, false, m, k, flags, text, off, n, count, pre_ms, run_ms);
}

int smartgpu_pfind_editl64(const uint8_t* P, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                           uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return peditl_find("pfind_editl64", P, false, m, k, flags, text, off, n, ends, distances, cap, count);
}

int smartgpu_psearch_sets_editl64(const uint8_t* sets, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                                  uint64_t* count, double* pre_ms, double* run_ms)
{
    return peditl_count("psearch_sets_editl64", sets, true, m, k, flags, text, off, n, count, pre_ms, run_ms);
}

int smartgpu_pfind_sets_editl64(const uint8_t* sets, uint32_t m, uint32_t k, uint32_t flags, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                                uint64_t* ends, uint8_t* distances, uint64_t cap, uint64_t* count)
{
    return peditl_find("pfind_sets_editl64", sets, true, m, k, flags, text, off, n, ends, distances, cap, count);
}

/* ---- edit distance: start positions and alignments of listed end positions (palign.hpp, k_palign.hip) ------------------ */
int smartgpu_palign_edit64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                           const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    return palign_run("palign_edit64", P, false, m, k, text, off, n, ends, count, starts, distances, ops);
}

int smartgpu_palign_sets_edit64(const uint8_t* sets, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                                const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    return palign_run("palign_sets_edit64", sets, true, m, k, text, off, n, ends, count, starts, distances, ops);
}

/* ---- the same on byte texts (talign.hpp, k_talign.hip) ------------------------------------------------------------------ */
int smartgpu_align_edit64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                          const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    return talign_run("align_edit64", P, false, m, k, text, off, n, ends, count, starts, distances, ops);
}

int smartgpu_align_edit_classes64(const uint8_t* classes, uint32_t m, uint32_t k, const smartgpu_text* text, uint64_t off, uint64_t n,
                                  const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    return talign_run("align_edit_classes64", classes, true, m, k, text, off, n, ends, count, starts, distances, ops);
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
