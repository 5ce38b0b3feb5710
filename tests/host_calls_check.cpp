// host_calls_check.cpp — tests/test_host_calls.py builds this with the C ABI's call layer (match_calls.cpp and align_calls.cpp,
// the real units) under AddressSanitizer and UBSan and runs it as a program: what those units need of api.cpp (host_ctx.hpp),
// of k_planes.hip (the launch_planes_* launchers) and of the self-registering kernel units (the g_* pointers) are STUBS here,
// and the text handles are plain structs.  No GPU: device_ctx_flushed answers "no device" with a marker message, so a call is
// followed exactly as far as its first step that needs one.
//
// One line per case on stdout, tab separated:  id  rc  device_ctx_flushed calls  launcher calls  outputs written  message
// (the message last: it may hold anything but a tab).  tests/golden/host_call_cases.json holds these lines as recorded from the
// library before the call layer was rearranged — a pair of violations under the line of its earlier one, which it must equal.  What the driver itself asserts (a failure is a line on stderr and exit 1):
//   * order: every call has its ORDERED list of violations, written from the code; a call with two of them answers as the
//     call with the earlier one alone;
//   * a refused call asks for no device and writes nothing;
//   * no case reaches what comes behind the device's context (batch_reserve, find_reserve, copy_positions, probe_read_ms,
//     smartgpu_text_upload, a launcher).
#include "../include/smartgpu.h"
#include "../smart_amd/csrc/host_ctx.hpp"
#include "../smart_amd/csrc/palign.hpp"
#include "../smart_amd/csrc/pedit.hpp"
#include "../smart_amd/csrc/peditl.hpp"
#include "../smart_amd/csrc/planes.hpp"
#include "../smart_amd/csrc/planes3.hpp"
#include "../smart_amd/csrc/talign.hpp"
#include "../smart_amd/csrc/talignl.hpp"
#include "../smart_amd/csrc/tedit.hpp"
#include "../smart_amd/csrc/teditl.hpp"
#include "../smart_amd/csrc/tmis.hpp"

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

// ---- the stubs --------------------------------------------------------------------------------------------------------
static char g_msg[512];
static int g_dev, g_launch, g_behind, g_failures;

void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
}

static const char kMarker[] = "(stub) device_ctx_flushed: this program has no device";
DeviceCtx* device_ctx_flushed(int) { ++g_dev; set_error("%s", kMarker); return nullptr; }
bool batch_reserve(DeviceCtx*, size_t, size_t) { ++g_behind; return false; }
unsigned long long* find_reserve(DeviceCtx*, uint64_t, bool*) { ++g_behind; return nullptr; }
bool copy_positions(DeviceCtx*, uint64_t*, const unsigned long long*, uint64_t) { ++g_behind; return false; }
int probe_read_ms(const DeviceCtx*, const uint8_t*, uint64_t, unsigned long long*, int, double*) { ++g_behind; return SMARTGPU_ERR_HIP; }
extern "C" smartgpu_text* smartgpu_text_upload(const void*, uint64_t, int) { ++g_behind; return nullptr; }
extern "C" void smartgpu_text_free(smartgpu_text*) { ++g_behind; }

// as in api.cpp
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
int pcount_done(uint64_t c, double pre, double run, uint64_t* count, double* pre_ms, double* run_ms)
{
    if (count) *count = c;
    if (pre_ms) *pre_ms = pre;
    if (run_ms) *run_ms = run;
    return SMARTGPU_OK;
}

template <typename... A>
static hipError_t launched(A...) { ++g_launch; return hipSuccess; }

namespace sg {
hipError_t launch_planes_pack(const uint8_t*, uint64_t, uint32_t*, uint32_t*, int, const uint8_t[3], hipStream_t) { return launched(); }
hipError_t launch_planes_scan(const PlaneArgs&, int, int, hipStream_t) { return launched(); }
hipError_t launch_planes_find(const PlaneArgs&, unsigned long long*, unsigned long long, int, int, hipStream_t) { return launched(); }
hipError_t launch_planes_sets_scan(const PlaneSetArgs&, int, int, hipStream_t) { return launched(); }
hipError_t launch_planes_sets_find(const PlaneSetArgs&, unsigned long long*, unsigned long long, int, int, hipStream_t) { return launched(); }
hipError_t launch_planes_mis_scan(const PlaneMisArgs&, int, int, hipStream_t) { return launched(); }
hipError_t launch_planes_mis_find(const PlaneMisArgs&, unsigned long long*, unsigned long long, int, int, hipStream_t) { return launched(); }
hipError_t launch_planes_sets_mis_scan(const PlaneSetMisArgs&, int, int, hipStream_t) { return launched(); }
hipError_t launch_planes_sets_mis_find(const PlaneSetMisArgs&, unsigned long long*, unsigned long long, int, int, hipStream_t) { return launched(); }
}

// the launchers of the units that register themselves: all of them linked (recording stubs), or none
template <typename... A>
static void link_one(hipError_t (*&p)(A...), bool linked) { p = linked ? &launched<A...> : nullptr; }

static void link_kernels(bool linked)
{
    link_one(sg::g_planes_edit_scan, linked);
    link_one(sg::g_planes_edit_find, linked);
    link_one(sg::g_planes_editl_scan, linked);
    link_one(sg::g_planes_editl_find, linked);
    link_one(sg::g_text_edit_scan, linked);
    link_one(sg::g_text_edit_find, linked);
    link_one(sg::g_text_editl_scan, linked);
    link_one(sg::g_text_editl_find, linked);
    link_one(sg::g_text_mis_scan, linked);
    link_one(sg::g_text_mis_find, linked);
    link_one(sg::g_planes_edit_align, linked);
    link_one(sg::g_text_edit_align, linked);
    link_one(sg::g_text_editl_align, linked);
    link_one(sg::g_planes3_pack, linked);
    link_one(sg::g_planes3_scan, linked);
    link_one(sg::g_planes3_find, linked);
}

// ---- the handles: a byte text of 100 bytes (four values, and one of six for smartgpu_ptext_pack8), packed texts of 100 symbols
// on one, two and three planes.  The memory behind them is real (a call computes addresses in it) and never read. ----
static const uint64_t kTextN = 100;
static std::vector<uint8_t> g_memory(sg::kFrontPad + 3 * sg::plane_stride(kTextN));
static smartgpu_text g_text, g_text6;
static smartgpu_ptext g_ptext[4];  // [planes]

static void make_handles()
{
    const uint8_t six[6] = {'-', 'A', 'C', 'G', 'N', 'T'};
    const uint8_t four[4] = {'A', 'C', 'G', 'T'};
    g_text.n = g_text6.n = kTextN;
    g_text.base = g_text6.base = g_memory.data();
    for (uint8_t c : four) g_text.alphabet[c >> 5] |= 1u << (c & 31);
    for (uint8_t c : six) g_text6.alphabet[c >> 5] |= 1u << (c & 31);
    for (int planes = 1; planes <= 3; ++planes) {
        smartgpu_ptext& p = g_ptext[planes];
        p.n = kTextN;
        p.planes = planes;
        p.nvalues = 2 * planes;
        std::memcpy(p.values, planes == 3 ? six : four, p.nvalues);
        p.base = g_memory.data();
    }
}

// ---- what a call may write: sentinels, as tests/test_refusal_messages.py keeps them ----
static const uint64_t kGuard64 = 0xDEADBEEFDEADBEEFull;
static const uint8_t kGuard8 = 0xA5;
static const uint64_t kRoom = 128;
struct Outputs {
    uint64_t count;
    double pre, run;
    uint64_t out[kRoom], starts[kRoom], ops[SMARTGPU_ALIGNL_OPS_WORDS * kRoom];
    uint8_t dist[kRoom], small[16];
    int planes;
    void reset()
    {
        count = 77;
        pre = -1.0;
        run = -2.0;
        for (auto& v : out) v = kGuard64;
        for (auto& v : starts) v = kGuard64;
        for (auto& v : ops) v = kGuard64;
        std::memset(dist, kGuard8, sizeof dist);
        std::memset(small, kGuard8, sizeof small);
        planes = -7;
    }
    template <typename T, size_t N>
    static size_t written(const T (&a)[N], T guard)
    {
        size_t w = 0;
        for (const T& v : a) w += v != guard;
        return w;
    }
    // "-" for nothing; else what changed: the count's value, the times, and of `out` how many entries, the first, and whether
    // they ascend by one
    std::string touched() const
    {
        std::string s;
        char b[96];
        if (count != 77) { snprintf(b, sizeof b, "count=%llu ", (unsigned long long)count); s += b; }
        if (pre != -1.0 || run != -2.0) { snprintf(b, sizeof b, "times=%g,%g ", pre, run); s += b; }
        if (const size_t w = written(out, kGuard64)) {
            bool seq = true;
            for (size_t i = 0; i < w; ++i) seq = seq && out[i] == out[0] + i;
            snprintf(b, sizeof b, "out=%zu from %llu%s ", w, (unsigned long long)out[0], seq ? " by one" : " NOT by one");
            s += b;
        }
        if (written(starts, kGuard64)) s += "starts ";
        if (written(ops, kGuard64)) s += "ops ";
        if (written(dist, kGuard8)) s += "dist ";
        if (written(small, kGuard8)) s += "small ";
        if (planes != -7) s += "planes ";
        if (s.empty()) return "-";
        s.pop_back();
        return s;
    }
};
static Outputs g_o;

// ---- the arguments of a call, valid unless a violation changes them ----
static uint8_t g_bytes[4300], g_sets[4300], g_classes[32 * 300];
static const uint8_t* g_set_of_two[2] = {g_bytes, g_bytes};
static const uint8_t* g_set_null_first[2] = {nullptr, g_bytes};
static std::vector<const uint8_t*> g_set_many(sg::kBatch3Max + 1, g_bytes);
static const uint64_t g_ends_ok[3] = {10, 50, 89};
static const uint64_t g_ends_bad[3] = {10, 90, 5};  // the range is [10,+80): [1] is the first outside it, [2] is outside too
static uint64_t g_ends_eight[8] = {0, 1, 2, 3, 4, 5, 6, 7};

struct Args {
    const uint8_t* pat;
    const uint8_t* const* set = g_set_of_two;
    uint32_t m = 4, K = 2, k = 1, flags = 0;
    const void* text;
    uint64_t off = 10, n = 80;
    uint64_t* count = &g_o.count;   // a count's and a find's count, a batch count's counts, a batch find's starts
    uint64_t* out = g_o.out;        // a find's entries
    uint64_t cap = kRoom;
    const uint64_t* ends = g_ends_ok;
    uint64_t nends = 3;
    uint64_t* starts = g_o.starts;  // an align call's
};

enum Family { kExactCount, kExactFind, kBatchCount, kBatchFind, kPExt, kPEdit, kText, kPAlign, kTAlign };

struct Call {
    const char* name;
    Family family;
    bool find, sets, has_k, has_flags, starts;  // starts: counts START positions (no launch when m > n), else ends (n + k < m)
    uint32_t max_m, max_k;
    std::function<long(const Args&)> fn;
    bool packed() const { return family != kText && family != kTAlign; }
    bool align() const { return family == kPAlign || family == kTAlign; }
    bool batch() const { return family == kBatchCount || family == kBatchFind; }
    Args valid(int planes = 2) const
    {
        Args a;
        a.pat = !sets ? g_bytes : packed() ? g_sets : g_classes;
        a.text = packed() ? static_cast<const void*>(&g_ptext[planes]) : &g_text;
        return a;
    }
};

#define PT(a) static_cast<const smartgpu_ptext*>(a.text)
#define BT(a) static_cast<const smartgpu_text*>(a.text)
#define TIMES &g_o.pre, &g_o.run
#define FN(expr) [](const Args& a) -> long { return expr; }
#define COUNT0(name, T) FN(smartgpu_##name(a.pat, a.m, T(a), a.off, a.n, a.count, TIMES))
#define COUNTK(name, T) FN(smartgpu_##name(a.pat, a.m, a.k, T(a), a.off, a.n, a.count, TIMES))
#define COUNTF(name, T) FN(smartgpu_##name(a.pat, a.m, a.k, a.flags, T(a), a.off, a.n, a.count, TIMES))
#define FIND0(name, T) FN(smartgpu_##name(a.pat, a.m, T(a), a.off, a.n, a.out, a.cap, a.count))
#define FINDK(name, T) FN(smartgpu_##name(a.pat, a.m, a.k, T(a), a.off, a.n, a.out, g_o.dist, a.cap, a.count))
#define FINDF(name, T) FN(smartgpu_##name(a.pat, a.m, a.k, a.flags, T(a), a.off, a.n, a.out, g_o.dist, a.cap, a.count))
#define ALIGN(name, T) FN(smartgpu_##name(a.pat, a.m, a.k, T(a), a.off, a.n, a.ends, a.nends, a.starts, g_o.dist, g_o.ops))

static const uint32_t X = SMARTGPU_XSIZE;
static const std::vector<Call> kCalls = {
    // name, family, find, sets, k, flags, starts, max m, max k
    {"psearch64", kExactCount, false, false, false, false, true, X, 0, COUNT0(psearch64, PT)},
    {"pfind64", kExactFind, true, false, false, false, true, X, 0, FIND0(pfind64, PT)},
    {"psearch_batch64", kBatchCount, false, false, false, false, true, X, 0,
     FN(smartgpu_psearch_batch64(a.set, a.m, a.K, PT(a), a.off, a.n, a.count, &g_o.run))},
    {"pfind_batch64", kBatchFind, true, false, false, false, true, X, 0,
     FN(smartgpu_pfind_batch64(a.set, a.m, a.K, PT(a), a.off, a.n, a.out, a.cap, a.count))},
    {"psearch_sets64", kPExt, false, true, false, false, true, X, 0, COUNT0(psearch_sets64, PT)},
    {"pfind_sets64", kPExt, true, true, false, false, true, X, 0, FIND0(pfind_sets64, PT)},
    {"psearch_mis64", kPExt, false, false, true, false, true, X, 7, COUNTK(psearch_mis64, PT)},
    {"pfind_mis64", kPExt, true, false, true, false, true, X, 7, FINDK(pfind_mis64, PT)},
    {"psearch_sets_mis64", kPExt, false, true, true, false, true, X, 7, COUNTK(psearch_sets_mis64, PT)},
    {"pfind_sets_mis64", kPExt, true, true, true, false, true, X, 7, FINDK(pfind_sets_mis64, PT)},
    {"psearch_edit64", kPEdit, false, false, true, false, false, 64, 7, COUNTK(psearch_edit64, PT)},
    {"pfind_edit64", kPEdit, true, false, true, false, false, 64, 7, FINDK(pfind_edit64, PT)},
    {"psearch_sets_edit64", kPEdit, false, true, true, false, false, 64, 7, COUNTK(psearch_sets_edit64, PT)},
    {"pfind_sets_edit64", kPEdit, true, true, true, false, false, 64, 7, FINDK(pfind_sets_edit64, PT)},
    {"psearch_editl64", kPEdit, false, false, true, true, false, 256, 31, COUNTF(psearch_editl64, PT)},
    {"pfind_editl64", kPEdit, true, false, true, true, false, 256, 31, FINDF(pfind_editl64, PT)},
    {"psearch_sets_editl64", kPEdit, false, true, true, true, false, 256, 31, COUNTF(psearch_sets_editl64, PT)},
    {"pfind_sets_editl64", kPEdit, true, true, true, true, false, 256, 31, FINDF(pfind_sets_editl64, PT)},
    {"search_edit64", kText, false, false, true, false, false, 64, 7, COUNTK(search_edit64, BT)},
    {"find_edit64", kText, true, false, true, false, false, 64, 7, FINDK(find_edit64, BT)},
    {"search_edit_classes64", kText, false, true, true, false, false, 64, 7, COUNTK(search_edit_classes64, BT)},
    {"find_edit_classes64", kText, true, true, true, false, false, 64, 7, FINDK(find_edit_classes64, BT)},
    {"search_editl64", kText, false, false, true, true, false, 256, 31, COUNTF(search_editl64, BT)},
    {"find_editl64", kText, true, false, true, true, false, 256, 31, FINDF(find_editl64, BT)},
    {"search_editl_classes64", kText, false, true, true, true, false, 256, 31, COUNTF(search_editl_classes64, BT)},
    {"find_editl_classes64", kText, true, true, true, true, false, 256, 31, FINDF(find_editl_classes64, BT)},
    {"search_mis64", kText, false, false, true, false, true, 64, 7, COUNTK(search_mis64, BT)},
    {"find_mis64", kText, true, false, true, false, true, 64, 7, FINDK(find_mis64, BT)},
    {"search_mis_classes64", kText, false, true, true, false, true, 64, 7, COUNTK(search_mis_classes64, BT)},
    {"find_mis_classes64", kText, true, true, true, false, true, 64, 7, FINDK(find_mis_classes64, BT)},
    {"palign_edit64", kPAlign, false, false, true, false, false, 64, 7, ALIGN(palign_edit64, PT)},
    {"palign_sets_edit64", kPAlign, false, true, true, false, false, 64, 7, ALIGN(palign_sets_edit64, PT)},
    {"align_edit64", kTAlign, false, false, true, false, false, 64, 7, ALIGN(align_edit64, BT)},
    {"align_edit_classes64", kTAlign, false, true, true, false, false, 64, 7, ALIGN(align_edit_classes64, BT)},
    {"align_editl64", kTAlign, false, false, true, false, false, 256, 31, ALIGN(align_editl64, BT)},
    {"align_editl_classes64", kTAlign, false, true, true, false, false, 256, 31, ALIGN(align_editl_classes64, BT)},
};

// ---- one case ----
struct Result {
    long rc;
    int dev, launch;
    std::string touched, msg;
    bool same_answer(const Result& o) const { return rc == o.rc && msg == o.msg; }
};

static void fail(const std::string& id, const char* what)
{
    fprintf(stderr, "FAIL %s: %s\n", id.c_str(), what);
    ++g_failures;
}

static void print_case(const std::string& id, const char* rc, const Result& r)
{
    printf("%s\t%s\t%d\t%d\t%s\t%s\n", id.c_str(), rc, r.dev, r.launch, r.touched.c_str(), r.msg.c_str());
}

template <typename F>
static Result run_case(const std::string& id, F call, bool known_message = false, const char* rc_text = nullptr)
{
    g_o.reset();
    g_dev = g_launch = 0;
    snprintf(g_msg, sizeof g_msg, "(no message)");
    if (known_message) (void)smartgpu_iupac_revcomp(nullptr, 1, nullptr);  // as tests/test_refusal_messages.py starts a case
    Result r;
    r.rc = call();
    r.dev = g_dev;
    r.launch = g_launch;
    r.touched = g_o.touched();
    r.msg = g_msg;
    print_case(id, rc_text ? rc_text : std::to_string(r.rc).c_str(), r);
    if (g_behind) { fail(id, "reached what comes behind the device's context"); g_behind = 0; }
    if (r.launch) fail(id, "reached a launcher");
    if (r.dev > 1) fail(id, "asked for the device more than once");
    return r;
}

static Result refused_case(const std::string& id, const Call& c, const Args& a)
{
    const Result r = run_case(id, [&] { return c.fn(a); });
    if (r.rc != SMARTGPU_ERR_ARG) fail(id, "not refused with SMARTGPU_ERR_ARG");
    if (r.dev) fail(id, "a refused call asked for the device");
    if (r.touched != "-") fail(id, "a refused call wrote an output");
    return r;
}

// ---- the violations.  A Form changes a valid call's arguments; `fields` says which, and two forms that change the same
// field do not combine.  A Slot is ONE check of the call: its forms are alternatives (m = 0 and m too large; the three
// ways out of the text).  A call's list of slots is in the order of its checks. ----
enum : unsigned { fPat = 1, fM = 2, fK = 4, fFlags = 8, fText = 16, fRange = 32, fCount = 64, fOut = 128, fEnds = 256, fStarts = 512, fSetK = 1024 };
struct Form {
    std::string name;
    unsigned fields;
    std::function<void(Args&)> apply;
};
using Slot = std::vector<Form>;

static std::vector<Slot> checks_of(const Call& c)
{
    const Form pat_null{"pat_null", fPat, [](Args& a) { a.pat = nullptr; a.set = g_set_null_first; }};
    const Form m_zero{"m_zero", fM, [](Args& a) { a.m = 0; }};
    const Form m_over{"m_over", fM, [&c](Args& a) { a.m = c.max_m + 1; }};
    const Form k_over{"k_over", fK, [&c](Args& a) { a.k = c.max_k + 1; }};
    const Form flag{"undefined_flag", fFlags, [](Args& a) { a.flags = 2; }};
    const Form text_null{"text_null", fText, [](Args& a) { a.text = nullptr; }};
    const Form planes3{"three_planes", fText, [](Args& a) { a.text = &g_ptext[3]; }};
    const Slot range = {{"off_beyond", fRange, [](Args& a) { a.off = kTextN + 1; }},
                        {"n_beyond", fRange, [](Args& a) { a.n = kTextN - a.off + 1; }},
                        {"off_wraps", fRange, [](Args& a) { a.off = ~0ull; a.n = 2; }}};
    const Form count_null{"count_null", fCount, [](Args& a) { a.count = nullptr; }};
    const Form out_null{"out_null", fOut, [](Args& a) { a.out = nullptr; }};
    const Form set_code{"set_code", fPat, [](Args& a) { static uint8_t bad[4] = {1, 2, 0x11, 0x20}; a.pat = bad; }};  // [2] names code 4 of 4 values
    const Form ends_null{"ends_null", fEnds, [](Args& a) { a.ends = nullptr; }};
    const Form starts_null{"starts_null", fStarts, [](Args& a) { a.starts = nullptr; }};
    const Form end_out{"end_outside", fEnds, [](Args& a) { a.ends = g_ends_bad; }};
    const Slot batch_args = {{"P_null", fPat, [](Args& a) { a.set = nullptr; }},
                             {"K_zero", fSetK, [](Args& a) { a.K = 0; }},
                             {c.family == kBatchCount ? "counts_null" : "starts_null", fCount, [](Args& a) { a.count = nullptr; }}};
    const Form batch3{"batch_of_7885_on_three_planes", fText | fSetK | fPat, [](Args& a) { a.text = &g_ptext[3]; a.K = sg::kBatch3Max + 1; a.set = g_set_many.data(); }};
    const Slot pattern = {pat_null, m_zero, m_over};  // check_psearch_args: ONE check, whose message holds m
    const Slot m = {m_zero, m_over};

    std::vector<Slot> s;
    switch (c.family) {
    case kExactCount: s = {pattern, {text_null}, range}; break;  // (count NULL is legal: the times alone)
    case kExactFind: s = {pattern, {text_null}, range, {count_null, out_null}}; break;
    case kBatchCount: s = {batch_args, pattern, {text_null}, range, {batch3}}; break;
    case kBatchFind: s = {batch_args, pattern, {text_null}, range, {out_null}, {batch3}}; break;
    case kPExt:  // check_pext_args: k before the length
        if (c.find) s.push_back({out_null});
        s.push_back({pat_null});
        if (c.has_k) s.push_back({k_over});
        s.insert(s.end(), {m, {text_null}, range, {count_null}});
        if (c.sets) s.push_back({set_code});
        break;
    case kPEdit:
    case kText:
        if (c.find) s.push_back({out_null});
        s.insert(s.end(), {{pat_null}, m, {k_over}});
        if (c.has_flags) s.push_back({flag});
        s.push_back({text_null});
        if (c.family == kPEdit) s.push_back({planes3});
        s.insert(s.end(), {range, {count_null}});
        if (c.family == kPEdit && c.sets) s.push_back({set_code});
        break;
    case kPAlign:
    case kTAlign:
        s = {{ends_null}, {starts_null}, {pat_null}, m, {k_over}, {text_null}};
        if (c.family == kPAlign) s.push_back({planes3});
        s.push_back(range);
        if (c.family == kPAlign && c.sets) s.push_back({set_code});
        s.push_back({end_out});
        break;
    }
    return s;
}

static void order_cases(const Call& c)
{
    const std::vector<Slot> slots = checks_of(c);
    const std::string stem = std::string("order/") + c.name + "/";
    for (size_t i = 0; i < slots.size(); ++i)
        for (const Form& first : slots[i]) {
            Args a = c.valid();
            first.apply(a);
            const Result alone = refused_case(stem + first.name, c, a);
            for (size_t j = i + 1; j < slots.size(); ++j)
                for (const Form& second : slots[j]) {
                    if (first.fields & second.fields) continue;
                    Args both = c.valid();
                    first.apply(both);
                    second.apply(both);
                    const std::string id = stem + first.name + "+" + second.name;
                    if (!refused_case(id, c, both).same_answer(alone)) fail(id, "not the earlier violation's answer");
                }
        }
}

// A valid call that needs a launch: with every kernel linked it comes as far as the device's context — once, after all the
// checks, before any launcher; with none linked a family whose kernels register themselves names kernel and unit and asks for
// no device (the two-plane exact, sets, mis and sets-mis kinds are part of every program: they come as far as before).
static void device_cases(const Call& c)
{
    const bool three_too = c.family != kPEdit && c.family != kPAlign && c.packed();
    for (int planes = 2; planes <= (three_too ? 3 : 2); ++planes)
        for (const bool linked : {true, false}) {
            link_kernels(linked);
            const std::string id = std::string(linked ? "device/" : "missing/") + c.name + (planes == 3 ? "@three_planes" : "");
            const Args a = c.valid(planes);
            const Result r = run_case(id, [&] { return c.fn(a); });
            const bool self_registered = c.family == kPEdit || c.family == kText || c.align() || planes == 3;
            if (r.rc != SMARTGPU_ERR_HIP || r.touched != "-") fail(id, "not SMARTGPU_ERR_HIP with nothing written");
            if (linked || !self_registered) {
                if (r.dev != 1 || r.msg != kMarker) fail(id, "did not come as far as the device's context, once");
            } else if (r.dev || r.msg.find("this program holds no ") == std::string::npos || r.msg.find(" is not linked)") == std::string::npos) {
                fail(id, "no missing-kernel refusal before the device");
            }
        }
    link_kernels(true);
}

// What is answered without a launch and without a device: SMARTGPU_OK (or SMARTGPU_ERR_NOMEM with *count set)
static void answer_case(const std::string& id, const Call& c, const Args& a, long want_rc)
{
    const Result r = run_case(id, [&] { return c.fn(a); });
    if (r.rc != want_rc || r.dev) fail(id, "not answered on the host");
}

static void answer_cases(const Call& c)
{
    const std::string stem = std::string("answer/") + c.name + "/";
    if (c.align()) {
        Args a = c.valid();
        a.nends = 0;
        a.ends = nullptr;
        a.starts = nullptr;
        answer_case(stem + "no_ends", c, a, SMARTGPU_OK);
        return;
    }
    if (c.batch() || c.family == kExactCount) return;  // these ask for the device before they look at the pattern
    Args a = c.valid();
    if (c.starts) { a.n = 3; } else { a.m = 10; a.k = 1; a.n = 8; }
    answer_case(stem + (c.starts ? "m_above_n" : "n_plus_k_below_m"), c, a, SMARTGPU_OK);
    if (c.family == kExactFind || (c.family == kPExt && !c.sets)) {  // 'N', twice: more than k = 1 positions accept nothing
        static const uint8_t foreign[4] = {'A', 'N', 'N', 'C'};
        a = c.valid();
        a.pat = foreign;
        answer_case(stem + "foreign_bytes", c, a, SMARTGPU_OK);
    }
    if (c.family == kPExt && c.sets && !c.has_k) {  // full sets: every start position of [10,+50), 47 of them
        static const uint8_t full[4] = {15, 15, 15, 15};
        a = c.valid();
        a.pat = full;
        a.n = 50;
        answer_case(stem + "full_sets", c, a, SMARTGPU_OK);
        if (c.find) {
            a.cap = 46;
            answer_case(stem + "full_sets_cap_one_short", c, a, SMARTGPU_ERR_NOMEM);
        }
    }
}

// ---- the cases of tests/golden/refusal_messages.json that need no live handle: the arguments of that test's call_match ----
static void null_handle_cases(const Call& c)
{
    struct Over { const char* name; bool applies; std::function<void(Args&)> apply; };
    const Over overs[] = {
        {"null_text", true, [](Args&) {}},
        {"null_pattern", true, [](Args& a) { a.pat = nullptr; a.set = g_set_null_first; }},
        {"m_zero", true, [](Args& a) { a.m = 0; }},
        {"m_over", true, [&c](Args& a) { a.m = c.max_m + 1; }},
        {"k_over", c.has_k, [&c](Args& a) { a.k = c.max_k + 1; }},
        {"undefined_flag", c.has_flags, [](Args& a) { a.flags = 2; }},
        {"null_count", !c.align() && !c.batch(), [](Args& a) { a.count = nullptr; }},
        {"null_out_with_cap", c.find, [](Args& a) { a.out = nullptr; }},
        {"null_ends", c.align(), [](Args& a) { a.ends = nullptr; }},
        {"null_starts", c.align(), [](Args& a) { a.starts = nullptr; }},
        {"K_zero", c.batch(), [](Args& a) { a.K = 0; }},
        {"null_P", c.batch(), [](Args& a) { a.set = nullptr; }},
        {c.family == kBatchCount ? "null_counts" : "null_starts", c.batch(), [](Args& a) { a.count = nullptr; }},
    };
    for (const Over& o : overs) {
        if (!o.applies) continue;
        Args a = c.valid();
        a.text = nullptr;
        a.off = 0;
        a.n = 100;
        a.cap = 8;
        a.ends = g_ends_eight;
        a.nends = 8;
        o.apply(a);
        const std::string id = std::string("null/") + c.name + ":" + o.name;
        const Result r = run_case(id, [&] { return c.fn(a); }, true);
        if (r.dev || r.touched != "-") fail(id, "asked for the device or wrote an output");
    }
}

// ---- the calls around the matchers ----
static void other_cases()
{
    uint64_t* bytes = &g_o.count;
    const auto ptr = [](const void* p) -> long { return p != nullptr; };
    // refused without a handle, as tests/test_refusal_messages.py calls them (a pointer or nothing returned: "None")
    run_case("null/ptext_layout:no_values", [&] { return smartgpu_ptext_layout(100, 0, &g_o.planes, bytes); }, true);
    run_case("null/ptext_layout:five_values", [&] { return smartgpu_ptext_layout(100, 5, &g_o.planes, bytes); }, true);
    run_case("null/ptext_layout8:no_values", [&] { return smartgpu_ptext_layout8(100, 0, &g_o.planes, bytes); }, true);
    run_case("null/ptext_layout8:nine_values", [&] { return smartgpu_ptext_layout8(100, 9, &g_o.planes, bytes); }, true);
    run_case("null/ptext_pack:null_text", [&] { return ptr(smartgpu_ptext_pack(nullptr)); }, true, "None");
    run_case("null/ptext_pack8:null_text", [&] { return ptr(smartgpu_ptext_pack8(nullptr)); }, true, "None");
    run_case("null/ptext_free:null_text", [&] { smartgpu_ptext_free(nullptr); return 0; }, true, "None");
    run_case("null/ptext_length:null_text", [&] { return (long)smartgpu_ptext_length(nullptr); }, true);
    run_case("null/ptext_device:null_text", [&] { return smartgpu_ptext_device(nullptr); }, true);
    run_case("null/ptext_planes:null_text", [&] { return smartgpu_ptext_planes(nullptr); }, true);
    run_case("null/ptext_bytes:null_text", [&] { return (long)smartgpu_ptext_bytes(nullptr); }, true);
    run_case("null/ptext_symbols:null_text", [&] { return smartgpu_ptext_symbols(nullptr, g_o.small); }, true);
    run_case("null/ptext_symbols8:null_text", [&] { return smartgpu_ptext_symbols8(nullptr, g_o.small); }, true);
    run_case("null/ptext_read:null_text", [&] { return smartgpu_ptext_read(nullptr, 0, 4, g_o.small); }, true);
    run_case("null/ptext_probe_read_ms:null_text", [&] { return smartgpu_ptext_probe_read_ms(nullptr, 1, &g_o.pre); }, true);
    const uint8_t* acgt = reinterpret_cast<const uint8_t*>("ACGT");
    run_case("null/iupac_sets:null_values", [&] { return smartgpu_iupac_sets(nullptr, 4, "ACGT", 4, g_o.small); }, true);
    run_case("null/iupac_sets:null_sets", [&] { return smartgpu_iupac_sets(acgt, 4, "ACGT", 4, nullptr); }, true);
    run_case("null/iupac_sets:no_values", [&] { return smartgpu_iupac_sets(acgt, 0, "ACGT", 4, g_o.small); }, true);
    run_case("null/iupac_sets:five_values", [&] { return smartgpu_iupac_sets(reinterpret_cast<const uint8_t*>("ACGNT"), 5, "ACGT", 4, g_o.small); }, true);
    run_case("null/iupac_sets:no_letter", [&] { return smartgpu_iupac_sets(acgt, 4, "ACJT", 4, g_o.small); }, true);
    run_case("null/iupac_sets8:null_values", [&] { return smartgpu_iupac_sets8(nullptr, 4, "ACGT", 4, g_o.small); }, true);
    run_case("null/iupac_sets8:nine_values", [&] { return smartgpu_iupac_sets8(reinterpret_cast<const uint8_t*>("-ACGNTXYZ"), 9, "ACGT", 4, g_o.small); }, true);
    run_case("null/iupac_sets8:no_letter", [&] { return smartgpu_iupac_sets8(reinterpret_cast<const uint8_t*>("ACGNT"), 5, "AC!T", 4, g_o.small); }, true);
    run_case("null/iupac_revcomp:null_out", [&] { return smartgpu_iupac_revcomp("ACGT", 4, nullptr); }, true);
    run_case("null/iupac_revcomp:no_letter", [&] { return smartgpu_iupac_revcomp("ACJT", 4, reinterpret_cast<char*>(g_o.small)); }, true);
    // with a live handle
    run_case("handle/ptext_symbols@three_planes", [&] { return smartgpu_ptext_symbols(&g_ptext[3], g_o.small); });
    run_case("handle/ptext_symbols8@three_planes", [&] { return smartgpu_ptext_symbols8(&g_ptext[3], g_o.small); });
    run_case("handle/ptext_symbols@two_planes", [&] { return smartgpu_ptext_symbols(&g_ptext[2], g_o.small); });
    run_case("handle/ptext_length_device_planes", [&] { return (long)smartgpu_ptext_length(&g_ptext[1]) * 100 + smartgpu_ptext_device(&g_ptext[1]) * 10 + smartgpu_ptext_planes(&g_ptext[1]); });
    run_case("handle/ptext_bytes@three_planes", [&] { return (long)smartgpu_ptext_bytes(&g_ptext[3]); });
    run_case("handle/ptext_read:range", [&] { return smartgpu_ptext_read(&g_ptext[2], 98, 3, g_o.small); });
    run_case("handle/ptext_read:nothing", [&] { return smartgpu_ptext_read(&g_ptext[2], 100, 0, nullptr); });
    run_case("device/ptext_read", [&] { return smartgpu_ptext_read(&g_ptext[2], 0, 4, g_o.small); });
    run_case("device/ptext_probe_read_ms", [&] { return smartgpu_ptext_probe_read_ms(&g_ptext[2], 1, &g_o.pre); });
    run_case("device/ptext_pack", [&] { return ptr(smartgpu_ptext_pack(&g_text)); }, false, "None");
    run_case("handle/ptext_pack:six_values", [&] { return ptr(smartgpu_ptext_pack(&g_text6)); }, false, "None");
    run_case("device/ptext_pack8:six_values", [&] { return ptr(smartgpu_ptext_pack8(&g_text6)); }, false, "None");
    link_kernels(false);
    run_case("missing/ptext_pack8:six_values", [&] { return ptr(smartgpu_ptext_pack8(&g_text6)); }, false, "None");
    run_case("missing/ptext_pack8:four_values", [&] { return ptr(smartgpu_ptext_pack8(&g_text)); }, false, "None");
    link_kernels(true);
}

int main()
{
    make_handles();
    std::memcpy(g_bytes, "ACAC", 4);           // bytes every one of the texts holds
    const uint8_t sets[4] = {1, 2, 3, 1};      // codes 0 and 1: every packed text holds them
    std::memcpy(g_sets, sets, 4);
    for (int j = 0; j < 4; ++j) g_classes[32 * j + ("ACAC"[j] >> 3)] = static_cast<uint8_t>(1u << ("ACAC"[j] & 7));
    link_kernels(true);
    for (const Call& c : kCalls) order_cases(c);
    for (const Call& c : kCalls) device_cases(c);
    for (const Call& c : kCalls) answer_cases(c);
    for (const Call& c : kCalls) null_handle_cases(c);
    other_cases();
    fprintf(stderr, "%d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
