// host_ctx.hpp — what the host units of the C ABI share: api.cpp (texts, plans, the launch queue, the exact calls on byte
// texts) defines all of it, match_calls.cpp (packed texts, the approximate matchers) and align_calls.cpp (the align calls) use
// it, through call_host.hpp.  Host only, included by those three and by no kernel unit.  The two handles are plain structs, so
// that a program without a device can fill them in (tests/host_calls_check.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/smartgpu.h"
#include "kernels.hpp"
#include "planes.hpp"

#pragma GCC visibility push(hidden)  // as when all of this lived in api.cpp: no symbol of the library's

// the text of smartgpu_last_error(), per thread
void set_error(const char* fmt, ...);

#define HIP_TRY(expr, fail)                                                          \
    do {                                                                             \
        hipError_t e_ = (expr);                                                      \
        if (e_ != hipSuccess) {                                                      \
            set_error("%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            fail;                                                                    \
        }                                                                            \
    } while (0)

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

// device_ctx for an entry point that waits for the device's stream or puts work of its own on it: nothing is queued
DeviceCtx* device_ctx_flushed(int device);

// make sure the device's batch arena holds `blob_bytes` of tables and `k` counts
bool batch_reserve(DeviceCtx* d, size_t blob_bytes, size_t k);

// The device buffer of `cap` positions for a find.  Up to kFindKeep entries it is the device's own, grown when a call needs
// more and kept (no hipMalloc per call: a find on a packed text takes less time than an allocation); a larger one is the
// call's (*own, to be freed by the caller).
constexpr size_t kFindKeep = size_t(8) << 20;  // entries: 64 MiB
unsigned long long* find_reserve(DeviceCtx* d, uint64_t cap, bool* own);

// Positions from the device to the caller's (pageable) memory through the device's pinned staging buffer, part by part
// (no overlap of copy and memcpy): a hipMemcpy into pageable memory stages as well, through buffers it sets up per call.
// The staging buffer is free: the patterns it held have been launched and the stream is synchronised.
bool copy_positions(DeviceCtx* d, uint64_t* dst, const unsigned long long* src, uint64_t count);

double now_ms();

// `reps` passes of probe_read over [first, first + bytes) after one warm-up pass, timed by two events of its own: both
// are released on every path
int probe_read_ms(const DeviceCtx* d, const uint8_t* first, uint64_t bytes, unsigned long long* sink, int reps, double* ms_per_pass);

// What a count call answers: the times for smartgpu_last_times, the count and the times for the caller (each where the
// pointer is not null).  Returns SMARTGPU_OK.
int pcount_done(uint64_t c, double pre, double run, uint64_t* count, double* pre_ms, double* run_ms);

#pragma GCC visibility pop

struct smartgpu_text {
    int device = 0;
    uint64_t n = 0;
    uint8_t* base = nullptr;  // allocation start; text byte 0 at base + kFrontPad
    const uint8_t* data() const { return base + sg::kFrontPad; }
    // what the text consists of, taken once when it is created (api.cpp: text_alphabet): the byte values that occur, and
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
