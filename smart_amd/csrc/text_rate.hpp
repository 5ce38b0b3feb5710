// text_rate.hpp — how often two symbols of a TEXT are equal, from a byte histogram of a sample of it: what api.cpp
// build_blob can only guess from a pattern (a plan cannot see the text), measured once when a text is created
// (api.cpp text_alphabet; the kernel is text_histogram, k_util.hip).  Host-only and free of HIP: tests/text_rate_check.cpp
// compiles it alone.
#pragma once
#include <cstdint>

namespace sg {

// The sample: chunks of 16 bytes at an even stride, at most kRateChunks of them.  A text of up to 16 MiB is counted
// whole, its last n % 16 bytes included, so what a small text reports does not depend on a stride.
constexpr uint64_t kRateChunk = 16;
constexpr uint64_t kRateChunks = 1ull << 20;
// The stride is a fixed-point number (20 fraction bits), so that the chunks of a text of 17 MiB are spread over all of it
// and not over its first 16 MiB: a whole-numbered stride leaves out up to half of a text.
struct RateSample {
    uint64_t chunks;  // 16-byte chunks counted: chunk j is text[16 * at(j), + 16)
    uint64_t step;    // the stride in chunks, times 2^20: 2^20 where the text is counted whole, n / 16 beyond
    uint32_t tail;    // bytes counted behind the last whole chunk of the text (a text that is counted whole), 0..15
    uint64_t bytes() const { return chunks * kRateChunk + tail; }
};
#ifdef __HIP__  // (the kernel calls this one; the attributes by their own names: this header includes nothing of HIP)
__attribute__((host)) __attribute__((device))
#endif
inline uint64_t rate_chunk_at(uint64_t j, uint64_t step) { return (j * step) >> 20; }  // j < 2^20, step < 2^44: a text below 2^48 bytes
inline RateSample rate_sample(uint64_t n)
{
    const uint64_t n16 = n / kRateChunk;
    if (n16 <= kRateChunks) return RateSample{n16, kRateChunks, static_cast<uint32_t>(n % kRateChunk)};
    return RateSample{kRateChunks, n16, 0};  // at(j) = j n16 / 2^20 < n16 for j < 2^20: every chunk lies in the text
}

// rate = sum c (c - 1) / (N (N - 1)) over the 256 counts, N their sum: the chance that two bytes drawn from the sample
// without replacement are equal — the unbiased form build_blob uses on a pattern's own histogram.  -1: no rate (fewer
// than two bytes).  A count may be near 2^32 and beyond, so c (c - 1) and the sum take 128 bits.
inline double text_repeat_rate(const uint64_t counts[256])
{
    unsigned __int128 pairs = 0, total = 0;
    for (int c = 0; c < 256; ++c) {
        const unsigned __int128 k = counts[c];
        total += k;
        if (k) pairs += k * (k - 1);
    }
    if (total < 2) return -1.0;
    return static_cast<double>(static_cast<long double>(pairs) / (static_cast<long double>(total) * static_cast<long double>(total - 1)));
}

// The launcher of text_histogram (k_util.hip), reached through a pointer that the unit's own static initialiser sets
// and api.cpp holds, as k_horm.hip's launcher is (multi.hpp).  In the library it is never null.  The pointer is there
// for the one program that includes api.cpp WITHOUT k_util.hip: tests/dispatch_driver.cpp defines a stub for every
// launcher api.cpp names (launch_text_alphabet among them) and would not link against one more name; with a pointer
// it links as it stands, creates no text, and the null test in text_alphabet is what keeps that case defined.  A
// declaration next to launch_text_alphabet in kernels.hpp would also have changed the source hash of every kernel
// unit (smart_amd/sources.py), to which measured traffic is bound.  Written without HIP's types so that this header
// stays free of them and compiles alone: `stream` is a hipStream_t, the result a hipError_t.  out: 256 zeroed u64 on
// the device.
extern int (*g_text_histogram)(const uint8_t* text, uint64_t n, unsigned long long* out, int num_cus, void* stream);

// Above this rate a skip loop meets a candidate every few windows (build_blob's rule); at or below
// it the windows of ANY pattern die on their first bytes, one whose own symbols repeat included.
inline bool text_rate_streams(double rate) { return rate >= 0.0 && rate * 48.0 <= 1.0; }

}  // namespace sg
