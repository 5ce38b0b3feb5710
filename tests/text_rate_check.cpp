// text_rate_check.cpp — tests/test_text_rate.py builds this alone, with AddressSanitizer and UBSan, and runs it: the rate
// of a text from its byte histogram (smart_amd/csrc/text_rate.hpp: text_repeat_rate), the sample a text of n bytes gives
// (rate_sample) and the side of 1/48 a rate lies on (text_rate_streams).  No GPU, no HIP call.
#include "text_rate.hpp"

#include <cmath>
#include <cstdio>

static int g_cases = 0, g_failures = 0;
static void check(bool ok, const char* what, double got, double want)
{
    ++g_cases;
    if (!ok) {
        ++g_failures;
        std::printf("FAIL %s: got %.12g, want %.12g\n", what, got, want);
    }
}

// N bytes spread evenly over the first `values` byte values (the remainder to the lowest ones)
static void uniform(uint64_t counts[256], uint64_t N, uint32_t values)
{
    for (uint32_t c = 0; c < 256; ++c) counts[c] = c < values ? N / values + (c < N % values ? 1 : 0) : 0;
}

int main()
{
    uint64_t counts[256];
    // uniform over 128, 48 and 32 values at N = 2^22: 1/128, 1/48 and 1/32 to within 1e-6
    const uint64_t N = 1ull << 22;
    for (uint32_t values : {128u, 48u, 32u}) {
        uniform(counts, N, values);
        const double got = sg::text_repeat_rate(counts), want = 1.0 / values;
        char what[64];
        std::snprintf(what, sizeof what, "uniform over %u values, N = 2^22", values);
        check(std::fabs(got - want) <= 1e-6, what, got, want);
        // ... and the exact value: every count is N / values (or one more), so the sum is known in closed form
        const long double q = N / values, r = N % values;
        const long double exact = (r * (q + 1) * q + (values - r) * q * (q - 1)) / ((long double)N * (N - 1));
        check(std::fabs(got - (double)exact) <= 1e-15, what, got, (double)exact);
    }
    // the side of 1/48: uniform over 48 values lies a hair BELOW it (unbiased: (q - 1) / (N - 1) with q = N / 48), 47 values above
    uniform(counts, 48 * 1000, 48);
    check(sg::text_rate_streams(sg::text_repeat_rate(counts)), "uniform over 48 values streams", sg::text_repeat_rate(counts), 1.0 / 48);
    uniform(counts, 47 * 1000, 47);
    check(!sg::text_rate_streams(sg::text_repeat_rate(counts)), "uniform over 47 values does not", sg::text_repeat_rate(counts), 1.0 / 47);
    check(sg::text_rate_streams(1.0 / 48) && !sg::text_rate_streams(1.0 / 48 + 1e-9) && sg::text_rate_streams(0.0) && !sg::text_rate_streams(-1.0),
          "text_rate_streams at 1/48, above it, at 0 and without a rate", 0, 0);
    // a single value: every pair is equal
    for (uint64_t n : {2ull, 3ull, 1ull << 24}) {
        uniform(counts, 0, 1);
        counts[200] = n;
        check(sg::text_repeat_rate(counts) == 1.0, "a single value", sg::text_repeat_rate(counts), 1.0);
    }
    // all different: no pair is equal
    uniform(counts, 256, 256);
    check(sg::text_repeat_rate(counts) == 0.0, "256 different bytes", sg::text_repeat_rate(counts), 0.0);
    // N = 0 and N = 1: no rate
    uniform(counts, 0, 1);
    check(sg::text_repeat_rate(counts) == -1.0, "N = 0", sg::text_repeat_rate(counts), -1.0);
    counts[7] = 1;
    check(sg::text_repeat_rate(counts) == -1.0, "N = 1", sg::text_repeat_rate(counts), -1.0);
    // counts near 2^32: c (c - 1) is near 2^64 and the sum of four of them beyond it
    {
        uniform(counts, 0, 1);
        const uint64_t c = 0xFFFFFFFFull;  // 2^32 - 1
        counts[0] = counts[1] = counts[128] = counts[255] = c;
        const long double n = 4.0L * c;
        const long double want = 4.0L * c * (c - 1) / (n * (n - 1));  // a hair below 1/4
        const double got = sg::text_repeat_rate(counts);
        check(std::fabs(got - (double)want) <= 1e-15 && got < 0.25 && got > 0.2499999, "four counts of 2^32 - 1", got, (double)want);
        counts[3] = 1ull << 33;  // and one count beyond 2^32
        const long double k = (long double)(1ull << 33), n2 = n + k;
        const long double want2 = (4.0L * c * (c - 1) + k * (k - 1)) / (n2 * (n2 - 1));
        check(std::fabs(sg::text_repeat_rate(counts) - (double)want2) <= 1e-15, "with a count of 2^33", sg::text_repeat_rate(counts), (double)want2);
    }
    // the sample: whole up to 16 MiB (the last n % 16 bytes included), 2^20 chunks at an even stride beyond, all inside the text
    for (uint64_t n : {0ull, 1ull, 15ull, 16ull, 17ull, 5000ull, 49929ull, (16ull << 20) - 1, 16ull << 20, (16ull << 20) + 15}) {
        const sg::RateSample s = sg::rate_sample(n);
        bool whole = s.bytes() == n && s.chunks == n / 16 && s.tail == n % 16;
        for (uint64_t j : {(uint64_t)0, s.chunks / 2, s.chunks ? s.chunks - 1 : 0}) whole = whole && sg::rate_chunk_at(j, s.step) == j;
        check(whole, "a text of up to 16 MiB is counted whole", (double)s.bytes(), (double)n);
    }
    for (uint64_t n : {(16ull << 20) + 16, 17ull << 20, (32ull << 20) - 1, 32ull << 20, 1ull << 30, (1ull << 30) + 31, (1ull << 35) + 12345, 1ull << 40}) {
        const sg::RateSample s = sg::rate_sample(n);
        // 2^20 chunks, ascending and apart, the first at the text's start, the last inside its last 2^-20th: an EVEN stride
        bool even = s.chunks == sg::kRateChunks && s.tail == 0 && sg::rate_chunk_at(0, s.step) == 0;
        uint64_t prev = 0;
        for (uint64_t j = 1; j < s.chunks; ++j) {
            const uint64_t at = sg::rate_chunk_at(j, s.step);
            even = even && at > prev && at - prev <= n / 16 / sg::kRateChunks + 1;
            prev = at;
        }
        const uint64_t last_end = (prev + 1) * 16;
        check(even && last_end <= n && last_end + (n / sg::kRateChunks + 32) > n, "a longer text gives 2^20 chunks spread over all of it", (double)last_end, (double)n);
    }
    std::printf("%d cases, %d failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
