// k_hors.hip — hor_sample_scan: the patterns of a shared pass (m >= 31) counted over the text's SAMPLE, and
// text_sample_build, which writes the sample when a text is created (a translation unit of its own: dev_common.hpp
// says why; sample.hpp has the layout, the rule and the proof that the count is exact)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "sample.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// The sample: dword k is T[28k .. 28k + 4), an aligned dword of the text (text byte 0 is 256-byte aligned).  Every
// 128-byte line of the text holds four or five of them, so the pass reads the text once, like text_alphabet.  The
// dwords behind sample_count(n) are zero.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void text_sample_build(const uint8_t* text, uint64_t count, uint64_t alloc, uint32_t* sample)
{
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < alloc; k += step)
        sample[k] = k < count ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(text + k * kSampleStride)) : 0u;
}

static hipError_t launch_sample_build(const uint8_t* text, uint64_t n, uint32_t* sample, int num_cus, hipStream_t stream)
{
    const uint64_t alloc = sample_alloc_dwords(n), want = (alloc + 255) / 256;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)num_cus * 16));
    hipLaunchKernelGGL(text_sample_build, dim3(grid), dim3(256), 0, stream, text, sample_count(n), alloc, sample);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// hor_sample_scan.  One workgroup of 1024 threads per CU.  Prologue, in LDS: a bit filter of 2^19 bits, 4096 chain
// heads, and for every pattern j of the pass and every offset i < 28 an entry (gram P_j[i .. i + 4), j, i, next), linked
// into the chain of its gram's bucket with one exchange; thread g < np keeps the result slot of pattern g in registers.
// The grams come from the rows in the arguments (by value) or from the front of each pattern's blob (a long pass); a
// thread reads its up to seven grams before it clears anything.
// Main loop: a workgroup owns a contiguous share of the sample's 16-byte quads, in rows of 1024; a lane loads a quad —
// four grams — of each of kHorsInFlight rows and the next step's quads before it looks at this step's.  No tile is
// staged and no barrier stands in the loop.  Per gram: a hash, an LDS read, a bit test; the bits of a step's sixteen
// grams collect in a mask, and the (rare) set bits are taken one at a time: the chain of the gram's bucket is walked
// and ONLY an entry whose stored gram equals the sample's goes on to memory — the range test of sample_window, then
// the text at s = p - i against the whole pattern in its blob.  About 1 % of the samples pass the filter; nearly all of
// them are aliases and end on the compare of two dwords in LDS.
// Patterns longer than kHorsLaneVerify: a lane parks its first gram-equal candidate of a step and the wave compares the
// parked windows together, 1 KiB per step (as hor_multi_scan does); further candidates of that lane and step are
// compared by the lane itself.  Parking is a choice of who compares: no candidate is dropped.
// Counts: an occurrence adds to its pattern's u32 counter in LDS; a workgroup sees each window at most once per pattern
// and the launcher gives no workgroup more than 2^15 rows (2^27 samples, under 2^32 windows).  At the end each workgroup
// adds its non-zero sums to the result slots.  All positions are 64-bit.
// ---------------------------------------------------------------------------
constexpr int kHorsInFlight = 4;
constexpr uint32_t kHorsLaneVerify = 64;  // up to here a lane compares its own window: at most four dependent reads
constexpr uint32_t kHorsGramsPerThread = (kSampleLongWidth * kSampleStride + kSampleThreads - 1) / kSampleThreads;

__device__ __forceinline__ const uint8_t* hors_global(unsigned long long v)
{
    typedef const __attribute__((address_space(1))) uint8_t* global_u8;
    return (const uint8_t*)reinterpret_cast<global_u8>(v);
}
__device__ __forceinline__ unsigned long long hors_area64(const MultiArgs& a, uint32_t at)
{
    return *reinterpret_cast<const unsigned long long*>(a.area + at);
}
__device__ __forceinline__ unsigned long long hors_lane(unsigned long long v, int src)
{
    // (through uint32_t: the builtin returns int, and an int OR-ed into 64 bits is sign-extended)
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, src), hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}
// the parked windows of a wave, one at a time, 16 bytes per lane and step; 1 in the lane whose window equals its pattern
__device__ __forceinline__ uint32_t hors_wave_verify(bool has, const uint8_t* tptr, const uint8_t* pptr, uint32_t len)
{
    unsigned long long todo = __ballot(has);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t mine = 0;
    while (todo) {
        const int src = __builtin_ctzll(todo);  // wave-uniform
        todo &= todo - 1;
        const uint8_t* t = hors_global(hors_lane((unsigned long long)tptr, src));
        const uint8_t* p = hors_global(hors_lane((unsigned long long)pptr, src));
        bool diff = false;
        for (uint32_t off = lane * 16u; off < len; off += 1024u)
            diff |= differ16(t + off, p + off, len - off < 16 ? len - off : 16u);
        if (!__any(diff) && lane == (uint32_t)src) mine = 1;
    }
    return mine;
}

// a quad of the sample: read once per pass, non-temporal like every once-read tile.  (The default cache policy, which
// could keep a sample of 146 MB in the Infinity Cache between passes, measured the same: profiles/coalesce/RESULTS.md.)
__device__ __forceinline__ uint4 hors_quad(const uint32_t* sample, uint64_t q)
{
    return ld_stream16(reinterpret_cast<const uint8_t*>(sample + 4 * q));
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void hor_sample_scan(MultiArgs a, const uint32_t* sample)
{
    static_assert(THREADS == (int)kSampleThreads, "sample.hpp counts the LDS and the widths for this workgroup");
    constexpr int U = kHorsInFlight;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t m = a.m, np = a.np, W = a.width;
    const bool by_value = a.reserved == kMultiByValue;
    uint32_t* filter = reinterpret_cast<uint32_t*>(smem);
    uint32_t* heads = filter + kSampleFilterWords;
    SampleEntry* entries = reinterpret_cast<SampleEntry*>(heads + kSampleBuckets);
    uint32_t* sums = reinterpret_cast<uint32_t*>(entries + np * kSampleStride);

    // what this thread takes of the arguments: the result slot of pattern g (thread g < np) and the grams it enters
    unsigned long long head_count = 0;
    if (threadIdx.x < np) head_count = hors_area64(a, multi_count_at(W, threadIdx.x));
    const uint32_t ngrams = np * kSampleStride;
    uint32_t mine[kHorsGramsPerThread];
#pragma unroll
    for (uint32_t r = 0; r < kHorsGramsPerThread; ++r) {
        const uint32_t idx = threadIdx.x + r * THREADS;
        mine[r] = 0;
        if (idx < ngrams) {
            const uint32_t j = idx / kSampleStride, i = idx - j * kSampleStride;
            // (two reads, not one pointer chosen between the arguments and memory: that one would no longer be a global pointer)
            if (by_value) mine[r] = sample_row_gram(a.area + multi_rows_at(W) + j * kSampleRow, i);
            else mine[r] = sample_row_gram(hors_global(hors_area64(a, multi_blob_at(j))), i);
        }
    }

    // the workgroup's share of the quads [q_first, q_end): rows [r, r1) of THREADS quads
    const uint64_t q_first = sample_quad_first(a.s_begin), q_end = sample_quad_end(a.s_end);
    const uint64_t rows = (q_end - q_first + THREADS - 1) / THREADS;
    const uint64_t per = (rows + gridDim.x - 1) / gridDim.x;
    uint64_t r = (uint64_t)blockIdx.x * per;
    const uint64_t r1 = r + per < rows ? r + per : rows;
    uint4 v[U], w[U];  // this step's quads and the next step's
    uint32_t okv = 0, okw = 0;  // which of them exist (bit u)
    auto issue = [&](uint64_t row, uint4 (&dst)[U], uint32_t& ok) {
        ok = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t q = q_first + (row + u) * THREADS + threadIdx.x;
            dst[u] = uint4{0, 0, 0, 0};
            if (row + u < r1 && q < q_end) {
                dst[u] = hors_quad(sample, q);
                ok |= 1u << u;
            }
        }
    };
    if (r < r1) issue(r, v, okv);

    // the filter, the heads and the sums cleared; a barrier; the entries
    {
        const uint4 zero = {0, 0, 0, 0};
        for (uint32_t j = threadIdx.x * 4u; j < kSampleFilterWords + kSampleBuckets; j += THREADS * 4u) *reinterpret_cast<uint4*>(filter + j) = zero;
        if (threadIdx.x < np) sums[threadIdx.x] = 0;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kHorsGramsPerThread; ++k) {
        const uint32_t idx = threadIdx.x + k * THREADS;
        if (idx < ngrams) {
            const uint32_t j = idx / kSampleStride, i = idx - j * kSampleStride;
            const uint32_t h = sample_hash(mine[k]);
            atomicOr(filter + sample_filter_word(h), sample_filter_bit(h));
            const uint32_t next = atomicExch(heads + sample_bucket(h), idx + 1u);
            entries[idx] = SampleEntry{mine[k], sample_link(j, i, next)};
        }
    }
    __syncthreads();

    const bool wave_wide = m > kHorsLaneVerify;
    for (; r < r1; r += U) {
        if (r + U < r1) issue(r + U, w, okw); else okw = 0;
        // the filter: bit 4u + c of the mask for gram c of quad u
        uint32_t mask = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t g[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t h = sample_hash(g[c]);
                mask |= ((filter[sample_filter_word(h)] >> (h & 31u)) & 1u) << (4 * u + c);
            }
        }
        // (a quad that does not exist is zeros: its bits are dropped here, whatever the filter says of gram 0)
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (!(okv >> u & 1u)) mask &= ~(0xFu << (4 * u));
        const uint64_t k0 = 4u * (q_first + r * THREADS + threadIdx.x);  // the sample index of gram 0 of quad 0
        bool parked = false;
        uint32_t parked_j = 0;
        const uint8_t* parked_at = a.text;
        unsigned long long parked_blob = (unsigned long long)a.text;
        while (mask) {
            const uint32_t b = (uint32_t)__builtin_ctz(mask);
            mask &= mask - 1u;
            uint32_t gram = 0;  // gram b of the step, without indexing registers
#pragma unroll
            for (int u = 0; u < U; ++u) {
                gram = b == 4u * u ? v[u].x : gram;
                gram = b == 4u * u + 1u ? v[u].y : gram;
                gram = b == 4u * u + 2u ? v[u].z : gram;
                gram = b == 4u * u + 3u ? v[u].w : gram;
            }
            const uint64_t p = (k0 + (uint64_t)(b >> 2) * (4u * THREADS) + (b & 3u)) * kSampleStride;
            for (uint32_t e = heads[sample_bucket(sample_hash(gram))]; e != 0;) {
                const SampleEntry ent = entries[e - 1u];
                e = sample_link_next(ent.link);
                uint64_t s;
                if (ent.gram != gram || !sample_window(p, sample_link_offset(ent.link), a.s_begin, a.s_end, &s)) continue;
                const uint32_t j = sample_link_pattern(ent.link);
                const unsigned long long blob = hors_area64(a, multi_blob_at(j));
                const uint8_t* at = a.text + s;
                if (wave_wide && !parked) {
                    parked = true;
                    parked_at = at;
                    parked_j = j;
                    parked_blob = blob;
                } else if (global_equal(at, hors_global(blob), m)) {
                    atomicAdd(sums + j, 1u);
                }
            }
        }
        if (wave_wide && hors_wave_verify(parked, parked_at, hors_global(parked_blob), m)) atomicAdd(sums + parked_j, 1u);
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = w[u];
        okv = okw;
    }

    // the workgroup's np sums, each straight to its pattern's result slot
    __syncthreads();
    if (threadIdx.x < np && sums[threadIdx.x] != 0) {
        typedef __attribute__((address_space(1))) unsigned long long* global_u64;
        atomicAdd((unsigned long long*)reinterpret_cast<global_u64>(head_count), (unsigned long long)sums[threadIdx.x]);
    }
}

static hipError_t launch_hor_sample(const MultiArgs& a, const uint32_t* sample, int num_cus, int grid_want, hipStream_t stream)
{
    if (!sample || a.m < kSampleMinM || (a.reserved != kMultiByValue && a.reserved != kMultiLong)) return hipErrorInvalidValue;
    const bool by_value = a.reserved == kMultiByValue;
    if (a.width != (by_value ? kSampleWidth : kSampleLongWidth) || a.stride != kSampleRow || a.np < 1 || a.np > a.width) return hipErrorInvalidValue;
    if (a.s_end <= a.s_begin) return hipSuccess;
    const uint64_t rows = (sample_quad_end(a.s_end) - sample_quad_first(a.s_begin) + kSampleThreads - 1) / kSampleThreads;
    uint64_t grid = grid_want > 0 ? (uint64_t)grid_want : (uint64_t)num_cus;
    if (grid > rows) grid = rows;
    const uint64_t least = (rows + (1u << 15) - 1) >> 15;  // a workgroup's u32 sums: at most 2^15 rows of 2^12 samples of 28 windows each
    if (grid < least) grid = least;
    const size_t lds = sample_lds(a.np);
    const void* kernel = reinterpret_cast<const void*>(&hor_sample_scan<(int)kSampleThreads>);
    allow_lds(kernel, sample_lds(kSampleLongWidth));
    hipLaunchKernelGGL((hor_sample_scan<(int)kSampleThreads>), dim3((uint32_t)grid), dim3(kSampleThreads), lds, stream, a, sample);
    return hipGetLastError();
}

// api.cpp builds samples and sends sampled passes only once this unit is part of the program
namespace {
struct RegisterHorSample {
    RegisterHorSample()
    {
        g_hor_sample = &launch_hor_sample;
        g_sample_build = &launch_sample_build;
    }
} g_register_hor_sample;
}  // namespace

}  // namespace sg
