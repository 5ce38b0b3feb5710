// k_planes.hip — packed texts: planes_pack (byte text -> bit planes, once per text), planes_scan (the matcher on planes),
// planes_find (the same matcher with an output stage: positions), planes_sets_scan / planes_sets_find (their siblings for
// patterns whose positions accept a SET of symbols), planes_mis_scan / planes_mis_find (occurrences with up to k mismatches),
// planes_sets_mis_scan / planes_sets_mis_find (set patterns with up to k mismatches)
// (one translation unit per kernel family: dev_common.hpp; the layout: planes.hpp)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "planes.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// planes_pack: a lane reads 32 consecutive text bytes (two non-temporal 16-byte loads) and forms the dword of each plane
// itself.  The code of a byte is its rank among the text's values: the number of values below it, three compares (v[] = 255
// where the text has fewer values).  Zero bytes of the text's back pad beyond n give code 0: the planes' tail bits are zero.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void planes_pack(const uint8_t* __restrict__ text, uint64_t ndwords, uint32_t* __restrict__ p0,
                                                   uint32_t* __restrict__ p1, uint32_t v0, uint32_t v1, uint32_t v2)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < ndwords; g += stride) {
        const uint4 a = ld_stream16(text + 32 * g), b = ld_stream16(text + 32 * g + 16);
        const uint32_t d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t b0 = 0, b1 = 0;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const uint32_t c = (d[i >> 2] >> (8 * (i & 3))) & 0xFFu;
            const uint32_t code = (uint32_t)(c > v0) + (uint32_t)(c > v1) + (uint32_t)(c > v2);
            b0 |= (code & 1u) << i;
            b1 |= (code >> 1) << i;
        }
        p0[g] = b0;
        if (p1) p1[g] = b1;
    }
}

hipError_t launch_planes_pack(const uint8_t* text, uint64_t n, uint32_t* p0, uint32_t* p1, int planes, const uint8_t values[3],
                              hipStream_t stream)
{
    const uint64_t ndwords = (n + 31) / 32;
    if (ndwords == 0) return hipSuccess;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((ndwords + 255) / 256, 65536);
    hipLaunchKernelGGL(planes_pack, dim3(grid), dim3(256), 0, stream, text, ndwords, p0, planes == 2 ? p1 : nullptr,
                       (uint32_t)values[0], (uint32_t)values[1], (uint32_t)values[2]);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// planes_scan<PLANES>: counts the start positions s in [s_begin, s_end) with T[s + j] == P[j] for all j < m.
//
// A lane owns kChunk = 4 consecutive dwords of start positions — 128 of them — per plane (one non-temporal
// global_load_dwordx4) and keeps a dword M of live positions for each.  Pattern symbol j against the 32 positions of
// dword w is t_b = v_alignbit(plane_b[w + 1], plane_b[w], j) per plane, then ONE three-input bit operation (v_bitop3) chosen by the
// symbol's code, which is wave-uniform (a scalar branch): M &= ~(t0 | t1), t0 & ~t1, ~t0 & t1 or t0 & t1 — three vector
// instructions per 32 positions and symbol on two planes, two on one.  The dword behind the lane's four comes by a second
// (cached) load; a wave's last lane would need it anyway.
// The first 32 symbols (x0, x1: kernel arguments) are taken eight at a time; after each eight the WAVE leaves when none of
// its 8192 positions is live (random text of four values: 0.13 live positions per wave after eight symbols, of two values:
// after sixteen).  Symbols from the 32nd on: planes_verify, the wave together for each lane that has a live position.
// Positions outside [s_begin, s_end) are masked off the range's first and last chunk: the zero pad behind the text looks
// like code 0 and is never counted.
// kUnroll chunks per lane and trip: their loads are issued before any is worked on.
// ---------------------------------------------------------------------------
constexpr int kPlanesT = 256;
constexpr uint32_t kChunk = 4;     // dwords per lane and plane
constexpr int kUnroll = 2;         // chunks per lane and trip of the loop
constexpr int kPlanesWgs = 8;      // workgroups per CU

struct PlaneWords { uint32_t a[kChunk + 1], b[kChunk + 1]; };  // five consecutive dwords of plane 0 / plane 1

// bits i with lo <= p + i < hi
static __device__ __forceinline__ uint32_t range_mask(uint64_t p, uint64_t lo, uint64_t hi)
{
    uint32_t m = ~0u;
    if (lo > p) m = lo - p >= 32 ? 0u : m << (uint32_t)(lo - p);
    if (hi < p + 32) m = hi <= p ? 0u : m & (~0u >> (32u - (uint32_t)(hi - p)));
    return m;
}

// symbols [j0, j1) (j1 <= 32) of a 32-symbol block of the pattern, bits x0 / x1, against the block's five dwords
template <int PLANES>
static __device__ __forceinline__ void planes_kill(uint32_t (&M)[kChunk], const PlaneWords& t, uint32_t x0, uint32_t x1, uint32_t j0, uint32_t j1)
{
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t c = ((x0 >> j) & 1u) | (PLANES == 2 ? ((x1 >> j) & 1u) << 1 : 0u);  // wave-uniform
// M & f(t0, t1) as ONE v_bitop3_b32 (truth table over M = 0xF0, t0 = 0xCC, t1 = 0xAA); written with & | ~ the compiler
// emits two or three instructions
#define SG_PLANES_STEP(table_)                                                             \
    _Pragma("unroll") for (uint32_t w = 0; w < kChunk; ++w) {                              \
        const uint32_t t0 = __builtin_amdgcn_alignbit(t.a[w + 1], t.a[w], j);              \
        const uint32_t t1 = PLANES == 2 ? __builtin_amdgcn_alignbit(t.b[w + 1], t.b[w], j) : 0u; \
        M[w] = __builtin_amdgcn_bitop3_b32(M[w], t0, t1, table_);                          \
    }
        if (PLANES == 2) {
            if (c == 0) { SG_PLANES_STEP(0x10) }       // M & ~(t0 | t1)
            else if (c == 1) { SG_PLANES_STEP(0x40) }  // M & t0 & ~t1
            else if (c == 2) { SG_PLANES_STEP(0x20) }  // M & ~t0 & t1
            else { SG_PLANES_STEP(0x80) }              // M & t0 & t1
        } else {
            if (c == 0) { SG_PLANES_STEP(0x30) }       // M & ~t0
            else { SG_PLANES_STEP(0xC0) }              // M & t0
        }
#undef SG_PLANES_STEP
    }
}

// Symbols from the 32nd on, for the live positions of ONE lane's chunk, by the whole wave (every lane is here): a lane
// that walks the pattern's up to 131 further dwords alone pays the latency of its loads 131 times in a row (0.4 ms for ONE
// occurrence of a 4096-symbol pattern — measured: a 1 GiB scan of 50 us then takes 480).  So lane l takes block k0 + l — the
// pattern's symbols 32 k .. 32 k + 31, x0 / x1 from the pattern's planes in memory, and the five text dwords k dwords behind
// the chunk — and the wave goes over the live positions (R: wave-uniform, scalar): position i of dword w survives when in
// every lane the 32 text symbols from it on equal the lane's block, one ballot.
template <int PLANES>
static __device__ __forceinline__ void planes_verify(uint32_t (&R)[kChunk], const PlaneArgs& a, uint64_t dw)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t k0 = 1; 32 * k0 < a.m && (R[0] | R[1] | R[2] | R[3]) != 0; k0 += 64) {
        const bool valid = 32 * (k0 + lane) < a.m;
        const uint32_t k = valid ? k0 + lane : k0;
        const uint32_t left = a.m - 32 * k;
        const uint32_t bmask = !valid ? 0u : left >= 32 ? ~0u : (1u << left) - 1u;  // the pattern's last block may be partial
        uint32_t ta[kChunk + 1], tb[kChunk + 1];
        __builtin_memcpy(ta, a.p0 + dw + k, 4 * (kChunk + 1));
        if (PLANES == 2) __builtin_memcpy(tb, a.p1 + dw + k, 4 * (kChunk + 1));
        const uint32_t x0 = a.pat[k], x1 = PLANES == 2 ? a.pat[kPatWords + k] : 0u;
#pragma unroll
        for (uint32_t w = 0; w < kChunk; ++w) {
            uint32_t r = R[w];
            while (r) {
                const uint32_t i = __builtin_ctz(r);
                r &= r - 1;
                uint32_t d = __builtin_amdgcn_alignbit(ta[w + 1], ta[w], i) ^ x0;
                if (PLANES == 2) d |= __builtin_amdgcn_alignbit(tb[w + 1], tb[w], i) ^ x1;
                if (__any((d & bmask) != 0)) R[w] &= ~(1u << i);
            }
        }
    }
}

template <int PLANES>
__global__ __launch_bounds__(kPlanesT, 8) void planes_scan(PlaneArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // 128 bytes: flush_hits
    constexpr uint64_t kPos = 32 * kChunk;                          // start positions per chunk
    const uint64_t c_end = (a.s_end + kPos - 1) / kPos;
    const uint64_t stride = (uint64_t)gridDim.x * kPlanesT * kUnroll;
    const uint32_t f1 = a.m < 32 ? a.m : 32u;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t hits = 0;
    // the trip count is the WAVE's (its first chunk decides): every lane stays for the ballots and the verification
    for (uint64_t cw = a.s_begin / kPos + (uint64_t)blockIdx.x * kPlanesT * kUnroll + 64u * wave; cw < c_end; cw += stride) {
        PlaneWords t[kUnroll];
        uint32_t M[kUnroll][kChunk];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const uint64_t c = cw + (uint64_t)u * kPlanesT + lane;
            const bool in = c < c_end;
            const uint64_t dw = in ? c * kChunk : 0;
            const uint4 va = ld_stream16(reinterpret_cast<const uint8_t*>(a.p0 + dw));
            t[u].a[0] = va.x; t[u].a[1] = va.y; t[u].a[2] = va.z; t[u].a[3] = va.w;
            t[u].a[4] = a.p0[dw + kChunk];
            if (PLANES == 2) {
                const uint4 vb = ld_stream16(reinterpret_cast<const uint8_t*>(a.p1 + dw));
                t[u].b[0] = vb.x; t[u].b[1] = vb.y; t[u].b[2] = vb.z; t[u].b[3] = vb.w;
                t[u].b[4] = a.p1[dw + kChunk];
            }
            const bool inner = c * kPos >= a.s_begin && (c + 1) * kPos <= a.s_end;
#pragma unroll
            for (uint32_t w = 0; w < kChunk; ++w)
                M[u][w] = !in ? 0u : inner ? ~0u : range_mask(c * kPos + 32 * w, a.s_begin, a.s_end);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            uint32_t live = 0;
            for (uint32_t j0 = 0; j0 < f1; j0 += 8) {
                planes_kill<PLANES>(M[u], t[u], a.x0, a.x1, j0, j0 + 8 < f1 ? j0 + 8 : f1);
                live = M[u][0] | M[u][1] | M[u][2] | M[u][3];
                if (!__any(live != 0)) break;
            }
            if (a.m > 32) {  // rarely: a lane has live positions after 32 symbols
                unsigned long long todo = __ballot(live != 0);
                while (todo) {
                    const int src = __builtin_ctzll(todo);  // wave-uniform
                    todo &= todo - 1;
                    const uint64_t dw = (cw + (uint64_t)u * kPlanesT + (uint32_t)src) * kChunk;
                    uint32_t R[kChunk];
#pragma unroll
                    for (uint32_t w = 0; w < kChunk; ++w) R[w] = __builtin_amdgcn_readlane(M[u][w], src);
                    planes_verify<PLANES>(R, a, dw);
                    if (lane == (uint32_t)src) {
#pragma unroll
                        for (uint32_t w = 0; w < kChunk; ++w) M[u][w] = R[w];
                    }
                }
            }
#pragma unroll
            for (uint32_t w = 0; w < kChunk; ++w) hits += __builtin_popcount(M[u][w]);
        }
    }
    flush_hits(hits, a.count, smem, reinterpret_cast<const uint8_t*>(a.p0));
}

hipError_t launch_planes_scan(const PlaneArgs& a, int planes, int num_cus, hipStream_t stream)
{
    if (a.s_end <= a.s_begin) return hipSuccess;
    constexpr uint64_t kPos = 32 * kChunk;
    const uint64_t chunks = (a.s_end + kPos - 1) / kPos - a.s_begin / kPos;
    const uint64_t want = (chunks + kPlanesT * kUnroll - 1) / (kPlanesT * kUnroll);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(want, (uint64_t)num_cus * kPlanesWgs);
    if (planes == 2)
        hipLaunchKernelGGL(planes_scan<2>, dim3(grid), dim3(kPlanesT), 128, stream, a);
    else
        hipLaunchKernelGGL(planes_scan<1>, dim3(grid), dim3(kPlanesT), 128, stream, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// planes_find<PLANES>: planes_scan with an output stage — the surviving start positions are appended to `out` (relative to
// symbol 0 of the text) and a.count, a 64-bit cursor, receives their number.
//
// The loop skeleton below REPEATS planes_scan's on purpose (about 40 lines; the helpers are shared).  Moving the body into
// one function template <PLANES, FIND> changes planes_scan's instruction stream (940 -> 968 and 1061 -> 1095 instructions
// cross-compiled for gfx950, same registers), and the counting path is measured and documented as it is: the repeated
// skeleton is the price of leaving it untouched.  A change to one of the two loops belongs in the other as well.
//
// The output stage runs once a chunk is final (after planes_verify when m > 32) and only when a lane of the wave has a
// survivor: one wave-uniform branch more than planes_scan for every other chunk.  The lanes' counts (popcount of the four M
// dwords) are prefix-summed inside the wave by shuffles, lane 0 reserves the wave's span of the output with ONE atomicAdd on
// the cursor, the base comes back to every lane by readfirstlane, and each lane stores its positions, ascending, with
// ordinary vector stores while slot < cap.  Entries beyond cap are dropped, the cursor counts them all the same.
// A span — one wave, one chunk row: kFindSpan start positions from the range's first chunk on — is contiguous and ascending
// in `out`; the spans of a launch cover disjoint position ranges and lie in the order their waves reserved them (the host
// orders them by their first entry, match_calls.cpp).  No LDS, no scratch.
// ---------------------------------------------------------------------------
static_assert(kFindSpan == 64 * 32 * kChunk, "a span of planes_find: one wave's lanes, one chunk each");
static_assert(kPlanesT % 64 == 0, "every wave's chunk row starts a multiple of 64 chunks behind the range's first: the host's span number");

template <int PLANES>
__global__ __launch_bounds__(kPlanesT, 8) void planes_find(PlaneArgs a, unsigned long long* __restrict__ out, unsigned long long cap)
{
    constexpr uint64_t kPos = 32 * kChunk;  // start positions per chunk
    const uint64_t c_end = (a.s_end + kPos - 1) / kPos;
    const uint64_t stride = (uint64_t)gridDim.x * kPlanesT * kUnroll;
    const uint32_t f1 = a.m < 32 ? a.m : 32u;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the trip count is the WAVE's (its first chunk decides): every lane stays for the ballots, the verification and the shuffles
    for (uint64_t cw = a.s_begin / kPos + (uint64_t)blockIdx.x * kPlanesT * kUnroll + 64u * wave; cw < c_end; cw += stride) {
        PlaneWords t[kUnroll];
        uint32_t M[kUnroll][kChunk];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const uint64_t c = cw + (uint64_t)u * kPlanesT + lane;
            const bool in = c < c_end;
            const uint64_t dw = in ? c * kChunk : 0;
            const uint4 va = ld_stream16(reinterpret_cast<const uint8_t*>(a.p0 + dw));
            t[u].a[0] = va.x; t[u].a[1] = va.y; t[u].a[2] = va.z; t[u].a[3] = va.w;
            t[u].a[4] = a.p0[dw + kChunk];
            if (PLANES == 2) {
                const uint4 vb = ld_stream16(reinterpret_cast<const uint8_t*>(a.p1 + dw));
                t[u].b[0] = vb.x; t[u].b[1] = vb.y; t[u].b[2] = vb.z; t[u].b[3] = vb.w;
                t[u].b[4] = a.p1[dw + kChunk];
            }
            const bool inner = c * kPos >= a.s_begin && (c + 1) * kPos <= a.s_end;
#pragma unroll
            for (uint32_t w = 0; w < kChunk; ++w)
                M[u][w] = !in ? 0u : inner ? ~0u : range_mask(c * kPos + 32 * w, a.s_begin, a.s_end);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            uint32_t live = 0;
            for (uint32_t j0 = 0; j0 < f1; j0 += 8) {
                planes_kill<PLANES>(M[u], t[u], a.x0, a.x1, j0, j0 + 8 < f1 ? j0 + 8 : f1);
                live = M[u][0] | M[u][1] | M[u][2] | M[u][3];
                if (!__any(live != 0)) break;
            }
            if (a.m > 32) {  // rarely: a lane has live positions after 32 symbols
                unsigned long long todo = __ballot(live != 0);
                while (todo) {
                    const int src = __builtin_ctzll(todo);  // wave-uniform
                    todo &= todo - 1;
                    const uint64_t dw = (cw + (uint64_t)u * kPlanesT + (uint32_t)src) * kChunk;
                    uint32_t R[kChunk];
#pragma unroll
                    for (uint32_t w = 0; w < kChunk; ++w) R[w] = __builtin_amdgcn_readlane(M[u][w], src);
                    planes_verify<PLANES>(R, a, dw);
                    if (lane == (uint32_t)src) {
#pragma unroll
                        for (uint32_t w = 0; w < kChunk; ++w) M[u][w] = R[w];
                    }
                }
                live = M[u][0] | M[u][1] | M[u][2] | M[u][3];
            }
            if (!__any(live != 0)) continue;
            // the output stage: wave-wide exclusive prefix sum of the lanes' counts, one atomic, the lanes' stores
            uint32_t mine = 0;
#pragma unroll
            for (uint32_t w = 0; w < kChunk; ++w) mine += __builtin_popcount(M[u][w]);
            unsigned long long slot = wave_reserve(mine, a.count, lane);
            const uint64_t pos = (cw + (uint64_t)u * kPlanesT + lane) * kPos;
#pragma unroll
            for (uint32_t w = 0; w < kChunk; ++w) {
                uint32_t r = M[u][w];
                while (r) {
                    const uint32_t i = __builtin_ctz(r);
                    r &= r - 1;
                    if (slot < cap) out[slot] = pos + 32 * w + i;
                    ++slot;
                }
            }
        }
    }
}

// Grid and occupancy: launch_planes_scan's.
hipError_t launch_planes_find(const PlaneArgs& a, unsigned long long* out, unsigned long long cap, int planes, int num_cus,
                              hipStream_t stream)
{
    if (a.s_end <= a.s_begin) return hipSuccess;
    constexpr uint64_t kPos = 32 * kChunk;
    const uint64_t chunks = (a.s_end + kPos - 1) / kPos - a.s_begin / kPos;
    const uint64_t want = (chunks + kPlanesT * kUnroll - 1) / (kPlanesT * kUnroll);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(want, (uint64_t)num_cus * kPlanesWgs);
    if (planes == 2)
        hipLaunchKernelGGL(planes_find<2>, dim3(grid), dim3(kPlanesT), 0, stream, a, out, cap);
    else
        hipLaunchKernelGGL(planes_find<1>, dim3(grid), dim3(kPlanesT), 0, stream, a, out, cap);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// planes_sets_scan<PLANES>, planes_sets_find<PLANES>: SET patterns — position j of the pattern accepts a set of codes.
// They count / list the start positions s in [s_begin, s_end) where the code of T[s + j] is a member of set j for all
// j < m.  Siblings of planes_scan and planes_find: the same geometry, loads, range masks, early leave and output stage;
// what differs is the step per pattern position and the verification beyond the 32nd.
//
// planes_kill picks one of four truth tables by the symbol's code.  A set's table is the OR of its members' tables, so a
// position costs the same v_alignbit per plane and ONE v_bitop3 whatever the set is (fewer where the table does not
// depend on a plane: the compiler drops that plane's v_alignbit), and a position that accepts every code costs nothing.
// The set of position j — bit j of y[0..3] — is wave-uniform: a scalar switch, one case per table.
//
// The two kernels share ONE body (planes_sets_body<PLANES, FIND>, if constexpr): unlike planes_scan, whose instruction
// stream is documented and measured, neither has a stream to preserve.  planes_scan and planes_find are not touched.
// ---------------------------------------------------------------------------
// the table of M & "the code (t1 t0) is a member of s" over M = 0xF0, t0 = 0xCC, t1 = 0xAA
constexpr uint32_t sets_table(int planes, uint32_t s)
{
    return planes == 2 ? ((s & 1u ? 0x10u : 0u) | (s & 2u ? 0x40u : 0u) | (s & 4u ? 0x20u : 0u) | (s & 8u ? 0x80u : 0u))
                       : ((s & 1u ? 0x30u : 0u) | (s & 2u ? 0xC0u : 0u));
}

template <int PLANES, uint32_t TABLE>
static __device__ __forceinline__ void planes_sets_step(uint32_t (&M)[kChunk], const PlaneWords& t, uint32_t j)
{
#pragma unroll
    for (uint32_t w = 0; w < kChunk; ++w) {
        const uint32_t t0 = __builtin_amdgcn_alignbit(t.a[w + 1], t.a[w], j);
        const uint32_t t1 = PLANES == 2 ? __builtin_amdgcn_alignbit(t.b[w + 1], t.b[w], j) : 0u;
        M[w] = __builtin_amdgcn_bitop3_b32(M[w], t0, t1, TABLE);
    }
}

// positions [j0, j1) (j1 <= 32) of the pattern's first block, membership bits y[c], against the block's five dwords
template <int PLANES>
static __device__ __forceinline__ void planes_sets_kill(uint32_t (&M)[kChunk], const PlaneWords& t, const uint32_t (&y)[4], uint32_t j0, uint32_t j1)
{
    for (uint32_t j = j0; j < j1; ++j) {
        uint32_t s = ((y[0] >> j) & 1u) | ((y[1] >> j) & 1u) << 1;  // wave-uniform
        if (PLANES == 2) s |= ((y[2] >> j) & 1u) << 2 | ((y[3] >> j) & 1u) << 3;
#define SG_SETS_CASE(s_) case s_: planes_sets_step<PLANES, sets_table(PLANES, s_)>(M, t, j); break;
        if (PLANES == 2) {
            switch (s) {
                SG_SETS_CASE(1) SG_SETS_CASE(2) SG_SETS_CASE(3) SG_SETS_CASE(4) SG_SETS_CASE(5) SG_SETS_CASE(6) SG_SETS_CASE(7)
                SG_SETS_CASE(8) SG_SETS_CASE(9) SG_SETS_CASE(10) SG_SETS_CASE(11) SG_SETS_CASE(12) SG_SETS_CASE(13) SG_SETS_CASE(14)
                case 0: M[0] = M[1] = M[2] = M[3] = 0u; break;  // (the host sends no empty set)
                default: break;                                  // every code: no instruction
            }
        } else {
            switch (s) {
                SG_SETS_CASE(1) SG_SETS_CASE(2)
                case 0: M[0] = M[1] = M[2] = M[3] = 0u; break;
                default: break;
            }
        }
#undef SG_SETS_CASE
    }
}

// planes_verify for sets: lane l takes block k0 + l of the pattern — the membership dwords Y0..Y3[k] (Y0, Y1 on one
// plane) — and the five text dwords k dwords behind the chunk.  Bit b of `acc` says that the text symbol b behind the live
// position is accepted by position 32 k + b: the Y dword its code selects, bit by bit — a two-level multiplexer, three
// v_bitop3 on two planes (four Y dwords and two text dwords are six inputs: two three-input operations cannot take them),
// one on one plane.  Positions beyond the pattern's end (the last block may be partial, lanes beyond the last block)
// accept everything: ~bmask is ORed into the Y dwords once per block.  One ballot per live position.
template <int PLANES>
static __device__ __forceinline__ void planes_sets_verify(uint32_t (&R)[kChunk], const PlaneSetArgs& a, uint64_t dw)
{
    constexpr uint32_t kMux = 0xCA;  // bitop3(sel, one, zero): sel ? one : zero, bit by bit
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t k0 = 1; 32 * k0 < a.m && (R[0] | R[1] | R[2] | R[3]) != 0; k0 += 64) {
        const bool valid = 32 * (k0 + lane) < a.m;
        const uint32_t k = valid ? k0 + lane : k0;
        const uint32_t left = a.m - 32 * k;
        const uint32_t bmask = !valid ? 0u : left >= 32 ? ~0u : (1u << left) - 1u;
        uint32_t ta[kChunk + 1], tb[kChunk + 1];
        __builtin_memcpy(ta, a.p0 + dw + k, 4 * (kChunk + 1));
        if (PLANES == 2) __builtin_memcpy(tb, a.p1 + dw + k, 4 * (kChunk + 1));
        const uint32_t y0 = a.pat[k] | ~bmask, y1 = a.pat[kPatWords + k] | ~bmask;
        const uint32_t y2 = PLANES == 2 ? a.pat[2 * kPatWords + k] | ~bmask : 0u;
        const uint32_t y3 = PLANES == 2 ? a.pat[3 * kPatWords + k] | ~bmask : 0u;
#pragma unroll
        for (uint32_t w = 0; w < kChunk; ++w) {
            uint32_t r = R[w];
            while (r) {
                const uint32_t i = __builtin_ctz(r);
                r &= r - 1;
                const uint32_t t0 = __builtin_amdgcn_alignbit(ta[w + 1], ta[w], i);
                uint32_t acc = __builtin_amdgcn_bitop3_b32(t0, y1, y0, kMux);
                if (PLANES == 2) {
                    const uint32_t t1 = __builtin_amdgcn_alignbit(tb[w + 1], tb[w], i);
                    acc = __builtin_amdgcn_bitop3_b32(t1, __builtin_amdgcn_bitop3_b32(t0, y3, y2, kMux), acc, kMux);
                }
                if (__any(acc != ~0u)) R[w] &= ~(1u << i);
            }
        }
    }
}

// The loop skeleton is planes_scan's (FIND = false) and planes_find's (FIND = true): a change to one of those belongs here
// as well.  smem: flush_hits' 128 bytes (the scan only).
template <int PLANES, bool FIND>
static __device__ __forceinline__ void planes_sets_body(const PlaneSetArgs& a, uint8_t* smem, unsigned long long* __restrict__ out,
                                                        unsigned long long cap)
{
    constexpr uint64_t kPos = 32 * kChunk;  // start positions per chunk
    const uint64_t c_end = (a.s_end + kPos - 1) / kPos;
    const uint64_t stride = (uint64_t)gridDim.x * kPlanesT * kUnroll;
    const uint32_t f1 = a.m < 32 ? a.m : 32u;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t hits = 0;
    // the trip count is the WAVE's (its first chunk decides): every lane stays for the ballots, the verification and the shuffles
    for (uint64_t cw = a.s_begin / kPos + (uint64_t)blockIdx.x * kPlanesT * kUnroll + 64u * wave; cw < c_end; cw += stride) {
        PlaneWords t[kUnroll];
        uint32_t M[kUnroll][kChunk];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const uint64_t c = cw + (uint64_t)u * kPlanesT + lane;
            const bool in = c < c_end;
            const uint64_t dw = in ? c * kChunk : 0;
            const uint4 va = ld_stream16(reinterpret_cast<const uint8_t*>(a.p0 + dw));
            t[u].a[0] = va.x; t[u].a[1] = va.y; t[u].a[2] = va.z; t[u].a[3] = va.w;
            t[u].a[4] = a.p0[dw + kChunk];
            if (PLANES == 2) {
                const uint4 vb = ld_stream16(reinterpret_cast<const uint8_t*>(a.p1 + dw));
                t[u].b[0] = vb.x; t[u].b[1] = vb.y; t[u].b[2] = vb.z; t[u].b[3] = vb.w;
                t[u].b[4] = a.p1[dw + kChunk];
            }
            const bool inner = c * kPos >= a.s_begin && (c + 1) * kPos <= a.s_end;
#pragma unroll
            for (uint32_t w = 0; w < kChunk; ++w)
                M[u][w] = !in ? 0u : inner ? ~0u : range_mask(c * kPos + 32 * w, a.s_begin, a.s_end);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            uint32_t live = 0;
            for (uint32_t j0 = 0; j0 < f1; j0 += 8) {
                planes_sets_kill<PLANES>(M[u], t[u], a.y, j0, j0 + 8 < f1 ? j0 + 8 : f1);
                live = M[u][0] | M[u][1] | M[u][2] | M[u][3];
                if (!__any(live != 0)) break;
            }
            if (a.m > 32) {  // a lane has live positions after 32 pattern positions
                unsigned long long todo = __ballot(live != 0);
                while (todo) {
                    const int src = __builtin_ctzll(todo);  // wave-uniform
                    todo &= todo - 1;
                    const uint64_t dw = (cw + (uint64_t)u * kPlanesT + (uint32_t)src) * kChunk;
                    uint32_t R[kChunk];
#pragma unroll
                    for (uint32_t w = 0; w < kChunk; ++w) R[w] = __builtin_amdgcn_readlane(M[u][w], src);
                    planes_sets_verify<PLANES>(R, a, dw);
                    if (lane == (uint32_t)src) {
#pragma unroll
                        for (uint32_t w = 0; w < kChunk; ++w) M[u][w] = R[w];
                    }
                }
                live = M[u][0] | M[u][1] | M[u][2] | M[u][3];
            }
            uint32_t mine = 0;
#pragma unroll
            for (uint32_t w = 0; w < kChunk; ++w) mine += __builtin_popcount(M[u][w]);
            if constexpr (!FIND) {
                hits += mine;
            } else {
                if (!__any(live != 0)) continue;
                // planes_find's output stage: wave-wide exclusive prefix sum of the lanes' counts, one atomic, the lanes' stores
                unsigned long long slot = wave_reserve(mine, a.count, lane);
                const uint64_t pos = (cw + (uint64_t)u * kPlanesT + lane) * kPos;
#pragma unroll
                for (uint32_t w = 0; w < kChunk; ++w) {
                    uint32_t r = M[u][w];
                    while (r) {
                        const uint32_t i = __builtin_ctz(r);
                        r &= r - 1;
                        if (slot < cap) out[slot] = pos + 32 * w + i;
                        ++slot;
                    }
                }
            }
        }
    }
    if constexpr (!FIND) flush_hits(hits, a.count, smem, reinterpret_cast<const uint8_t*>(a.p0));
}

template <int PLANES>
__global__ __launch_bounds__(kPlanesT, 8) void planes_sets_scan(PlaneSetArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // 128 bytes: flush_hits
    planes_sets_body<PLANES, false>(a, smem, nullptr, 0);
}

template <int PLANES>
__global__ __launch_bounds__(kPlanesT, 8) void planes_sets_find(PlaneSetArgs a, unsigned long long* __restrict__ out, unsigned long long cap)
{
    planes_sets_body<PLANES, true>(a, nullptr, out, cap);
}

// Grid and occupancy: launch_planes_scan's.
static uint32_t planes_sets_grid(const PlaneSetArgs& a, int num_cus)
{
    constexpr uint64_t kPos = 32 * kChunk;
    const uint64_t chunks = (a.s_end + kPos - 1) / kPos - a.s_begin / kPos;
    const uint64_t want = (chunks + kPlanesT * kUnroll - 1) / (kPlanesT * kUnroll);
    return (uint32_t)std::min<uint64_t>(want, (uint64_t)num_cus * kPlanesWgs);
}

hipError_t launch_planes_sets_scan(const PlaneSetArgs& a, int planes, int num_cus, hipStream_t stream)
{
    if (a.s_end <= a.s_begin) return hipSuccess;
    const uint32_t grid = planes_sets_grid(a, num_cus);
    if (planes == 2)
        hipLaunchKernelGGL(planes_sets_scan<2>, dim3(grid), dim3(kPlanesT), 128, stream, a);
    else
        hipLaunchKernelGGL(planes_sets_scan<1>, dim3(grid), dim3(kPlanesT), 128, stream, a);
    return hipGetLastError();
}

hipError_t launch_planes_sets_find(const PlaneSetArgs& a, unsigned long long* out, unsigned long long cap, int planes, int num_cus,
                                   hipStream_t stream)
{
    if (a.s_end <= a.s_begin) return hipSuccess;
    const uint32_t grid = planes_sets_grid(a, num_cus);
    if (planes == 2)
        hipLaunchKernelGGL(planes_sets_find<2>, dim3(grid), dim3(kPlanesT), 0, stream, a, out, cap);
    else
        hipLaunchKernelGGL(planes_sets_find<1>, dim3(grid), dim3(kPlanesT), 0, stream, a, out, cap);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// planes_mis_scan<PLANES, BITS>, planes_mis_find<PLANES, BITS>: occurrences with at most `budget` MISMATCHES — they count /
// list the start positions s in [s_begin, s_end) whose number of j < m with T[s + j] != P[j] (positions of the skip plane
// excepted: pattern bytes the text does not hold, counted by the host) is at most a.budget.  Siblings of the sets kernels:
// the same geometry, loads, range masks, early leave and output stage; what differs is the state per 32 positions.
//
// In place of the one dword M of live positions: a BIT-SLICED COUNTER C[0..BITS) — bit i of C[b] is bit b of position i's
// count — and one sticky dword S, "over budget".  Every counter starts at 2^BITS - 1 - budget, so the carry out of the top
// bit is exactly "one mismatch more than the budget"; it ORs into S and stays there: a window with hundreds of mismatches
// wraps its counter bits many times, S is the verdict.  BITS = 1 / 2 / 3 serves budgets up to 1 / 3 / 7 (the launcher
// picks).  Per pattern symbol and dword: the v_alignbit per plane, then the mismatch dword f(t0, t1) — the complement of
// planes_kill's table for the symbol's code — is never formed: the counter's lowest stage takes it inside its two v_bitop3
// (sum C0 ^ f, carry C0 & f), the higher stages ripple (v_xor, v_and; the last: v_xor and one v_bitop3 S | C & carry).
// 5 / 6 / 8 vector instructions per 32 positions and symbol on two planes against planes_scan's 3.
// Positions outside the range start with their S bit set.  After every eight symbols the wave leaves when all of its
// positions are over budget: later than the exact scan, the more so the larger the budget.
// Symbols from the 32nd on: planes_mis_verify.  The find's entries are pos << 3 | distance: monotone in pos, so the spans
// are ordered on the host as planes_find's (match_calls.cpp order_spans, with a shift).
// kUnroll: planes_scan's (2 chunks per trip).  Occupancy: planes_scan's 8 workgroups per CU (39-63 VGPRs) — except BITS = 3
// on TWO planes, which keeps 3 * kChunk * kUnroll counter dwords beside both planes' words and does not fit 64 VGPRs
// without scratch (67 / 69 for scan / find): it is bounded for 128 and launched at 7 workgroups per CU.  Neither choice is swept.  planes_scan,
// planes_find and planes_sets_* are not touched.
// ---------------------------------------------------------------------------
template <int PLANES, int BITS, uint32_t F>  // F: the table of "mismatch" over t0 = 0xCC, t1 = 0xAA
static __device__ __forceinline__ void planes_mis_step(uint32_t (&C)[BITS][kChunk], uint32_t (&S)[kChunk], const PlaneWords& t, uint32_t j)
{
#pragma unroll
    for (uint32_t w = 0; w < kChunk; ++w) {
        const uint32_t t0 = __builtin_amdgcn_alignbit(t.a[w + 1], t.a[w], j);
        const uint32_t t1 = PLANES == 2 ? __builtin_amdgcn_alignbit(t.b[w + 1], t.b[w], j) : 0u;
        uint32_t carry = __builtin_amdgcn_bitop3_b32(C[0][w], t0, t1, 0xF0u & F);
        C[0][w] = __builtin_amdgcn_bitop3_b32(C[0][w], t0, t1, 0xF0u ^ F);
        if constexpr (BITS == 1) {
            S[w] |= carry;
        } else {
#pragma unroll
            for (int b = 1; b < BITS - 1; ++b) {
                const uint32_t c = C[b][w];
                C[b][w] = c ^ carry;
                carry &= c;
            }
            const uint32_t c = C[BITS - 1][w];
            C[BITS - 1][w] = c ^ carry;
            S[w] = __builtin_amdgcn_bitop3_b32(S[w], c, carry, 0xF8);  // S | c & carry
        }
    }
}

// symbols [j0, j1) (j1 <= 32) of the pattern's first block, bits x0 / x1, skip: positions that are not compared
template <int PLANES, int BITS>
static __device__ __forceinline__ void planes_mis_add(uint32_t (&C)[BITS][kChunk], uint32_t (&S)[kChunk], const PlaneWords& t, uint32_t x0,
                                                      uint32_t x1, uint32_t skip, uint32_t j0, uint32_t j1)
{
    for (uint32_t j = j0; j < j1; ++j) {
        if ((skip >> j) & 1u) continue;                                                     // wave-uniform
        const uint32_t c = ((x0 >> j) & 1u) | (PLANES == 2 ? ((x1 >> j) & 1u) << 1 : 0u);  // wave-uniform
        if (PLANES == 2) {
            if (c == 0) planes_mis_step<PLANES, BITS, 0xEE>(C, S, t, j);       // t0 | t1
            else if (c == 1) planes_mis_step<PLANES, BITS, 0xBB>(C, S, t, j);  // ~t0 | t1
            else if (c == 2) planes_mis_step<PLANES, BITS, 0xDD>(C, S, t, j);  // t0 | ~t1
            else planes_mis_step<PLANES, BITS, 0x77>(C, S, t, j);              // ~t0 | ~t1
        } else {
            if (c == 0) planes_mis_step<PLANES, BITS, 0xCC>(C, S, t, j);       // t0
            else planes_mis_step<PLANES, BITS, 0x33>(C, S, t, j);              // ~t0
        }
    }
}

// planes_verify with a count: the whole wave works on ONE lane's live positions (R, and their counters Cs: wave-uniform,
// scalar).  Lane l takes block k0 + l of the pattern — x0 / x1 and the skip plane from memory, the five text dwords k dwords
// behind the chunk — and popcounts its mismatch dword (skipped positions, the part of the last block beyond m and lanes
// beyond the last block masked off).  The wave SUMS the lanes' counts: they are at most 32, so six ballots, one per bit of
// the count, and six scalar popcounts give the sum wave-uniform with no shuffle.  It is added to the position's counter; a
// counter beyond 2^BITS - 1 is over budget, otherwise the new value goes back into the counter bits: the find reports it.
template <int PLANES, int BITS>
static __device__ __forceinline__ void planes_mis_verify(uint32_t (&R)[kChunk], uint32_t (&Cs)[BITS][kChunk], const PlaneMisArgs& a, uint64_t dw)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t k0 = 1; 32 * k0 < a.m && (R[0] | R[1] | R[2] | R[3]) != 0; k0 += 64) {
        const bool valid = 32 * (k0 + lane) < a.m;
        const uint32_t k = valid ? k0 + lane : k0;
        const uint32_t left = a.m - 32 * k;
        const uint32_t bmask = !valid ? 0u : left >= 32 ? ~0u : (1u << left) - 1u;  // the pattern's last block may be partial
        uint32_t ta[kChunk + 1], tb[kChunk + 1];
        __builtin_memcpy(ta, a.p0 + dw + k, 4 * (kChunk + 1));
        if (PLANES == 2) __builtin_memcpy(tb, a.p1 + dw + k, 4 * (kChunk + 1));
        const uint32_t x0 = a.pat[k], x1 = PLANES == 2 ? a.pat[kPatWords + k] : 0u;
        const uint32_t cmp = bmask & ~a.pat[2 * kPatWords + k];
#pragma unroll
        for (uint32_t w = 0; w < kChunk; ++w) {
            uint32_t r = R[w];
            while (r) {
                const uint32_t i = __builtin_ctz(r);
                r &= r - 1;
                uint32_t d = __builtin_amdgcn_alignbit(ta[w + 1], ta[w], i) ^ x0;
                if (PLANES == 2) d |= __builtin_amdgcn_alignbit(tb[w + 1], tb[w], i) ^ x1;
                const uint32_t cnt = __builtin_popcount(d & cmp);
                uint32_t cur = 0;
#pragma unroll
                for (int b = 0; b < 6; ++b) cur += (uint32_t)__builtin_popcountll(__ballot((cnt >> b) & 1u)) << b;
#pragma unroll
                for (int b = 0; b < BITS; ++b) cur += ((Cs[b][w] >> i) & 1u) << b;
                if (cur > (1u << BITS) - 1u) {
                    R[w] &= ~(1u << i);
                } else {
#pragma unroll
                    for (int b = 0; b < BITS; ++b) Cs[b][w] = (Cs[b][w] & ~(1u << i)) | (((cur >> b) & 1u) << i);
                }
            }
        }
    }
}

// The loop skeleton is planes_sets_body's: a change to one belongs in the other.  smem: flush_hits' 128 bytes (the scan only).
template <int PLANES, int BITS, bool FIND>
static __device__ __forceinline__ void planes_mis_body(const PlaneMisArgs& a, uint8_t* smem, unsigned long long* __restrict__ out,
                                                       unsigned long long cap)
{
    constexpr uint64_t kPos = 32 * kChunk;  // start positions per chunk
    const uint64_t c_end = (a.s_end + kPos - 1) / kPos;
    const uint64_t stride = (uint64_t)gridDim.x * kPlanesT * kUnroll;
    const uint32_t f1 = a.m < 32 ? a.m : 32u;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t start = (1u << BITS) - 1u - a.budget;  // every counter's first value: the carry out of bit BITS - 1 is "over budget"
    uint32_t hits = 0;
    // the trip count is the WAVE's (its first chunk decides): every lane stays for the ballots, the verification and the shuffles
    for (uint64_t cw = a.s_begin / kPos + (uint64_t)blockIdx.x * kPlanesT * kUnroll + 64u * wave; cw < c_end; cw += stride) {
        PlaneWords t[kUnroll];
        uint32_t C[kUnroll][BITS][kChunk], S[kUnroll][kChunk];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const uint64_t c = cw + (uint64_t)u * kPlanesT + lane;
            const bool in = c < c_end;
            const uint64_t dw = in ? c * kChunk : 0;
            const uint4 va = ld_stream16(reinterpret_cast<const uint8_t*>(a.p0 + dw));
            t[u].a[0] = va.x; t[u].a[1] = va.y; t[u].a[2] = va.z; t[u].a[3] = va.w;
            t[u].a[4] = a.p0[dw + kChunk];
            if (PLANES == 2) {
                const uint4 vb = ld_stream16(reinterpret_cast<const uint8_t*>(a.p1 + dw));
                t[u].b[0] = vb.x; t[u].b[1] = vb.y; t[u].b[2] = vb.z; t[u].b[3] = vb.w;
                t[u].b[4] = a.p1[dw + kChunk];
            }
            const bool inner = c * kPos >= a.s_begin && (c + 1) * kPos <= a.s_end;
#pragma unroll
            for (uint32_t w = 0; w < kChunk; ++w) {
                S[u][w] = !in ? ~0u : inner ? 0u : ~range_mask(c * kPos + 32 * w, a.s_begin, a.s_end);
#pragma unroll
                for (int b = 0; b < BITS; ++b) C[u][b][w] = (start >> b) & 1u ? ~0u : 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            uint32_t live = ~(S[u][0] & S[u][1] & S[u][2] & S[u][3]);
            for (uint32_t j0 = 0; j0 < f1; j0 += 8) {
                planes_mis_add<PLANES, BITS>(C[u], S[u], t[u], a.x0, a.x1, a.skip, j0, j0 + 8 < f1 ? j0 + 8 : f1);
                live = ~(S[u][0] & S[u][1] & S[u][2] & S[u][3]);
                if (!__any(live != 0)) break;
            }
            if (a.m > 32) {  // a lane has positions within the budget after 32 symbols
                unsigned long long todo = __ballot(live != 0);
                while (todo) {
                    const int src = __builtin_ctzll(todo);  // wave-uniform
                    todo &= todo - 1;
                    const uint64_t dw = (cw + (uint64_t)u * kPlanesT + (uint32_t)src) * kChunk;
                    uint32_t R[kChunk], Cs[BITS][kChunk];
#pragma unroll
                    for (uint32_t w = 0; w < kChunk; ++w) {
                        R[w] = ~__builtin_amdgcn_readlane(S[u][w], src);
#pragma unroll
                        for (int b = 0; b < BITS; ++b) Cs[b][w] = __builtin_amdgcn_readlane(C[u][b][w], src);
                    }
                    planes_mis_verify<PLANES, BITS>(R, Cs, a, dw);
                    if (lane == (uint32_t)src) {
#pragma unroll
                        for (uint32_t w = 0; w < kChunk; ++w) {
                            S[u][w] = ~R[w];
#pragma unroll
                            for (int b = 0; b < BITS; ++b) C[u][b][w] = Cs[b][w];
                        }
                    }
                }
                live = ~(S[u][0] & S[u][1] & S[u][2] & S[u][3]);
            }
            uint32_t mine = 0;
#pragma unroll
            for (uint32_t w = 0; w < kChunk; ++w) mine += __builtin_popcount(~S[u][w]);
            if constexpr (!FIND) {
                hits += mine;
            } else {
                if (!__any(live != 0)) continue;
                // planes_find's output stage: wave-wide exclusive prefix sum of the lanes' counts, one atomic, the lanes' stores
                unsigned long long slot = wave_reserve(mine, a.count, lane);
                const uint64_t pos = (cw + (uint64_t)u * kPlanesT + lane) * kPos;
                const uint32_t bias = a.foreign - start;  // distance = counter - start + the positions the host counted
#pragma unroll
                for (uint32_t w = 0; w < kChunk; ++w) {
                    uint32_t r = ~S[u][w];
                    while (r) {
                        const uint32_t i = __builtin_ctz(r);
                        r &= r - 1;
                        uint32_t dist = bias;
#pragma unroll
                        for (int b = 0; b < BITS; ++b) dist += ((C[u][b][w] >> i) & 1u) << b;
                        if (slot < cap) out[slot] = (pos + 32 * w + i) << kMisShift | dist;
                        ++slot;
                    }
                }
            }
        }
    }
    if constexpr (!FIND) flush_hits(hits, a.count, smem, reinterpret_cast<const uint8_t*>(a.p0));
}

// waves per SIMD the register allocation is bounded for, and workgroups per CU of the launch (see above)
template <int PLANES, int BITS> constexpr int kMisWaves = PLANES == 2 && BITS == 3 ? 4 : 8;
constexpr int mis_wgs(int planes, int bits) { return planes == 2 && bits == 3 ? 7 : kPlanesWgs; }

template <int PLANES, int BITS>
__global__ __launch_bounds__(kPlanesT, (kMisWaves<PLANES, BITS>)) void planes_mis_scan(PlaneMisArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // 128 bytes: flush_hits
    planes_mis_body<PLANES, BITS, false>(a, smem, nullptr, 0);
}

template <int PLANES, int BITS>
__global__ __launch_bounds__(kPlanesT, (kMisWaves<PLANES, BITS>)) void planes_mis_find(PlaneMisArgs a, unsigned long long* __restrict__ out, unsigned long long cap)
{
    planes_mis_body<PLANES, BITS, true>(a, nullptr, out, cap);
}

// Grid: launch_planes_scan's with mis_wgs workgroups per CU.  BITS from the budget: 1 / 2 / 3 for at most 1 / 3 / 7.
static uint32_t planes_mis_grid(const PlaneMisArgs& a, int planes, int num_cus, int bits)
{
    constexpr uint64_t kPos = 32 * kChunk;
    const uint64_t chunks = (a.s_end + kPos - 1) / kPos - a.s_begin / kPos;
    const uint64_t want = (chunks + kPlanesT * kUnroll - 1) / (kPlanesT * kUnroll);
    return (uint32_t)std::min<uint64_t>(want, (uint64_t)num_cus * mis_wgs(planes, bits));
}

hipError_t launch_planes_mis_scan(const PlaneMisArgs& a, int planes, int num_cus, hipStream_t stream)
{
    if (a.budget > SMARTGPU_PMIS_MAX) return hipErrorInvalidValue;
    if (a.s_end <= a.s_begin) return hipSuccess;
    const int bits = a.budget <= 1 ? 1 : a.budget <= 3 ? 2 : 3;
    const uint32_t grid = planes_mis_grid(a, planes, num_cus, bits);
#define SG_MIS_SCAN(p_, b_) hipLaunchKernelGGL((planes_mis_scan<p_, b_>), dim3(grid), dim3(kPlanesT), 128, stream, a)
    if (planes == 2) {
        if (bits == 1) SG_MIS_SCAN(2, 1); else if (bits == 2) SG_MIS_SCAN(2, 2); else SG_MIS_SCAN(2, 3);
    } else {
        if (bits == 1) SG_MIS_SCAN(1, 1); else if (bits == 2) SG_MIS_SCAN(1, 2); else SG_MIS_SCAN(1, 3);
    }
#undef SG_MIS_SCAN
    return hipGetLastError();
}

hipError_t launch_planes_mis_find(const PlaneMisArgs& a, unsigned long long* out, unsigned long long cap, int planes, int num_cus,
                                  hipStream_t stream)
{
    if (a.budget > SMARTGPU_PMIS_MAX) return hipErrorInvalidValue;
    if (a.s_end <= a.s_begin) return hipSuccess;
    const int bits = a.budget <= 1 ? 1 : a.budget <= 3 ? 2 : 3;
    const uint32_t grid = planes_mis_grid(a, planes, num_cus, bits);
#define SG_MIS_FIND(p_, b_) hipLaunchKernelGGL((planes_mis_find<p_, b_>), dim3(grid), dim3(kPlanesT), 0, stream, a, out, cap)
    if (planes == 2) {
        if (bits == 1) SG_MIS_FIND(2, 1); else if (bits == 2) SG_MIS_FIND(2, 2); else SG_MIS_FIND(2, 3);
    } else {
        if (bits == 1) SG_MIS_FIND(1, 1); else if (bits == 2) SG_MIS_FIND(1, 2); else SG_MIS_FIND(1, 3);
    }
#undef SG_MIS_FIND
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// planes_sets_mis_scan<PLANES, BITS>, planes_sets_mis_find<PLANES, BITS>: SET patterns with at most `budget` MISMATCHES —
// they count / list the start positions s in [s_begin, s_end) whose number of j < m with "the code of T[s + j] is NOT a
// member of set j" is at most a.budget.  The combination of the two families above: planes_mis_*'s geometry, loads, range
// masks in S, counter (start value 2^BITS - 1 - budget, sticky S), early leave after every eight positions, output stage
// (entries pos << kMisShift | distance) and choice of BITS; planes_sets_*'s wave-uniform set per position (bit j of
// y[0..3]: a scalar switch).  The mismatch table of a set is the complement of its membership table — 0xFF ^ the OR of its
// members' tables over t0 = 0xCC, t1 = 0xAA — and goes into planes_mis_step as it is: a set position costs what an exact
// symbol costs there, a position that accepts every code costs nothing.  There is no skip plane: positions the host does
// not compare (empty sets, a mismatch in every window: counted by the host as `foreign`, the budget lowered by them) arrive
// as "accepts every code".  An empty set that did arrive would be a mismatch everywhere (table 0xFF; beyond the 32nd
// position an all-zero membership bit): the kernels are total, the host merely never spends the launch's budget on it.
// Positions from the 32nd on: planes_sets_mis_verify.
// Occupancy: planes_mis_*'s choices, taken over UNMEASURED for these kernels — 8 workgroups per CU, except BITS = 3 on two
// planes, bounded for 128 VGPRs and launched at 7 workgroups per CU (cross-compiled for gfx950 it takes 60 / 62 VGPRs for
// scan / find, the others 39-56: it would fit eight waves, the bound is kept as its sibling's until it is measured).  Every
// instantiation has ScratchSize 0 and no static LDS.  planes_scan, planes_find, planes_sets_* and planes_mis_* are not touched.
// ---------------------------------------------------------------------------
// the table of "the code (t1 t0) is NOT a member of s" over t0 = 0xCC, t1 = 0xAA
constexpr uint32_t sets_mis_table(int planes, uint32_t s)
{
    return 0xFFu ^ (planes == 2 ? ((s & 1u ? 0x11u : 0u) | (s & 2u ? 0x44u : 0u) | (s & 4u ? 0x22u : 0u) | (s & 8u ? 0x88u : 0u))
                                : ((s & 1u ? 0x33u : 0u) | (s & 2u ? 0xCCu : 0u)));
}
static_assert(sets_mis_table(2, 1) == 0xEE && sets_mis_table(2, 2) == 0xBB && sets_mis_table(2, 4) == 0xDD && sets_mis_table(2, 8) == 0x77 &&
              sets_mis_table(1, 1) == 0xCC && sets_mis_table(1, 2) == 0x33, "singleton sets: planes_mis_add's tables");

// positions [j0, j1) (j1 <= 32) of the pattern's first block, membership bits y[c]
template <int PLANES, int BITS>
static __device__ __forceinline__ void planes_sets_mis_add(uint32_t (&C)[BITS][kChunk], uint32_t (&S)[kChunk], const PlaneWords& t,
                                                           const uint32_t (&y)[4], uint32_t j0, uint32_t j1)
{
    for (uint32_t j = j0; j < j1; ++j) {
        uint32_t s = ((y[0] >> j) & 1u) | ((y[1] >> j) & 1u) << 1;  // wave-uniform
        if (PLANES == 2) s |= ((y[2] >> j) & 1u) << 2 | ((y[3] >> j) & 1u) << 3;
#define SG_SETS_MIS_CASE(s_) case s_: planes_mis_step<PLANES, BITS, sets_mis_table(PLANES, s_)>(C, S, t, j); break;
        if (PLANES == 2) {
            switch (s) {
                SG_SETS_MIS_CASE(0) SG_SETS_MIS_CASE(1) SG_SETS_MIS_CASE(2) SG_SETS_MIS_CASE(3) SG_SETS_MIS_CASE(4) SG_SETS_MIS_CASE(5)
                SG_SETS_MIS_CASE(6) SG_SETS_MIS_CASE(7) SG_SETS_MIS_CASE(8) SG_SETS_MIS_CASE(9) SG_SETS_MIS_CASE(10) SG_SETS_MIS_CASE(11)
                SG_SETS_MIS_CASE(12) SG_SETS_MIS_CASE(13) SG_SETS_MIS_CASE(14)
                default: break;  // every code: no instruction
            }
        } else {
            switch (s) {
                SG_SETS_MIS_CASE(0) SG_SETS_MIS_CASE(1) SG_SETS_MIS_CASE(2)
                default: break;
            }
        }
#undef SG_SETS_MIS_CASE
    }
}

// planes_mis_verify for sets: the whole wave works on ONE lane's positions within the budget (R, and their counters Cs:
// wave-uniform).  Lane l takes block k0 + l of the pattern — the membership dwords Y0..Y3[k] (Y0, Y1 on one plane), ~bmask
// ORed in: positions beyond the pattern's end and lanes beyond the last block accept everything, as the positions the host
// does not compare do by their all-ones bits — forms the "accepted" dword with planes_sets_verify's multiplexer and
// popcounts its complement.  The wave sums the lanes' counts (at most 32 each) by six ballots, as planes_mis_verify.
template <int PLANES, int BITS>
static __device__ __forceinline__ void planes_sets_mis_verify(uint32_t (&R)[kChunk], uint32_t (&Cs)[BITS][kChunk], const PlaneSetMisArgs& a,
                                                              uint64_t dw)
{
    constexpr uint32_t kMux = 0xCA;  // bitop3(sel, one, zero): sel ? one : zero, bit by bit
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t k0 = 1; 32 * k0 < a.m && (R[0] | R[1] | R[2] | R[3]) != 0; k0 += 64) {
        const bool valid = 32 * (k0 + lane) < a.m;
        const uint32_t k = valid ? k0 + lane : k0;
        const uint32_t left = a.m - 32 * k;
        const uint32_t bmask = !valid ? 0u : left >= 32 ? ~0u : (1u << left) - 1u;  // the pattern's last block may be partial
        uint32_t ta[kChunk + 1], tb[kChunk + 1];
        __builtin_memcpy(ta, a.p0 + dw + k, 4 * (kChunk + 1));
        if (PLANES == 2) __builtin_memcpy(tb, a.p1 + dw + k, 4 * (kChunk + 1));
        const uint32_t y0 = a.pat[k] | ~bmask, y1 = a.pat[kPatWords + k] | ~bmask;
        const uint32_t y2 = PLANES == 2 ? a.pat[2 * kPatWords + k] | ~bmask : 0u;
        const uint32_t y3 = PLANES == 2 ? a.pat[3 * kPatWords + k] | ~bmask : 0u;
#pragma unroll
        for (uint32_t w = 0; w < kChunk; ++w) {
            uint32_t r = R[w];
            while (r) {
                const uint32_t i = __builtin_ctz(r);
                r &= r - 1;
                const uint32_t t0 = __builtin_amdgcn_alignbit(ta[w + 1], ta[w], i);
                uint32_t acc = __builtin_amdgcn_bitop3_b32(t0, y1, y0, kMux);
                if (PLANES == 2) {
                    const uint32_t t1 = __builtin_amdgcn_alignbit(tb[w + 1], tb[w], i);
                    acc = __builtin_amdgcn_bitop3_b32(t1, __builtin_amdgcn_bitop3_b32(t0, y3, y2, kMux), acc, kMux);
                }
                const uint32_t cnt = __builtin_popcount(~acc);
                uint32_t cur = 0;
#pragma unroll
                for (int b = 0; b < 6; ++b) cur += (uint32_t)__builtin_popcountll(__ballot((cnt >> b) & 1u)) << b;
#pragma unroll
                for (int b = 0; b < BITS; ++b) cur += ((Cs[b][w] >> i) & 1u) << b;
                if (cur > (1u << BITS) - 1u) {
                    R[w] &= ~(1u << i);
                } else {
#pragma unroll
                    for (int b = 0; b < BITS; ++b) Cs[b][w] = (Cs[b][w] & ~(1u << i)) | (((cur >> b) & 1u) << i);
                }
            }
        }
    }
}

// The loop skeleton is planes_mis_body's: a change to one belongs in the other.  smem: flush_hits' 128 bytes (the scan only).
template <int PLANES, int BITS, bool FIND>
static __device__ __forceinline__ void planes_sets_mis_body(const PlaneSetMisArgs& a, uint8_t* smem, unsigned long long* __restrict__ out,
                                                            unsigned long long cap)
{
    constexpr uint64_t kPos = 32 * kChunk;  // start positions per chunk
    const uint64_t c_end = (a.s_end + kPos - 1) / kPos;
    const uint64_t stride = (uint64_t)gridDim.x * kPlanesT * kUnroll;
    const uint32_t f1 = a.m < 32 ? a.m : 32u;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t start = (1u << BITS) - 1u - a.budget;  // every counter's first value: the carry out of bit BITS - 1 is "over budget"
    uint32_t hits = 0;
    // the trip count is the WAVE's (its first chunk decides): every lane stays for the ballots, the verification and the shuffles
    for (uint64_t cw = a.s_begin / kPos + (uint64_t)blockIdx.x * kPlanesT * kUnroll + 64u * wave; cw < c_end; cw += stride) {
        PlaneWords t[kUnroll];
        uint32_t C[kUnroll][BITS][kChunk], S[kUnroll][kChunk];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const uint64_t c = cw + (uint64_t)u * kPlanesT + lane;
            const bool in = c < c_end;
            const uint64_t dw = in ? c * kChunk : 0;
            const uint4 va = ld_stream16(reinterpret_cast<const uint8_t*>(a.p0 + dw));
            t[u].a[0] = va.x; t[u].a[1] = va.y; t[u].a[2] = va.z; t[u].a[3] = va.w;
            t[u].a[4] = a.p0[dw + kChunk];
            if (PLANES == 2) {
                const uint4 vb = ld_stream16(reinterpret_cast<const uint8_t*>(a.p1 + dw));
                t[u].b[0] = vb.x; t[u].b[1] = vb.y; t[u].b[2] = vb.z; t[u].b[3] = vb.w;
                t[u].b[4] = a.p1[dw + kChunk];
            }
            const bool inner = c * kPos >= a.s_begin && (c + 1) * kPos <= a.s_end;
#pragma unroll
            for (uint32_t w = 0; w < kChunk; ++w) {
                S[u][w] = !in ? ~0u : inner ? 0u : ~range_mask(c * kPos + 32 * w, a.s_begin, a.s_end);
#pragma unroll
                for (int b = 0; b < BITS; ++b) C[u][b][w] = (start >> b) & 1u ? ~0u : 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            uint32_t live = ~(S[u][0] & S[u][1] & S[u][2] & S[u][3]);
            for (uint32_t j0 = 0; j0 < f1; j0 += 8) {
                planes_sets_mis_add<PLANES, BITS>(C[u], S[u], t[u], a.y, j0, j0 + 8 < f1 ? j0 + 8 : f1);
                live = ~(S[u][0] & S[u][1] & S[u][2] & S[u][3]);
                if (!__any(live != 0)) break;
            }
            if (a.m > 32) {  // a lane has positions within the budget after 32 pattern positions
                unsigned long long todo = __ballot(live != 0);
                while (todo) {
                    const int src = __builtin_ctzll(todo);  // wave-uniform
                    todo &= todo - 1;
                    const uint64_t dw = (cw + (uint64_t)u * kPlanesT + (uint32_t)src) * kChunk;
                    uint32_t R[kChunk], Cs[BITS][kChunk];
#pragma unroll
                    for (uint32_t w = 0; w < kChunk; ++w) {
                        R[w] = ~__builtin_amdgcn_readlane(S[u][w], src);
#pragma unroll
                        for (int b = 0; b < BITS; ++b) Cs[b][w] = __builtin_amdgcn_readlane(C[u][b][w], src);
                    }
                    planes_sets_mis_verify<PLANES, BITS>(R, Cs, a, dw);
                    if (lane == (uint32_t)src) {
#pragma unroll
                        for (uint32_t w = 0; w < kChunk; ++w) {
                            S[u][w] = ~R[w];
#pragma unroll
                            for (int b = 0; b < BITS; ++b) C[u][b][w] = Cs[b][w];
                        }
                    }
                }
                live = ~(S[u][0] & S[u][1] & S[u][2] & S[u][3]);
            }
            uint32_t mine = 0;
#pragma unroll
            for (uint32_t w = 0; w < kChunk; ++w) mine += __builtin_popcount(~S[u][w]);
            if constexpr (!FIND) {
                hits += mine;
            } else {
                if (!__any(live != 0)) continue;
                // planes_find's output stage: wave-wide exclusive prefix sum of the lanes' counts, one atomic, the lanes' stores
                unsigned long long slot = wave_reserve(mine, a.count, lane);
                const uint64_t pos = (cw + (uint64_t)u * kPlanesT + lane) * kPos;
                const uint32_t bias = a.foreign - start;  // distance = counter - start + the positions the host counted
#pragma unroll
                for (uint32_t w = 0; w < kChunk; ++w) {
                    uint32_t r = ~S[u][w];
                    while (r) {
                        const uint32_t i = __builtin_ctz(r);
                        r &= r - 1;
                        uint32_t dist = bias;
#pragma unroll
                        for (int b = 0; b < BITS; ++b) dist += ((C[u][b][w] >> i) & 1u) << b;
                        if (slot < cap) out[slot] = (pos + 32 * w + i) << kMisShift | dist;
                        ++slot;
                    }
                }
            }
        }
    }
    if constexpr (!FIND) flush_hits(hits, a.count, smem, reinterpret_cast<const uint8_t*>(a.p0));
}

template <int PLANES, int BITS>
__global__ __launch_bounds__(kPlanesT, (kMisWaves<PLANES, BITS>)) void planes_sets_mis_scan(PlaneSetMisArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // 128 bytes: flush_hits
    planes_sets_mis_body<PLANES, BITS, false>(a, smem, nullptr, 0);
}

template <int PLANES, int BITS>
__global__ __launch_bounds__(kPlanesT, (kMisWaves<PLANES, BITS>)) void planes_sets_mis_find(PlaneSetMisArgs a, unsigned long long* __restrict__ out, unsigned long long cap)
{
    planes_sets_mis_body<PLANES, BITS, true>(a, nullptr, out, cap);
}

// Grid and BITS: launch_planes_mis_scan's.
static uint32_t planes_sets_mis_grid(const PlaneSetMisArgs& a, int planes, int num_cus, int bits)
{
    constexpr uint64_t kPos = 32 * kChunk;
    const uint64_t chunks = (a.s_end + kPos - 1) / kPos - a.s_begin / kPos;
    const uint64_t want = (chunks + kPlanesT * kUnroll - 1) / (kPlanesT * kUnroll);
    return (uint32_t)std::min<uint64_t>(want, (uint64_t)num_cus * mis_wgs(planes, bits));
}

hipError_t launch_planes_sets_mis_scan(const PlaneSetMisArgs& a, int planes, int num_cus, hipStream_t stream)
{
    if (a.budget > SMARTGPU_PMIS_MAX) return hipErrorInvalidValue;
    if (a.s_end <= a.s_begin) return hipSuccess;
    const int bits = a.budget <= 1 ? 1 : a.budget <= 3 ? 2 : 3;
    const uint32_t grid = planes_sets_mis_grid(a, planes, num_cus, bits);
#define SG_SETS_MIS_SCAN(p_, b_) hipLaunchKernelGGL((planes_sets_mis_scan<p_, b_>), dim3(grid), dim3(kPlanesT), 128, stream, a)
    if (planes == 2) {
        if (bits == 1) SG_SETS_MIS_SCAN(2, 1); else if (bits == 2) SG_SETS_MIS_SCAN(2, 2); else SG_SETS_MIS_SCAN(2, 3);
    } else {
        if (bits == 1) SG_SETS_MIS_SCAN(1, 1); else if (bits == 2) SG_SETS_MIS_SCAN(1, 2); else SG_SETS_MIS_SCAN(1, 3);
    }
#undef SG_SETS_MIS_SCAN
    return hipGetLastError();
}

hipError_t launch_planes_sets_mis_find(const PlaneSetMisArgs& a, unsigned long long* out, unsigned long long cap, int planes, int num_cus,
                                       hipStream_t stream)
{
    if (a.budget > SMARTGPU_PMIS_MAX) return hipErrorInvalidValue;
    if (a.s_end <= a.s_begin) return hipSuccess;
    const int bits = a.budget <= 1 ? 1 : a.budget <= 3 ? 2 : 3;
    const uint32_t grid = planes_sets_mis_grid(a, planes, num_cus, bits);
#define SG_SETS_MIS_FIND(p_, b_) hipLaunchKernelGGL((planes_sets_mis_find<p_, b_>), dim3(grid), dim3(kPlanesT), 0, stream, a, out, cap)
    if (planes == 2) {
        if (bits == 1) SG_SETS_MIS_FIND(2, 1); else if (bits == 2) SG_SETS_MIS_FIND(2, 2); else SG_SETS_MIS_FIND(2, 3);
    } else {
        if (bits == 1) SG_SETS_MIS_FIND(1, 1); else if (bits == 2) SG_SETS_MIS_FIND(1, 2); else SG_SETS_MIS_FIND(1, 3);
    }
#undef SG_SETS_MIS_FIND
    return hipGetLastError();
}

}  // namespace sg
