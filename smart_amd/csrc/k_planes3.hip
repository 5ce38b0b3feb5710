// k_planes3.hip — packed texts of five to eight values on THREE bit planes: planes3_pack (byte text -> planes, once per
// text), planes3_scan<BITS> / planes3_find<BITS> (one body for the exact, set, mismatch and set-with-mismatch calls, count
// and find)
// (one translation unit per kernel family: dev_common.hpp; the layout and the arguments: planes3.hpp)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "planes3.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// planes3_pack: planes_pack (k_planes.hip) with seven compares for the rank and three output dwords.  A lane reads 32
// consecutive text bytes (two non-temporal 16-byte loads) and forms the dword of each plane itself; v[] = 255 where the
// text has fewer values.  Zero bytes of the text's back pad beyond n give code 0: the planes' tail bits are zero.
// ---------------------------------------------------------------------------
struct Pack3Values { uint32_t v[7]; };

__global__ __launch_bounds__(256) void planes3_pack(const uint8_t* __restrict__ text, uint64_t ndwords, uint32_t* __restrict__ p0,
                                                    uint32_t* __restrict__ p1, uint32_t* __restrict__ p2, Pack3Values vs)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < ndwords; g += stride) {
        const uint4 a = ld_stream16(text + 32 * g), b = ld_stream16(text + 32 * g + 16);
        const uint32_t d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t b0 = 0, b1 = 0, b2 = 0;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const uint32_t c = (d[i >> 2] >> (8 * (i & 3))) & 0xFFu;
            uint32_t code = 0;
#pragma unroll
            for (int k = 0; k < 7; ++k) code += (uint32_t)(c > vs.v[k]);
            b0 |= (code & 1u) << i;
            b1 |= ((code >> 1) & 1u) << i;
            b2 |= (code >> 2) << i;
        }
        p0[g] = b0;
        p1[g] = b1;
        p2[g] = b2;
    }
}

static hipError_t launch_planes3_pack(const uint8_t* text, uint64_t n, uint32_t* p0, uint32_t* p1, uint32_t* p2, const uint8_t values[7],
                                      hipStream_t stream)
{
    const uint64_t ndwords = (n + 31) / 32;
    if (ndwords == 0) return hipSuccess;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((ndwords + 255) / 256, 65536);
    Pack3Values vs;
    for (int k = 0; k < 7; ++k) vs.v[k] = values[k];
    hipLaunchKernelGGL(planes3_pack, dim3(grid), dim3(256), 0, stream, text, ndwords, p0, p1, p2, vs);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// planes3_scan<BITS>, planes3_find<BITS>: they count / list the start positions s in [s_begin, s_end) whose number of
// j < m with "the code of T[s + j] is NOT a member of set j" is at most a.budget.  One body, planes3_body<BITS, FIND>,
// serves all ten calls on a three-plane text: an exact pattern travels as singleton sets, a position the host does not
// compare (an empty set, a foreign byte of a mismatch pattern: counted by the host as `foreign`) as "accepts every code".
//
// The scheme is planes_sets_mis_body's (k_planes.hip) and these are taken from it unchanged: 256 lanes, a lane owns
// kChunk = 4 consecutive dwords of start positions per plane (one non-temporal global_load_dwordx4 and a cached load of the
// dword behind them, per plane), kUnroll = 2 chunks per lane and trip, the WAVE's trip count, the range masks, the early
// leave after every eight positions when none of the wave's 8192 positions is live, the wave-wide verification of
// positions from the 32nd on (lane l takes block k0 + l), the find's output stage (spans of kFindSpan, ordered on the host
// by order_spans) and flush_hits through the front pad below plane 0.
//
// State per 32 start positions: a dword M of LIVE positions (positions outside the range start dead), and for BITS > 0 a
// bit-sliced counter C[0..BITS) — bit i of C[b] is bit b of position i's count, every counter starts at 2^BITS - 1 - budget,
// so the carry out of the top bit is "one non-member more than the budget" and clears the position's M bit for good: a
// window with hundreds of mismatches wraps its counter many times, M is the verdict.  BITS = 1 / 2 / 3 serves budgets up
// to 1 / 3 / 7; BITS = 0 is the live-mask form for budget 0 — the exact and set calls pay for no counter.
//
// The step per pattern position j.  Its set S — bit j of y[0..7], kernel arguments for the first 32 positions — is
// wave-uniform; lo = S & 15 are the members among codes 0..3 (plane 2 clear), hi = S >> 4 among codes 4..7:
//     member = t2 ? f_hi(t0, t1) : f_lo(t0, t1),   t_b = v_alignbit(plane_b[w + 1], plane_b[w], j).
// f_lo and f_hi are one v_bitop3 each with an immediate table (k_planes.hip's two-plane tables: mem2_table, mis2_table),
// chosen by two scalar 16-way switches, and a third v_bitop3 (table 0xCA) is the multiplexer.  BITS = 0 folds M into the
// two table operations (M & f): 3 v_alignbit + 3 v_bitop3 per 32 positions where planes_scan takes 3 in all.  BITS > 0
// forms the non-member dword the same way (three operations) and adds it to the counter as planes_mis_step adds its own
// (v_and, v_xor for the lowest stage, then the ripple).  Cheaper cases, all wave-uniform branches: S = 0xFF costs nothing;
// hi == lo (the set does not depend on plane 2) is the two-plane step with no third v_alignbit; hi == 0 and lo == 0 (every
// singleton, so every exact pattern) take one table operation and one v_and / v_or with plane 2 — five instructions.
//
// Occupancy.  Three planes are 15 text dwords per chunk and 30 per trip beside M, the counters and a position's aligned
// dwords: NO form fits the 64 VGPRs of eight waves per SIMD without scratch (bounded for eight waves the BITS = 0 scan
// spills 32 bytes per lane), and a kernel with scratch is not shipped (tests/test_build.py).  So every instantiation is
// bounded for 128 VGPRs, as planes_mis_scan<2, 3> is, and launched at the workgroups per CU its registers allow.
// Cross-compiled for gfx950, VGPRs scan / find: BITS = 0: 68 / 70, 1: 72 / 75, 2: 76 / 79, 3: 80 / 83 — 7 / 7, 7 / 6,
// 6 / 6 and 6 / 5 workgroups per CU (512 registers per lane and SIMD, allocated in eights).  The choice is not swept.
// Every instantiation has ScratchSize 0 and no static LDS.
// ---------------------------------------------------------------------------
constexpr int kP3T = 256;
constexpr uint32_t kChunk = 4;  // dwords per lane and plane
constexpr int kUnroll = 2;      // chunks per lane and trip of the loop
constexpr uint32_t kMux = 0xCA;  // bitop3(sel, one, zero): sel ? one : zero, bit by bit
static_assert(kFindSpan == 64 * 32 * kChunk, "a span of planes3_find: one wave's lanes, one chunk each");
static_assert(kP3T % 64 == 0, "every wave's chunk row starts a multiple of 64 chunks behind the range's first: the host's span number");

template <int BITS> constexpr int kCB = BITS > 0 ? BITS : 1;  // counter dwords held (none is used with BITS = 0)
// waves per SIMD the register allocation is bounded for, and workgroups per CU of the launch (see above)
constexpr int kP3Waves = 4;
constexpr int p3_wgs(int bits, bool find) { return find ? (bits == 0 ? 7 : bits == 3 ? 5 : 6) : (bits <= 1 ? 7 : 6); }

struct Plane3Words { uint32_t a[kChunk + 1], b[kChunk + 1], c[kChunk + 1]; };  // five consecutive dwords of planes 0 / 1 / 2

// bits i with lo <= p + i < hi
static __device__ __forceinline__ uint32_t range_mask(uint64_t p, uint64_t lo, uint64_t hi)
{
    uint32_t m = ~0u;
    if (lo > p) m = lo - p >= 32 ? 0u : m << (uint32_t)(lo - p);
    if (hi < p + 32) m = hi <= p ? 0u : m & (~0u >> (32u - (uint32_t)(hi - p)));
    return m;
}

// One half of a set (four codes, two planes) against four dwords: BITS = 0: X & "member" (X = M), else "not a member".
template <int BITS, uint32_t S4>
static __device__ __forceinline__ void p3_half(uint32_t (&r)[kChunk], const uint32_t (&X)[kChunk], const uint32_t (&t0)[kChunk],
                                               const uint32_t (&t1)[kChunk])
{
#pragma unroll
    for (uint32_t w = 0; w < kChunk; ++w) {
        if constexpr (BITS == 0) r[w] = __builtin_amdgcn_bitop3_b32(X[w], t0[w], t1[w], mem2_table(S4));
        else r[w] = __builtin_amdgcn_bitop3_b32(t0[w], t0[w], t1[w], mis2_table(S4));
    }
}

// the scalar 16-way switch: one case per table
template <int BITS>
static __device__ __forceinline__ void p3_half_of(uint32_t s4, uint32_t (&r)[kChunk], const uint32_t (&X)[kChunk],
                                                  const uint32_t (&t0)[kChunk], const uint32_t (&t1)[kChunk])
{
#define SG_P3_CASE(s_) case s_: p3_half<BITS, s_>(r, X, t0, t1); break;
    switch (s4) {
        SG_P3_CASE(0) SG_P3_CASE(1) SG_P3_CASE(2) SG_P3_CASE(3) SG_P3_CASE(4) SG_P3_CASE(5) SG_P3_CASE(6) SG_P3_CASE(7)
        SG_P3_CASE(8) SG_P3_CASE(9) SG_P3_CASE(10) SG_P3_CASE(11) SG_P3_CASE(12) SG_P3_CASE(13) SG_P3_CASE(14)
        default: p3_half<BITS, 15>(r, X, t0, t1); break;
    }
#undef SG_P3_CASE
}

// the non-member dword f into the counters of dword w, as planes_mis_step: the carry out of the top bit kills the position
template <int BITS>
static __device__ __forceinline__ void p3_count(uint32_t& M, uint32_t (&C)[kCB<BITS>][kChunk], uint32_t w, uint32_t f)
{
    uint32_t carry = C[0][w] & f;
    C[0][w] ^= f;
    if constexpr (BITS == 1) {
        M &= ~carry;
    } else {
#pragma unroll
        for (int b = 1; b < BITS - 1; ++b) {
            const uint32_t c = C[b][w];
            C[b][w] = c ^ carry;
            carry &= c;
        }
        const uint32_t c = C[BITS - 1][w];
        C[BITS - 1][w] = c ^ carry;
        M = __builtin_amdgcn_bitop3_b32(M, c, carry, 0x70);  // M & ~(c & carry)
    }
}

// positions [j0, j1) (j1 <= 32) of the pattern's first block, membership bits y[c], against the block's five dwords per plane
template <int BITS>
static __device__ __forceinline__ void p3_add(uint32_t (&M)[kChunk], uint32_t (&C)[kCB<BITS>][kChunk], const Plane3Words& t,
                                              const uint32_t (&y)[8], uint32_t j0, uint32_t j1)
{
    for (uint32_t j = j0; j < j1; ++j) {
        uint32_t s = 0;  // wave-uniform
#pragma unroll
        for (uint32_t c = 0; c < 8; ++c) s |= ((y[c] >> j) & 1u) << c;
        if (s == 0xFFu) continue;  // every code: no instruction
        const uint32_t lo = s & 15u, hi = s >> 4;
        uint32_t t0[kChunk], t1[kChunk], r[kChunk];
#pragma unroll
        for (uint32_t w = 0; w < kChunk; ++w) {
            t0[w] = __builtin_amdgcn_alignbit(t.a[w + 1], t.a[w], j);
            t1[w] = __builtin_amdgcn_alignbit(t.b[w + 1], t.b[w], j);
        }
        p3_half_of<BITS>(lo, r, M, t0, t1);
        if (hi != lo) {  // the set depends on plane 2
            uint32_t t2[kChunk];
#pragma unroll
            for (uint32_t w = 0; w < kChunk; ++w) t2[w] = __builtin_amdgcn_alignbit(t.c[w + 1], t.c[w], j);
            if (hi == 0) {  // codes 0..3 only
#pragma unroll
                for (uint32_t w = 0; w < kChunk; ++w) r[w] = BITS == 0 ? r[w] & ~t2[w] : r[w] | t2[w];
            } else {
                uint32_t h[kChunk];
                p3_half_of<BITS>(hi, h, M, t0, t1);
                if (lo == 0) {  // codes 4..7 only
#pragma unroll
                    for (uint32_t w = 0; w < kChunk; ++w) r[w] = BITS == 0 ? h[w] & t2[w] : h[w] | ~t2[w];
                } else {
#pragma unroll
                    for (uint32_t w = 0; w < kChunk; ++w) r[w] = __builtin_amdgcn_bitop3_b32(t2[w], h[w], r[w], kMux);
                }
            }
        }
#pragma unroll
        for (uint32_t w = 0; w < kChunk; ++w) {
            if constexpr (BITS == 0) M[w] = r[w];
            else p3_count<BITS>(M[w], C, w, r[w]);
        }
    }
}

// Pattern positions from the 32nd on, for the live positions of ONE lane's chunk, by the whole wave (R, and their counters
// Cs: wave-uniform, scalar), as planes_sets_mis_verify: lane l takes block k0 + l of the pattern — the membership dwords
// Y0..Y7[k], ~bmask ORed in: positions beyond the pattern's end and lanes beyond the last block accept everything, as the
// positions the host does not compare do by their all-ones bits — and the five text dwords of each plane k dwords behind the
// chunk.  Bit b of `acc` says that the text symbol b behind the live position is accepted by pattern position 32 k + b:
// the Y dword its code selects, bit by bit — a three-level multiplexer, seven v_bitop3.  BITS = 0: the position survives
// when every lane accepts all 32, one ballot.  BITS > 0: the lanes popcount their non-members, the wave sums the counts (at
// most 32 each) by six ballots, the sum is added to the position's counter; beyond 2^BITS - 1 it is over budget, otherwise
// the new value goes back into the counter bits: the find reports it.
template <int BITS>
static __device__ __forceinline__ void p3_verify(uint32_t (&R)[kChunk], uint32_t (&Cs)[kCB<BITS>][kChunk], const Plane3Args& a, uint64_t dw)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t k0 = 1; 32 * k0 < a.m && (R[0] | R[1] | R[2] | R[3]) != 0; k0 += 64) {
        const bool valid = 32 * (k0 + lane) < a.m;
        const uint32_t k = valid ? k0 + lane : k0;
        const uint32_t left = a.m - 32 * k;
        const uint32_t bmask = !valid ? 0u : left >= 32 ? ~0u : (1u << left) - 1u;  // the pattern's last block may be partial
        uint32_t ta[kChunk + 1], tb[kChunk + 1], tc[kChunk + 1], y[8];
        __builtin_memcpy(ta, a.p0 + dw + k, 4 * (kChunk + 1));
        __builtin_memcpy(tb, a.p1 + dw + k, 4 * (kChunk + 1));
        __builtin_memcpy(tc, a.p2 + dw + k, 4 * (kChunk + 1));
#pragma unroll
        for (uint32_t c = 0; c < 8; ++c) y[c] = a.pat[c * kPatWords + k] | ~bmask;
#pragma unroll
        for (uint32_t w = 0; w < kChunk; ++w) {
            uint32_t r = R[w];
            while (r) {
                const uint32_t i = __builtin_ctz(r);
                r &= r - 1;
                const uint32_t t0 = __builtin_amdgcn_alignbit(ta[w + 1], ta[w], i);
                const uint32_t t1 = __builtin_amdgcn_alignbit(tb[w + 1], tb[w], i);
                const uint32_t t2 = __builtin_amdgcn_alignbit(tc[w + 1], tc[w], i);
                const uint32_t lo = __builtin_amdgcn_bitop3_b32(t1, __builtin_amdgcn_bitop3_b32(t0, y[3], y[2], kMux),
                                                                __builtin_amdgcn_bitop3_b32(t0, y[1], y[0], kMux), kMux);
                const uint32_t hi = __builtin_amdgcn_bitop3_b32(t1, __builtin_amdgcn_bitop3_b32(t0, y[7], y[6], kMux),
                                                                __builtin_amdgcn_bitop3_b32(t0, y[5], y[4], kMux), kMux);
                const uint32_t acc = __builtin_amdgcn_bitop3_b32(t2, hi, lo, kMux);
                if constexpr (BITS == 0) {
                    if (__any(acc != ~0u)) R[w] &= ~(1u << i);
                } else {
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
}

// The loop skeleton is planes_sets_mis_body's (k_planes.hip): a change to one belongs in the other.  smem: flush_hits' 128
// bytes (the scan only).
template <int BITS, bool FIND>
static __device__ __forceinline__ void planes3_body(const Plane3Args& a, uint8_t* smem, unsigned long long* __restrict__ out,
                                                    unsigned long long cap)
{
    constexpr uint64_t kPos = 32 * kChunk;  // start positions per chunk
    const uint64_t c_end = (a.s_end + kPos - 1) / kPos;
    const uint64_t stride = (uint64_t)gridDim.x * kP3T * kUnroll;
    const uint32_t f1 = a.m < 32 ? a.m : 32u;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t start = (1u << BITS) - 1u - a.budget;  // every counter's first value: the carry out of bit BITS - 1 is "over budget"
    uint32_t hits = 0;
    // the trip count is the WAVE's (its first chunk decides): every lane stays for the ballots, the verification and the shuffles
    for (uint64_t cw = a.s_begin / kPos + (uint64_t)blockIdx.x * kP3T * kUnroll + 64u * wave; cw < c_end; cw += stride) {
        Plane3Words t[kUnroll];
        uint32_t M[kUnroll][kChunk], C[kUnroll][kCB<BITS>][kChunk];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const uint64_t c = cw + (uint64_t)u * kP3T + lane;
            const bool in = c < c_end;
            const uint64_t dw = in ? c * kChunk : 0;
            const uint4 va = ld_stream16(reinterpret_cast<const uint8_t*>(a.p0 + dw));
            t[u].a[0] = va.x; t[u].a[1] = va.y; t[u].a[2] = va.z; t[u].a[3] = va.w;
            t[u].a[4] = a.p0[dw + kChunk];
            const uint4 vb = ld_stream16(reinterpret_cast<const uint8_t*>(a.p1 + dw));
            t[u].b[0] = vb.x; t[u].b[1] = vb.y; t[u].b[2] = vb.z; t[u].b[3] = vb.w;
            t[u].b[4] = a.p1[dw + kChunk];
            const uint4 vc = ld_stream16(reinterpret_cast<const uint8_t*>(a.p2 + dw));
            t[u].c[0] = vc.x; t[u].c[1] = vc.y; t[u].c[2] = vc.z; t[u].c[3] = vc.w;
            t[u].c[4] = a.p2[dw + kChunk];
            const bool inner = c * kPos >= a.s_begin && (c + 1) * kPos <= a.s_end;
#pragma unroll
            for (uint32_t w = 0; w < kChunk; ++w) {
                M[u][w] = !in ? 0u : inner ? ~0u : range_mask(c * kPos + 32 * w, a.s_begin, a.s_end);
#pragma unroll
                for (int b = 0; b < kCB<BITS>; ++b) C[u][b][w] = (start >> b) & 1u ? ~0u : 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            uint32_t live = M[u][0] | M[u][1] | M[u][2] | M[u][3];
            for (uint32_t j0 = 0; j0 < f1; j0 += 8) {
                p3_add<BITS>(M[u], C[u], t[u], a.y, j0, j0 + 8 < f1 ? j0 + 8 : f1);
                live = M[u][0] | M[u][1] | M[u][2] | M[u][3];
                if (!__any(live != 0)) break;
            }
            if (a.m > 32) {  // a lane has live positions after 32 pattern positions
                unsigned long long todo = __ballot(live != 0);
                while (todo) {
                    const int src = __builtin_ctzll(todo);  // wave-uniform
                    todo &= todo - 1;
                    const uint64_t dw = (cw + (uint64_t)u * kP3T + (uint32_t)src) * kChunk;
                    uint32_t R[kChunk], Cs[kCB<BITS>][kChunk];
#pragma unroll
                    for (uint32_t w = 0; w < kChunk; ++w) {
                        R[w] = __builtin_amdgcn_readlane(M[u][w], src);
#pragma unroll
                        for (int b = 0; b < kCB<BITS>; ++b) Cs[b][w] = BITS ? __builtin_amdgcn_readlane(C[u][b][w], src) : 0u;
                    }
                    p3_verify<BITS>(R, Cs, a, dw);
                    if (lane == (uint32_t)src) {
#pragma unroll
                        for (uint32_t w = 0; w < kChunk; ++w) {
                            M[u][w] = R[w];
#pragma unroll
                            for (int b = 0; b < kCB<BITS>; ++b) C[u][b][w] = Cs[b][w];
                        }
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
                const uint64_t pos = (cw + (uint64_t)u * kP3T + lane) * kPos;
                const uint32_t bias = a.foreign - (BITS ? start : 0u);  // distance = counter - start + the positions the host counted
#pragma unroll
                for (uint32_t w = 0; w < kChunk; ++w) {
                    uint32_t r = M[u][w];
                    while (r) {
                        const uint32_t i = __builtin_ctz(r);
                        r &= r - 1;
                        uint32_t dist = bias;
#pragma unroll
                        for (int b = 0; b < BITS; ++b) dist += ((C[u][b][w] >> i) & 1u) << b;
                        if (slot < cap) out[slot] = (pos + 32 * w + i) << a.shift | dist;
                        ++slot;
                    }
                }
            }
        }
    }
    if constexpr (!FIND) flush_hits(hits, a.count, smem, reinterpret_cast<const uint8_t*>(a.p0));
}

template <int BITS>
__global__ __launch_bounds__(kP3T, kP3Waves) void planes3_scan(Plane3Args a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // 128 bytes: flush_hits
    planes3_body<BITS, false>(a, smem, nullptr, 0);
}

template <int BITS>
__global__ __launch_bounds__(kP3T, kP3Waves) void planes3_find(Plane3Args a, unsigned long long* __restrict__ out, unsigned long long cap)
{
    planes3_body<BITS, true>(a, nullptr, out, cap);
}

// Grid: launch_planes_scan's with p3_wgs workgroups per CU.  BITS from the budget: 0 / 1 / 2 / 3 for 0 / 1 / at most 3 / at most 7.
static int p3_bits(uint32_t budget) { return budget == 0 ? 0 : budget <= 1 ? 1 : budget <= 3 ? 2 : 3; }

static uint32_t planes3_grid(const Plane3Args& a, int num_cus, int bits, bool find)
{
    constexpr uint64_t kPos = 32 * kChunk;
    const uint64_t chunks = (a.s_end + kPos - 1) / kPos - a.s_begin / kPos;
    const uint64_t want = (chunks + kP3T * kUnroll - 1) / (kP3T * kUnroll);
    return (uint32_t)std::min<uint64_t>(want, (uint64_t)num_cus * p3_wgs(bits, find));
}

static hipError_t launch_planes3_scan(const Plane3Args& a, int planes, int num_cus, hipStream_t stream)
{
    if (planes != kPlanes3 || a.budget > SMARTGPU_PMIS_MAX) return hipErrorInvalidValue;
    if (a.s_end <= a.s_begin) return hipSuccess;
    const int bits = p3_bits(a.budget);
    const uint32_t grid = planes3_grid(a, num_cus, bits, false);
#define SG_P3_SCAN(b_) hipLaunchKernelGGL((planes3_scan<b_>), dim3(grid), dim3(kP3T), 128, stream, a)
    if (bits == 0) SG_P3_SCAN(0); else if (bits == 1) SG_P3_SCAN(1); else if (bits == 2) SG_P3_SCAN(2); else SG_P3_SCAN(3);
#undef SG_P3_SCAN
    return hipGetLastError();
}

static hipError_t launch_planes3_find(const Plane3Args& a, unsigned long long* out, unsigned long long cap, int planes, int num_cus,
                                      hipStream_t stream)
{
    if (planes != kPlanes3 || a.budget > SMARTGPU_PMIS_MAX) return hipErrorInvalidValue;
    if (a.s_end <= a.s_begin) return hipSuccess;
    const int bits = p3_bits(a.budget);
    const uint32_t grid = planes3_grid(a, num_cus, bits, true);
#define SG_P3_FIND(b_) hipLaunchKernelGGL((planes3_find<b_>), dim3(grid), dim3(kP3T), 0, stream, a, out, cap)
    if (bits == 0) SG_P3_FIND(0); else if (bits == 1) SG_P3_FIND(1); else if (bits == 2) SG_P3_FIND(2); else SG_P3_FIND(3);
#undef SG_P3_FIND
    return hipGetLastError();
}

// match_calls.cpp reaches the launchers once this unit is part of the program (planes3.hpp)
namespace {
struct RegisterPlanes3 {
    RegisterPlanes3()
    {
        g_planes3_pack = &launch_planes3_pack;
        g_planes3_scan = &launch_planes3_scan;
        g_planes3_find = &launch_planes3_find;
    }
} g_register_planes3;
}  // namespace

}  // namespace sg
