// k_horm.hip — hor_multi_scan: Horspool (and Tuned BM) on hor_scan's LDS tiles for up to 32 patterns of one length
// in ONE pass over the text (a translation unit of its own: dev_common.hpp says why)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "multi.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// hor_scan<.., VAR 0> (k_hor.hip) with the tile staged ONCE for np <= NP patterns: searches of one text that are queued
// together (api.cpp) share the fetch and HBM bytes per pattern fall by np.  Same tiles on absolute offsets indexed by
// window end, same back halo, same prefetch one tile ahead, same swizzle, same range clamps.
// LDS: u64 blob[32] | u64 count[32] | u64 hits[32] | u32 gram[kGramSlots] | np x pattern tail P[m-1-H..m-1] | text [tile0-H16, tile0+TB)
// The walk: a Horspool walk per pattern asks np times, one pattern at a time, whether a pattern ends near a window end,
// and np such walks of a staged tile cost more than its fetch.  ONE walk per lane asks it for all patterns at once:
// the workgroup builds, in its prologue, the skip table of multi.hpp — indexed by the window's last two bytes, the
// least shift any pattern of the pass allows and the CLASSES of the patterns whose last gram falls into the slot (LDS
// atomics: min for the shifts, a barrier, or for the class bits and the tag of the last gram).  An entry has eight
// class bits and a pass up to kMultiMax = 32 patterns: pattern g is of class g & 7, and a window whose entry passes the
// tag test is compared with the patterns c, c + 8, c + 16, c + 24 below np of every class c that is set.  A gram hit is
// rare (about np / 16384 per step on rand128) and a class mate that is not the pattern dies on its first byte; counts
// stay exact because every compare is a whole one.  A pass of at most eight has one pattern per class: nothing changes.
// np x (m - 2) grams hardly fill
// kGramSlots slots, so nearly every step moves the window end by m - 1 and a lane leaves its 64-byte segment after
// about 64 / (m - 1) steps whatever np is.  A step: two byte reads (tile_at permutes dwords, the two bytes of a gram
// may lie in different ones), the slot, the entry; compare for every pattern of every class bit, but only where the entry's tag
// says that the window ends in a pattern's last gram and not merely in its slot; add the shift.
// The prologue reads no pattern from memory: the bytes the table and the tails are made of, at most 65 per pattern,
// come BY VALUE in the rows of MultiArgs (multi.hpp), each thread reads its few of them from the arguments first, and
// the first tile is asked for before the table is built — measured, a pass of eight fell from 167-170 us to 164-165 us
// against a solo hor_scan's 156 us (1 GiB rand128, m = 32; profiles/coalesce/RESULTS.md); the tag took it to 162-163.
// The arguments are 3112 bytes at 32 patterns, with tile_first and ntiles 3124 of the 4096 a kernel may take
// (multi.hpp asserts it).  The pointer arrays of MultiArgs are read once, in the prologue: thread g < np takes blob[g]
// and count[g] from the argument segment AS NUMBERS and writes them to LDS — one thread filling all 32 would unroll
// into 64 selects, and a pointer picked by a run-time index and then dereferenced is loaded through flat_load;
// a pattern's pointer — needed only to complete a window in memory — is read from LDS as a number and cast to GLOBAL
// memory.  The kernel is as long as hor_scan
// whatever NP is, so NP, the most patterns a pass can take, is instantiated once, at kMultiMax, and completion in
// memory (m - 1 > H) is a run-time branch of that one kernel, taken by rare candidates only: the product library has a
// size to keep (tests/test_abi.py holds it below 0.7 of the A/B build).
// Counts: an occurrence is rare for a streaming pattern (the only kind that gets here), so a lane adds each one straight
// to its pattern's LDS counter, and at the end the workgroup adds every non-zero counter to that pattern's result slot.
// Not through the staging slots of flush_hits: those assume ONE flush per grid, and here a grid flushes np sums.
// ---------------------------------------------------------------------------
constexpr uint32_t kHormHead = 3 * 8 * kMultiMax;  // the three u64 arrays in front of the skip table
constexpr uint32_t kHormGram = 4 * kGramSlots;    // the skip table
static_assert(kHormHead % 64 == 0 && kHormGram % 64 == 0, "the tails and the tile stay 16-byte aligned");

// a pointer into global memory from the number an LDS slot holds (per lane: lanes may ask for different patterns)
__device__ __forceinline__ const uint8_t* horm_global(unsigned long long v)
{
    typedef const __attribute__((address_space(1))) uint8_t* global_u8;
    return (const uint8_t*)reinterpret_cast<global_u8>(v);
}

// a 64-bit value of the first active lane / of lane `src`, wave-uniform.  The halves go through uint32_t: the builtins
// return int, and an int OR-ed into 64 bits is sign-extended — a pointer whose low word has bit 31 set would come out
// with its high word all ones.
__device__ __forceinline__ unsigned long long horm_first(unsigned long long v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long horm_lane(unsigned long long v, int src)
{
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, src), hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

// wave_verify (dev_common.hpp) with the pattern as well as the text pointer taken from the parked lane: the candidates
// a wave has parked may belong to different patterns.  Returns 1 in the lane whose candidate verified, 0 elsewhere.
__device__ __forceinline__ uint32_t horm_wave_verify(bool has, const uint8_t* tptr, const uint8_t* pptr, uint32_t len)
{
    unsigned long long todo = __ballot(has);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t mine = 0;
    while (todo) {
        const int src = __builtin_ctzll(todo);  // wave-uniform
        todo &= todo - 1;
        const uint8_t* t = horm_global(horm_lane((unsigned long long)tptr, src));
        const uint8_t* p = horm_global(horm_lane((unsigned long long)pptr, src));
        bool diff = false;
        for (uint32_t off = lane * 16u; off < len; off += 1024u)
            diff |= differ16(t + off, p + off, len - off < 16 ? len - off : 16u);
        if (!__any(diff) && lane == (uint32_t)src) mine = 1;
    }
    return mine;
}

template <int THREADS, int L, int NP>
__global__ __launch_bounds__(THREADS) void hor_multi_scan(MultiArgs a, uint64_t tile_first, uint32_t ntiles)
{
    constexpr int TB = THREADS * L;
    static_assert(NP == kMultiMax && NP <= 4 * (int)kGramClasses && NP <= THREADS, "a class bit in an entry's byte 2 stands for at most four patterns");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t m = a.m, H = a.halo, H16 = round16(H), np = a.np;
    const bool in_memory = m - 1 > H;  // windows are completed in HBM
    const uint32_t tslot = round16(H + 1);  // one pattern's tail; ptail[H-k] == P[m-1-k]
    unsigned long long* blobs = reinterpret_cast<unsigned long long*>(smem);
    unsigned long long* counts = blobs + kMultiMax;
    unsigned long long* sums = counts + kMultiMax;
    uint32_t* gram = reinterpret_cast<uint32_t*>(smem + kHormHead);
    uint8_t* tails = smem + kHormHead + kHormGram;
    uint8_t* txt = tails + np * tslot;  // txt[H16 + x] == T[tile0 + x]

    // What this thread takes of the rows in the arguments (multi.hpp), read before anything else: every address is the
    // arguments' plus an index of the thread's, so no read waits for another.  Loads come back in the order they
    // were sent, so these go out in front of the tile's and the table is built while the tile is on the way.  A thread
    // with nothing to take reads a byte that exists all the same (m >= 3): no branch, no wait between the reads.
    // The rounds beyond a pass of eight stand behind a test of np, the same for the whole workgroup: a pass of at most
    // eight sends the reads of its own patterns only.
    constexpr uint32_t kTslotMax = (kHaloMax + 16u) & ~15u;                // the longest tail, rounded: 32
    constexpr uint32_t kTailPer = THREADS / kTslotMax;                     // 8 patterns' tails in a round
    constexpr uint32_t kTailRounds = kMultiMax / kTailPer;                 // 4
    constexpr uint32_t kShiftPer = THREADS / kGramCap;                     // 4 patterns' grams in a round
    constexpr uint32_t kShiftRounds = kMultiMax / kShiftPer;               // 8
    static_assert(kTailRounds * kTailPer == kMultiMax && kShiftRounds * kShiftPer == kMultiMax && kTailPer * kTslotMax == THREADS && kShiftPer * kGramCap == THREADS,
                  "kTailRounds tail bytes and kShiftRounds grams per thread");
    // tails: in round r thread x takes byte x % 32 of pattern x / 32 + 8 r: ptail[j] = P[m-1-H+j], j <= H
    const uint32_t tail_j = threadIdx.x % kTslotMax;
    uint32_t tail_byte[kTailRounds];
#pragma unroll
    for (uint32_t r = 0; r < kTailRounds; ++r) {
        tail_byte[r] = 0;
        if (r == 0 || np > r * kTailPer) {
            const uint32_t g = threadIdx.x / kTslotMax + r * kTailPer;
            const bool mine = g < np && tail_j <= H;
            tail_byte[r] = tail_at(a.tail[mine ? g : 0u], m, m - 1 - (mine ? H - tail_j : 0u));
        }
    }
    // shifts: in round r thread x takes the gram at position gram_first(m) + x % kGramCap of pattern x / kGramCap + 4 r,
    // both bytes in one read (at most kGramCap - 1 positions of a pattern shift by less than the default)
    const uint32_t shift_i = gram_first(m) + threadIdx.x % kGramCap;
    const bool shift_mine = shift_i + 3 <= m;
    uint32_t shift_gram[kShiftRounds];
#pragma unroll
    for (uint32_t r = 0; r < kShiftRounds; ++r) {
        shift_gram[r] = 0;
        if (r * kShiftPer < 8 || np > r * kShiftPer) {
            const uint32_t g = threadIdx.x / kGramCap + r * kShiftPer;
            shift_gram[r] = tail_gram_at(a.tail[g < np ? g : 0u], m, shift_mine ? shift_i : gram_first(m));
        }
    }
    // class bits: thread g < np takes pattern g's last gram — and its blob and its result slot, as numbers
    const uint32_t bit_g = threadIdx.x < np ? threadIdx.x : 0u;
    const uint32_t bit_gram = tail_gram_at(a.tail[bit_g], m, m - 2);
    const unsigned long long head_blob = (unsigned long long)a.blob[bit_g], head_count = (unsigned long long)a.count[bit_g];

    const uint64_t e_begin = a.s_begin + m - 1, e_end = a.s_end + m - 1;
    const uint64_t t_end = tile_first + ntiles;
    static_assert(TB == THREADS * 64, "prefetch registers are written out for L = 64");
    uint4 p0, p1, p2, p3, ph;  // prefetch registers: 4 tile rows + one halo chunk
    const bool halo_lane = threadIdx.x * 16u < H16;
    auto issue = [&](uint64_t tile0) {
        const uint8_t* src = a.text + tile0 + threadIdx.x * 16u;
        p0 = ld_stream16(src);
        p1 = ld_stream16(src + THREADS * 16);
        p2 = ld_stream16(src + THREADS * 32);
        p3 = ld_stream16(src + THREADS * 48);
        if (halo_lane) ph = ld_stream16(src - H16);
    };
    uint64_t t = tile_first + blockIdx.x;
    issue(t * TB);  // (the launcher starts no more workgroups than there are tiles)

    // the table and the tails, in LDS: the default, a barrier, the least shift per slot, a barrier, the pattern bits
    if (threadIdx.x < (uint32_t)NP) {
        blobs[threadIdx.x] = threadIdx.x < np ? head_blob : 0ull;
        counts[threadIdx.x] = threadIdx.x < np ? head_count : 0ull;
        sums[threadIdx.x] = 0;
    }
    const uint32_t dflt = gram_default(m);
    for (uint32_t j = threadIdx.x; j < kGramSlots; j += THREADS) gram[j] = dflt;
#pragma unroll
    for (uint32_t r = 0; r < kTailRounds; ++r) {
        const uint32_t g = threadIdx.x / kTslotMax + r * kTailPer;
        if (g < np && tail_j <= H) tails[g * tslot + tail_j] = (uint8_t)tail_byte[r];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kShiftRounds; ++r)
        if (threadIdx.x / kGramCap + r * kShiftPer < np && shift_mine) atomicMin(gram + gram_slot(shift_gram[r] & 0xFFu, shift_gram[r] >> 8), gram_shift(m, shift_i));
    __syncthreads();  // every shift is in before a class bit makes an entry larger
    if (threadIdx.x < np) atomicOr(gram + gram_slot(bit_gram & 0xFFu, bit_gram >> 8), gram_entry_class_bit(threadIdx.x) | gram_entry_tag(bit_gram & 0xFFu));
    // (the loop's first barrier stands between these bits and the first walk)

    for (; t < t_end; t += gridDim.x) {
        const uint64_t tile0 = t * TB;
        __syncthreads();  // previous tile fully consumed (and tables visible)
        {
            const uint32_t i0 = H16 + threadIdx.x * 16u;
            tile_park(txt, i0, p0);
            tile_park(txt, i0 + THREADS * 16, p1);
            tile_park(txt, i0 + THREADS * 32, p2);
            tile_park(txt, i0 + THREADS * 48, p3);
            if (halo_lane) tile_park(txt, threadIdx.x * 16u, ph);
        }
        __syncthreads();
        if (t + gridDim.x < t_end) issue((t + gridDim.x) * TB);
        const uint64_t seg = tile0 + (uint64_t)threadIdx.x * L;
        const uint64_t lo = seg > e_begin ? seg : e_begin;
        const uint64_t hi = seg + L < e_end ? seg + L : e_end;
        // the lane's window ends of this tile, [e0, ehi) in tile coordinates; none: the lane starts finished
        const bool any = lo < hi;
        const uint32_t e0 = any ? (uint32_t)(lo - tile0) + H16 : H16;
        const uint32_t ehi = any ? (uint32_t)(hi - tile0) + H16 : H16;
        bool parked = false;  // first candidate of this tile awaiting the wave-wide compare, and its pattern
        uint32_t parked_g = 0;
        const uint8_t* parked_at = a.text;
        // the staged tile, walked once for all patterns (a lane without a window end has e0 == ehi)
        for (uint32_t e = e0; e < ehi;) {
            const uint32_t prev = txt[tile_at(e - 1)], last = txt[tile_at(e)];  // e >= H16 >= 16: e - 1 is in the halo at least
            const uint32_t ent = gram[gram_slot(prev, last)];
            for (uint32_t cls = gram_entry_hit(ent, prev); cls != 0; cls &= cls - 1) {  // (a slot hit that is no gram hit: no compare)
                // the class's patterns below np: a mate that is not the pattern dies on its first byte, almost always
                for (uint32_t g = __builtin_ctz(cls); g < np; g += kGramClasses) {
                    const uint8_t* ptail = tails + g * tslot;
                    uint32_t k = 0;  // bytes matched so far, right to left (the slot promises none of them)
                    while (k <= H && ptail[H - k] == txt[tile_at(e - k)]) ++k;
                    bool ok = k == H + 1;
                    if (in_memory && ok) {  // the rest of the window is not in LDS
                        const uint8_t* rest = a.text + tile0 + (e - H16) - (m - 1);
                        if (!parked) {
                            parked = true;
                            parked_at = rest;
                            parked_g = g;
                            ok = false;  // counted after the loop
                        } else {
                            ok = global_equal(rest, horm_global(blobs[g]), m - 1 - H);
                        }
                    }
                    if (ok) atomicAdd(sums + g, 1ull);
                }
            }
            e += gram_entry_shift(ent);
        }
        if (in_memory && horm_wave_verify(parked, parked_at, horm_global(blobs[parked_g]), m - 1 - H)) atomicAdd(sums + parked_g, 1ull);
    }

    // the workgroup's np sums, each straight to its pattern's result slot
    __syncthreads();
    if (threadIdx.x < np && sums[threadIdx.x] != 0) {
        typedef __attribute__((address_space(1))) unsigned long long* global_u64;
        atomicAdd((unsigned long long*)reinterpret_cast<global_u64>(counts[threadIdx.x]), sums[threadIdx.x]);
    }
}

// ---------------------------------------------------------------------------
// launcher: the grid and the tile's LDS as launch_hor's streaming branch, plus the skip table and the tails of np patterns
// ---------------------------------------------------------------------------
// Workgroups per CU.  A workgroup takes up to 33.8 KB of LDS (the table 16 KB of it) and 62 VGPRs, so four are resident
// at most — and with the table of 2048 slots, where six were, FOUR won: swept on 1 GiB of rand128 at m = 16, 32, 256 in
// groups of 2, 4, 8 (8 patterns, m = 32: 0.0207 ms per pattern with 4, 0.0215 with 5, 0.0214 with 6, 0.0222 with 7), and
// at m = 16, 32, 64, 256 in groups of 8 to 32, where 5 won a pass of 32 at m = 32 alone (0.0059 against 0.0063) and lost
// at the other lengths by 2 - 5 % (profiles/coalesce/RESULTS.md) — the solo kernels' value.
static int horm_wgs(uint32_t m)
{
    ScanArgs one = {};
    one.m = m;
    one.sparse = 1;
    return tile_wgs(one);
}

hipError_t launch_hor_multi(const MultiArgs& a, int num_cus, hipStream_t stream)
{
    if (a.np < 1 || a.np > (uint32_t)kMultiMax || a.m < 3 || a.halo < 1 || a.halo > kHaloMax || a.halo > a.m - 1) return hipErrorInvalidValue;  // (a gram and the byte before a lane's first window end exist)
    const uint32_t m = a.m, H = a.halo;
    const TileRange tr = tiles_for(a.s_begin + m - 1, a.s_end + m - 1, (uint64_t)kHorT * kHorL);
    if (tr.count == 0) return hipSuccess;
    const size_t lds = kHormHead + kHormGram + (size_t)a.np * r16(H + 1) + ((r16(H) + (size_t)kHorT * kHorL + 16 + 63) & ~(size_t)63);  // whole 64-byte blocks: tile_at() permutes inside them
    const int wgs_per_cu = g_tune[4] ? g_tune[4] : horm_wgs(m);  // smartgpu_tune(4, .) applies
    uint32_t grid = (uint32_t)num_cus * (uint32_t)wgs_per_cu;
    if (grid > tr.count) grid = tr.count;
    hipLaunchKernelGGL((hor_multi_scan<kHorT, kHorL, kMultiMax>), dim3(grid), dim3(kHorT), lds, stream, a, tr.first, tr.count);
    return hipGetLastError();
}

// api.cpp queues launches only once this unit is part of the program
namespace {
struct RegisterHorMulti {
    RegisterHorMulti() { g_hor_multi = &launch_hor_multi; }
} g_register_hor_multi;
}  // namespace

}  // namespace sg
