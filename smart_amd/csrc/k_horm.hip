// k_horm.hip — hor_multi_scan: Horspool (and Tuned BM) on hor_scan's LDS tiles for up to kPassMax = 96 patterns of one
// length in ONE pass over the text (a translation unit of its own: dev_common.hpp says why)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "multi.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// hor_scan<.., VAR 0> (k_hor.hip) with the tile staged ONCE for the np patterns of a pass: searches of one text that are
// queued together (api.cpp) share the fetch and HBM bytes per pattern fall by np.  Same tiles on absolute offsets indexed
// by window end, same back halo, same prefetch one tile ahead, same swizzle, same range clamps.
// LDS: u8 gram[kGramSlots] | u32 heads[kGramBuckets] | u32 next[kPassMax] | u32 sums[kPassMax] | np rows | text [tile0-H16, tile0+TB)
// The walk: a Horspool walk per pattern asks np times, one pattern at a time, whether a pattern ends near a window end,
// and np such walks of a staged tile cost more than its fetch.  ONE walk per lane asks it for all patterns at once:
// the workgroup builds, in its prologue, the skip table of multi.hpp — one BYTE per slot, indexed by the window's last
// two bytes: the least shift any pattern of the pass allows, and a bit that says that some pattern's last gram falls
// into the slot.  LDS has no byte atomics: a shift is entered with a compare-and-swap on the dword that holds the byte
// (horm_byte_min), the bit after a barrier with an OR.  A step: two byte reads (tile_at permutes dwords, the two bytes
// of a gram may lie in different ones), the slot, the entry, add the shift.  np x (m - 2) grams hardly fill 16384
// slots, and the slot function is exact on 7-bit symbols, so nearly every step moves the window end by m - 1 and a lane
// leaves its 64-byte segment after about 64 / (m - 1) steps whatever np is.
// The candidates: a window whose entry has the bit follows the chain of its gram's bucket — heads[gram_bucket], then
// next[g]; pattern g + 1 stands for g, 0 ends the chain; thread g < np links pattern g in with one atomicExch — and is
// compared, whole, right to left, with each pattern on it.  A hit is rare (about np / 16384 per step on rand128), a
// chain holds one pattern and seldom two, and a pattern of the bucket that is not the window's dies on its first bytes;
// counts stay exact because every compare is a whole one.  The same pattern twice in a pass is twice on its chain.
// The prologue reads no pattern from memory: the rows of the pass come BY VALUE in the arguments' area (multi.hpp), at
// the stride of their own length; thread x copies 16 bytes of them to LDS with ONE read, sent before the first tile is
// asked for, and the table is built from LDS while the tile is on the way.  A row in LDS is also what a lane compares a
// window with (its last H + 1 stored bytes).  A narrow pass sends few reads: np x stride / 16.
// A LONG pass (multi.hpp: MultiArgs::reserved == kMultiLong) holds more patterns than the arguments have room for by
// value — up to long_width(m): 252 up to m = 16, 152 up to m = 32, 108, 84, 68 beyond — and carries pointers only:
// its prologue reads each row from the front of the pattern's blob, one dependent read (the pointer from the
// arguments, then 16 bytes of the pattern), still sent before the first tile is asked for.  Its links and sums take np
// entries each, behind the rows: u8 gram | u32 heads | np rows | u32 next[np] | u32 sums[np] | text.  From the first
// barrier on the two kinds of pass run the same code over pointers that differ.
// The arguments are 4080 bytes, with tile_first and ntiles 4092 of the 4096 a kernel may take (multi.hpp asserts it).
// The pointers in the area are read as numbers and cast to GLOBAL memory: thread g < np keeps count[g] in registers
// from the prologue to the end; blob[g] is read by the rare lane that completes a window in memory.
// One instantiation; completion in memory (m - 1 > H) is a run-time branch of it, taken by rare candidates only: the
// product library has a size to keep (tests/test_abi.py holds it below 0.7 of the A/B build).
// Counts: a lane adds each occurrence straight to its pattern's LDS counter, and at the end the workgroup adds every
// non-zero counter to that pattern's result slot.  For a streaming pattern an occurrence is rare.  Not every pattern
// of a pass is one: a RIDER (api.cpp queue_launch) is a pattern whose own symbols repeat, over a text whose symbols do
// not, and it may occur often — a planted periodic run gives an occurrence every period, several to a lane's 64 window
// ends and in every lane of a wave.  Nothing here needs occurrences to be rare for the count to be right:
//  * A counter is a u32 PER PATTERN: a workgroup counts at most one occurrence per window end and pattern, and the
//    launcher gives no workgroup more than 2^17 tiles of 2^14 window ends (launch_hor_multi), so 2^31 bounds it however
//    often the pattern occurs.  The same pattern twice in a pass has two counters.
//  * A lane parks ONE candidate per tile for the wave-wide compare (the first whose end matched in LDS) and completes
//    every further one itself (global_equal): parking is a choice of who does the compare, no candidate is dropped.
//  * horm_wave_verify takes the parked lanes one at a time, each with its own text and pattern pointer, so a wave in
//    which all 64 lanes have parked does 64 compares; frequent occurrences cost time there, not correctness.
// Many adds to one LDS counter serialise, which is what a frequent rider pays (tests/test_coalesce_ride_gpu.py has one).
// Not through the staging slots of flush_hits: those assume ONE flush per grid, and here a grid flushes np sums.
// ---------------------------------------------------------------------------
constexpr uint32_t kHormHead = kGramSlots + 4 * (kGramBuckets + 2 * kPassMax);  // the table, the heads, the links and the sums
static_assert(kHormHead % 64 == 0, "the rows stay 16-byte aligned and the tile 64-byte aligned");
// four workgroups per CU: 160 KB of LDS, allocated in blocks of at most 2 KB
static_assert(kHormHead + ((kPassMax * 16u + 63u) & ~63u) + 16448u <= 40960u && kHormHead + ((50u * 64u + 63u) & ~63u) + 16448u <= 40960u &&
              kHormHead + ((42u * kTailRow + 63u) & ~63u) + 16448u <= 40960u, "the widest pass of every row stride leaves four workgroups per CU resident");

// (a long pass: multi.hpp asserts the same of long_head at every long_width, with this tile)
static_assert(kHaloMax == 16 && kMultiTileLds == ((16u + (uint32_t)kHorT * kHorL + 16u + 63u) & ~63u) && kMultiLdsBudget == 40960u, "the tile that multi.hpp's LDS budget counts");

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

// the least of the byte at `slot` and s, in a table of bytes that has no byte atomics: compare-and-swap on its dword.
// (Bit 7 of every byte is still clear: the hit bits are set after a barrier.)
__device__ __forceinline__ void horm_byte_min(uint8_t* table, uint32_t slot, uint32_t s)
{
    uint32_t* const word = reinterpret_cast<uint32_t*>(table + (slot & ~3u));
    const uint32_t sh = 8u * (slot & 3u);
    uint32_t old = *word;
    while (((old >> sh) & 0xFFu) > s) {
        const uint32_t seen = atomicCAS(word, old, (old & ~(0xFFu << sh)) | (s << sh));
        if (seen == old) break;
        old = seen;
    }
}

// a u64 of the arguments' area as a number, at an offset of the lane's own
__device__ __forceinline__ unsigned long long horm_area64(const MultiArgs& a, uint32_t at)
{
    return *reinterpret_cast<const unsigned long long*>(a.area + at);
}

// 16 bytes of a pattern in global memory, at any alignment, in one read
__device__ __forceinline__ uint4 horm_row16(const uint8_t* p)
{
    uint4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

template <int THREADS, int L>
__global__ __launch_bounds__(THREADS) void hor_multi_scan(MultiArgs a, uint64_t tile_first, uint32_t ntiles)
{
    constexpr int TB = THREADS * L;
    static_assert(kPassMax <= THREADS && THREADS % (int)kGramCap == 0, "a thread per pattern; the grams of THREADS / kGramCap patterns in a round");
    static_assert(THREADS == (int)kMultiThreads && kLongMax <= (uint32_t)THREADS && kMultiLdsBudget - kMultiTileLds - kGramSlots - 4u * kGramBuckets <= 2u * THREADS * 16u,
                  "a long pass: a thread per pattern, and the rows that the LDS has room for in two pieces per thread");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t m = a.m, H = a.halo, H16 = round16(H), np = a.np, W = a.width, stride = a.stride;
    const bool in_memory = m - 1 > H;  // windows are completed in HBM
    const bool by_value = a.reserved == kMultiByValue;  // the area's layout (multi.hpp): rows in the arguments, or a long pass
    const uint32_t rlast = m - 1 - gram_first(m);  // P[m-1-k] is byte rlast - k of a row
    const uint32_t row_bytes = np * stride;        // a multiple of 16
    const uint32_t nlink = by_value ? (uint32_t)kPassMax : np;  // links and sums: kHormHead's by value, np each in a long pass
    uint8_t* gram = smem;
    uint32_t* heads = reinterpret_cast<uint32_t*>(smem + kGramSlots);
    uint8_t* rows = by_value ? smem + kHormHead : smem + kGramSlots + 4 * kGramBuckets;
    uint32_t* next = by_value ? heads + kGramBuckets : reinterpret_cast<uint32_t*>(rows + row_bytes);
    uint32_t* sums = next + nlink;
    uint8_t* txt = by_value ? rows + ((row_bytes + 63u) & ~63u) : smem + long_head(np, stride);  // txt[H16 + x] == T[tile0 + x]

    // What this thread takes of the arguments' area (multi.hpp), read before anything else: 16 bytes of the rows, and
    // (thread g < np) the result slot of pattern g as a number.  Loads come back in the order they were sent, so these
    // go out in front of the tile's and the table is built while the tile is on the way.
    // A long pass has no rows in its area: the thread reads blob[g] there and its 16 bytes from the pattern at the front
    // of that blob, blob[g] + gram_first(m) + offset — at no alignment from m = 66 on — and, where np rows are more
    // than THREADS pieces, a second piece THREADS further on.  A row's last piece reaches up to 15 bytes behind the
    // pattern's end: still inside the blob's pattern slot (api.cpp asserts it), and no byte behind tail_stored(m) is
    // ever looked at (the grams end at m - 1, a compare starts there and goes left).
    const bool row_mine = threadIdx.x * 16u < row_bytes;
    bool row_mine2 = false;
    uint4 row16 = {}, row16b = {};
    if (by_value) {
        if (row_mine) row16 = *reinterpret_cast<const uint4*>(a.area + multi_rows_at(W) + threadIdx.x * 16u);
    } else {
        const uint32_t pieces = stride / 16u, second = threadIdx.x + THREADS;
        row_mine2 = second * 16u < row_bytes;
        if (row_mine) {
            const uint32_t g = threadIdx.x / pieces;
            row16 = horm_row16(horm_global(horm_area64(a, multi_blob_at(g))) + gram_first(m) + (threadIdx.x - g * pieces) * 16u);
        }
        if (row_mine2) {
            const uint32_t g = second / pieces;
            row16b = horm_row16(horm_global(horm_area64(a, multi_blob_at(g))) + gram_first(m) + (second - g * pieces) * 16u);
        }
    }
    unsigned long long head_count = 0;
    if (threadIdx.x < np) head_count = horm_area64(a, multi_count_at(W, threadIdx.x));

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

    // the table, the chains and the rows, in LDS: the default and the rows, a barrier, the least shift per slot, a
    // barrier, the hit bits and the links
    {
        const uint32_t dflt = gram_default(m) * 0x01010101u;
        const uint4 dflt16 = {dflt, dflt, dflt, dflt};
        for (uint32_t j = threadIdx.x * 16u; j < kGramSlots; j += THREADS * 16u) *reinterpret_cast<uint4*>(gram + j) = dflt16;
        for (uint32_t j = threadIdx.x; j < kGramBuckets; j += THREADS) heads[j] = 0;
        if (threadIdx.x < nlink) sums[threadIdx.x] = 0;
        if (row_mine) *reinterpret_cast<uint4*>(rows + threadIdx.x * 16u) = row16;
        if (row_mine2) *reinterpret_cast<uint4*>(rows + (threadIdx.x + THREADS) * 16u) = row16b;
    }
    __syncthreads();
    {
        // shifts: in a round, thread x takes the gram at position gram_first(m) + x % kGramCap of pattern x / kGramCap +
        // (THREADS / kGramCap) r (at most kGramCap - 1 positions of a pattern shift by less than the default); the
        // rounds a pass takes follow np, the same for the whole workgroup
        const uint32_t shift_i = gram_first(m) + threadIdx.x % kGramCap;
        if (shift_i + 3 <= m)
            for (uint32_t g = threadIdx.x / kGramCap; g < np; g += THREADS / kGramCap) {
                const uint32_t two = tail_gram_at(rows + g * stride, m, shift_i);
                horm_byte_min(gram, gram_slot(two & 0xFFu, two >> 8), gram_shift(m, shift_i));
            }
    }
    __syncthreads();  // every shift is in before a hit bit makes a byte larger
    if (threadIdx.x < np) {
        const uint32_t two = tail_gram_at(rows + threadIdx.x * stride, m, m - 2);
        const uint32_t slot = gram_slot(two & 0xFFu, two >> 8);
        atomicOr(reinterpret_cast<uint32_t*>(gram + (slot & ~3u)), kGramHit << (8u * (slot & 3u)));
        next[threadIdx.x] = atomicExch(heads + gram_bucket(two & 0xFFu, two >> 8), threadIdx.x + 1u);
    }
    // (the loop's first barrier stands between these and the first walk)

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
        bool parked = false;  // first candidate of this tile awaiting the wave-wide compare, its pattern and that pattern's blob
        uint32_t parked_g = 0;
        const uint8_t* parked_at = a.text;
        unsigned long long parked_blob = (unsigned long long)a.text;
        // the staged tile, walked once for all patterns (a lane without a window end has e0 == ehi)
        for (uint32_t e = e0; e < ehi;) {
            const uint32_t prev = txt[tile_at(e - 1)], last = txt[tile_at(e)];  // e >= H16 >= 16: e - 1 is in the halo at least
            const uint32_t ent = gram[gram_slot(prev, last)];
            if (gram_byte_hit(ent)) {
                // the patterns of the gram's bucket: one that is not the window's dies on its first bytes
                for (uint32_t c = heads[gram_bucket(prev, last)]; c != 0; c = next[c - 1u]) {
                    const uint32_t g = c - 1u;
                    const uint8_t* prow = rows + g * stride;
                    uint32_t k = 0;  // bytes matched so far, right to left (the slot promises none of them)
                    while (k <= H && prow[rlast - k] == txt[tile_at(e - k)]) ++k;
                    bool ok = k == H + 1;
                    if (in_memory && ok) {  // the rest of the window is not in LDS
                        const uint8_t* rest = a.text + tile0 + (e - H16) - (m - 1);
                        const unsigned long long blob = horm_area64(a, multi_blob_at(g));
                        if (!parked) {
                            parked = true;
                            parked_at = rest;
                            parked_g = g;
                            parked_blob = blob;
                            ok = false;  // counted after the loop
                        } else {
                            ok = global_equal(rest, horm_global(blob), m - 1 - H);
                        }
                    }
                    if (ok) atomicAdd(sums + g, 1u);
                }
            }
            e += gram_byte_shift(ent);
        }
        if (in_memory && horm_wave_verify(parked, parked_at, horm_global(parked_blob), m - 1 - H)) atomicAdd(sums + parked_g, 1u);
    }

    // the workgroup's np sums, each straight to its pattern's result slot
    __syncthreads();
    if (threadIdx.x < np && sums[threadIdx.x] != 0) {
        typedef __attribute__((address_space(1))) unsigned long long* global_u64;
        atomicAdd((unsigned long long*)reinterpret_cast<global_u64>(head_count), (unsigned long long)sums[threadIdx.x]);
    }
}

// ---------------------------------------------------------------------------
// launcher: the grid and the tile's LDS as launch_hor's streaming branch, plus the skip table, the chains and the rows
// ---------------------------------------------------------------------------
// Workgroups per CU.  A workgroup takes up to 39 KB of LDS (the table 16 KB of it), so four are resident at most — and
// with the table of 2048 u32 slots, where six were, FOUR won: swept on 1 GiB of rand128 at m = 16, 32, 256 in
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
    if (a.m < 3 || a.halo < 1 || a.halo > kHaloMax || a.halo > a.m - 1) return hipErrorInvalidValue;  // (a gram and the byte before a lane's first window end exist)
    if (a.reserved != kMultiByValue && a.reserved != kMultiLong) return hipErrorInvalidValue;
    const bool by_value = a.reserved == kMultiByValue;
    if (a.width != (by_value ? pass_width(a.m) : long_width(a.m)) || a.stride != tail_stride(a.m) || a.np < 1 || a.np > a.width) return hipErrorInvalidValue;
    const uint32_t m = a.m, H = a.halo;
    const size_t head = by_value ? kHormHead + (((size_t)a.np * a.stride + 63) & ~(size_t)63) : long_head(a.np, a.stride);
    const TileRange tr = tiles_for(a.s_begin + m - 1, a.s_end + m - 1, (uint64_t)kHorT * kHorL);
    if (tr.count == 0) return hipSuccess;
    const size_t lds = head + ((r16(H) + (size_t)kHorT * kHorL + 16 + 63) & ~(size_t)63);  // whole 64-byte blocks: tile_at() permutes inside them
    const int wgs_per_cu = g_tune[4] ? g_tune[4] : horm_wgs(m);  // smartgpu_tune(4, .) applies
    uint32_t grid = (uint32_t)num_cus * (uint32_t)wgs_per_cu;
    if (grid > tr.count) grid = tr.count;
    const uint32_t least = (uint32_t)(((uint64_t)tr.count + (1u << 17) - 1) >> 17);  // a workgroup's u32 sums: at most 2^17 tiles each
    if (grid < least) grid = least;
    hipLaunchKernelGGL((hor_multi_scan<kHorT, kHorL>), dim3(grid), dim3(kHorT), lds, stream, a, tr.first, tr.count);
    return hipGetLastError();
}

// api.cpp queues launches only once this unit is part of the program
namespace {
struct RegisterHorMulti {
    RegisterHorMulti() { g_hor_multi = &launch_hor_multi; }
} g_register_hor_multi;
}  // namespace

}  // namespace sg
