// k_hormf.hip — hor_multi_find: the POSITIONS of up to find_width(m) patterns of one length in ONE pass over a byte text
// (a translation unit of its own: dev_common.hpp says why; k_horm.hip, k_hors.hip and multi.hpp are not touched)
#include "dev_common.hpp"
#include "launch_common.hpp"
#include "multi_find.hpp"

namespace sg {

// ---------------------------------------------------------------------------
// hor_multi_scan (k_horm.hip) that lists what it counts.  The same tiles on absolute offsets indexed by window end, the
// same back halo, prefetch one tile ahead, swizzle and range clamps; the same table of multi.hpp — a byte per slot, indexed
// by a window's last two bytes: the least shift any pattern of the pass allows and a bit that says that some pattern's
// last gram falls into the slot —, the same walk (one per lane, for all patterns at once) and the same chains (a window
// whose entry has the bit is compared, whole, with every pattern of its gram's bucket).  What differs:
//  * The patterns come through the ARENA, not by value: smartgpu_find_batch64 is a synchronous call, it stages the rows of
//    all its patterns (tail_fill's bytes at tail_stride(m)) and, where a window is completed in memory (m - 1 > H), the
//    whole patterns at find_pitch(m), and a pass receives two pointers.  The prologue reads the pass's rows, 16 bytes
//    per thread and at most twice, before the first tile is asked for.
//  * An occurrence of pattern g at start s is an ENTRY, (s << kFindBatchShift) | (base + g).  Lanes walk independently, so
//    nothing wave-wide belongs in the walk: the lane takes a slot of the workgroup's STAGE in LDS with an LDS atomic.
//    Between two tiles (and after the last) the workgroup reserves what the stage holds with ONE atomicAdd on the call's
//    cursor and writes it with vector stores while slot < cap.  A lane that finds the stage full reserves one slot of
//    the output itself: frequent occurrences cost time, never correctness.  Entries beyond cap are counted and dropped.
//  * The cursor and the counts are two tallies of the same occurrences (the u32 LDS sums per pattern, added to
//    counts[base + g] at the end, exactly as the scan's): the host refuses a call in which they disagree.
// LDS: u8 gram[kGramSlots] | u32 heads[kGramBuckets] | np rows | u32 next[np] | u32 sums[np] | pad to 64 | the stage
// (kFindStageLds: u64 entries[kFindStage] | u32 taken | u32 | u64 base | pad) | text [tile0-H16, tile0+TB).
// The flush's barrier is reached by the whole workgroup: what decides it (the stage's fill) is read after a barrier and
// written again only behind the next one, and the tile loop's trip count is uniform.
// One instantiation; completion in memory is a run-time branch of it.
// ---------------------------------------------------------------------------
static_assert(kHaloMaxFind == kHaloMax, "multi_find.hpp counts the staged bytes with kernels.hpp's halo");
static_assert(kMultiTileLds == ((16u + (uint32_t)kHorT * kHorL + 16u + 63u) & ~63u), "the tile that find_fits counts");

// k_horm.hip's helpers, this unit's own copies (as k_hors.hip keeps its own): a pointer into global memory from a number
__device__ __forceinline__ const uint8_t* hormf_global(unsigned long long v)
{
    typedef const __attribute__((address_space(1))) uint8_t* global_u8;
    return (const uint8_t*)reinterpret_cast<global_u8>(v);
}

// a 64-bit value of lane `src`, wave-uniform (the halves go through uint32_t: the builtin returns int)
__device__ __forceinline__ unsigned long long hormf_lane(unsigned long long v, int src)
{
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, src), hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

// horm_wave_verify's counterpart: the parked lanes one at a time, each with its own text and pattern pointer, the 64
// lanes comparing 1 KiB per step together.  Returns 1 in the lane whose candidate verified, 0 elsewhere.  Every lane of
// the wave reaches the call.
__device__ __forceinline__ uint32_t hormf_wave_verify(bool has, const uint8_t* tptr, const uint8_t* pptr, uint32_t len)
{
    unsigned long long todo = __ballot(has);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t mine = 0;
    while (todo) {
        const int src = __builtin_ctzll(todo);  // wave-uniform
        todo &= todo - 1;
        const uint8_t* t = hormf_global(hormf_lane((unsigned long long)tptr, src));
        const uint8_t* p = hormf_global(hormf_lane((unsigned long long)pptr, src));
        bool diff = false;
        for (uint32_t off = lane * 16u; off < len; off += 1024u)
            diff |= differ16(t + off, p + off, len - off < 16 ? len - off : 16u);
        if (!__any(diff) && lane == (uint32_t)src) mine = 1;
    }
    return mine;
}

// the least of the byte at `slot` and s, in a table of bytes that has no byte atomics: compare-and-swap on its dword
__device__ __forceinline__ void hormf_byte_min(uint8_t* table, uint32_t slot, uint32_t s)
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

template <int THREADS, int L>
__global__ __launch_bounds__(THREADS) void hor_multi_find(MultiFindArgs a, uint64_t tile_first, uint32_t ntiles)
{
    constexpr int TB = THREADS * L;
    static_assert(THREADS == (int)kMultiThreads && THREADS % (int)kGramCap == 0, "a thread per pattern; the grams of THREADS / kGramCap patterns in a round");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t m = a.m, H = a.halo, H16 = round16(H), np = a.np, stride = tail_stride(m);
    const bool in_memory = m - 1 > H;  // windows are completed in HBM
    const uint32_t rlast = m - 1 - gram_first(m);  // P[m-1-k] is byte rlast - k of a row
    const uint32_t row_bytes = np * stride;        // a multiple of 16, at most 2 * THREADS * 16 (find_fits)
    const uint32_t pitch = find_pitch(m);
    uint8_t* gram = smem;
    uint32_t* heads = reinterpret_cast<uint32_t*>(smem + kGramSlots);
    uint8_t* rows = smem + kGramSlots + 4 * kGramBuckets;
    uint32_t* next = reinterpret_cast<uint32_t*>(rows + row_bytes);
    uint32_t* sums = next + np;
    uint8_t* stage_at = smem + find_head(np, stride) - kFindStageLds;
    unsigned long long* stage = reinterpret_cast<unsigned long long*>(stage_at);
    uint32_t* taken = reinterpret_cast<uint32_t*>(stage_at + 8u * kFindStage);
    unsigned long long* flush_base = reinterpret_cast<unsigned long long*>(stage_at + 8u * kFindStage + 8u);
    uint8_t* txt = smem + find_head(np, stride);  // txt[H16 + x] == T[tile0 + x]

    // the rows of the pass, 16 bytes per thread and at most twice, sent before the first tile is asked for
    const bool row_mine = threadIdx.x * 16u < row_bytes, row_mine2 = (threadIdx.x + THREADS) * 16u < row_bytes;
    uint4 row16 = {}, row16b = {};
    if (row_mine) row16 = *reinterpret_cast<const uint4*>(a.rows + threadIdx.x * 16u);
    if (row_mine2) row16b = *reinterpret_cast<const uint4*>(a.rows + (threadIdx.x + THREADS) * 16u);

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
        if (threadIdx.x < np) sums[threadIdx.x] = 0;
        if (threadIdx.x == 0) *taken = 0;
        if (row_mine) *reinterpret_cast<uint4*>(rows + threadIdx.x * 16u) = row16;
        if (row_mine2) *reinterpret_cast<uint4*>(rows + (threadIdx.x + THREADS) * 16u) = row16b;
    }
    __syncthreads();
    {
        const uint32_t shift_i = gram_first(m) + threadIdx.x % kGramCap;
        if (shift_i + 3 <= m)
            for (uint32_t g = threadIdx.x / kGramCap; g < np; g += THREADS / kGramCap) {
                const uint32_t two = tail_gram_at(rows + g * stride, m, shift_i);
                hormf_byte_min(gram, gram_slot(two & 0xFFu, two >> 8), gram_shift(m, shift_i));
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

    // an occurrence of pattern g at start s: counted, and its entry into the stage, or — the stage is full — straight
    // behind the cursor
    auto emit = [&](uint32_t g, uint64_t s) {
        atomicAdd(sums + g, 1u);
        const unsigned long long entry = ((unsigned long long)s << kFindBatchShift) | (a.base + g);
        const uint32_t at = atomicAdd(taken, 1u);
        if (at < kFindStage) {
            stage[at] = entry;
        } else {
            const unsigned long long slot = atomicAdd(a.cursor, 1ull);
            if (slot < a.cap) a.out[slot] = entry;
        }
    };
    // The stage to the output.  Called by the WHOLE workgroup behind a barrier that ends a walk, and followed by a barrier
    // before the next walk: `taken` is the same for every thread here, so the barrier inside is reached by all or by none.
    auto flush = [&]() {
        const uint32_t all = *taken;
        if (all == 0) return;
        const uint32_t held = all < kFindStage ? all : kFindStage;  // (the others went behind the cursor themselves)
        if (threadIdx.x == 0) *flush_base = atomicAdd(a.cursor, (unsigned long long)held);
        __syncthreads();
        const unsigned long long base = *flush_base;
        for (uint32_t i = threadIdx.x; i < held; i += THREADS)
            if (base + i < a.cap) a.out[base + i] = stage[i];
        if (threadIdx.x == 0) *taken = 0;  // (every thread has read it: they are past the barrier above)
    };

    for (; t < t_end; t += gridDim.x) {
        const uint64_t tile0 = t * TB;
        __syncthreads();  // previous tile fully consumed (and tables visible)
        flush();
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
        uint64_t parked_s = 0;
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
                    const uint64_t s = tile0 + (e - H16) - (m - 1);  // the window's start (>= s_begin: e >= e_begin)
                    if (in_memory && ok) {  // the rest of the window is not in LDS
                        if (!parked) {
                            parked = true;
                            parked_g = g;
                            parked_s = s;
                            ok = false;  // listed after the loop
                        } else {
                            ok = global_equal(a.text + s, a.pats + (size_t)g * pitch, m - 1 - H);
                        }
                    }
                    if (ok) emit(g, s);
                }
            }
            e += gram_byte_shift(ent);
        }
        if (in_memory && hormf_wave_verify(parked, a.text + parked_s, a.pats + (size_t)parked_g * pitch, m - 1 - H)) emit(parked_g, parked_s);
    }
    __syncthreads();
    flush();

    // the workgroup's np sums, each straight to its pattern's count
    __syncthreads();
    if (threadIdx.x < np && sums[threadIdx.x] != 0) atomicAdd(a.counts + a.base + threadIdx.x, (unsigned long long)sums[threadIdx.x]);
}

// ---------------------------------------------------------------------------
// launcher: launch_hor_multi's grid, with the stage in the LDS
// ---------------------------------------------------------------------------
static hipError_t launch_hor_multi_find(const MultiFindArgs& a, int num_cus, hipStream_t stream)
{
    if (a.m < 3 || a.halo < 1 || a.halo > kHaloMax || a.halo != (a.m - 1 < kHaloMax ? a.m - 1 : kHaloMax)) return hipErrorInvalidValue;  // (a gram and the byte before a lane's first window end exist)
    if (a.np < 1 || a.np > find_width(a.m) || (uint64_t)a.base + a.np > kFindBatchMaxK) return hipErrorInvalidValue;
    if (a.s_end + a.m - 1 >= kFindBatchMaxEnd ||(a.cap != 0 && !a.out) || !a.rows || !a.counts || !a.cursor) return hipErrorInvalidValue;
    if (find_in_memory(a.m) && !a.pats) return hipErrorInvalidValue;
    const TileRange tr = tiles_for(a.s_begin + a.m - 1, a.s_end + a.m - 1, (uint64_t)kHorT * kHorL);
    if (tr.count == 0) return hipSuccess;
    const size_t lds = find_head(a.np, tail_stride(a.m)) + ((r16(a.halo) + (size_t)kHorT * kHorL + 16 + 63) & ~(size_t)63);  // whole 64-byte blocks: tile_at() permutes inside them
    ScanArgs one = {};
    one.m = a.m;
    one.sparse = 1;
    const int wgs_per_cu = g_tune[4] ? g_tune[4] : tile_wgs(one);  // the scan's value; smartgpu_tune(4, .) applies
    uint32_t grid = (uint32_t)num_cus * (uint32_t)wgs_per_cu;
    if (grid > tr.count) grid = tr.count;
    const uint32_t least = (uint32_t)(((uint64_t)tr.count + (1u << 17) - 1) >> 17);  // a workgroup's u32 sums: at most 2^17 tiles each
    if (grid < least) grid = least;
    hipLaunchKernelGGL((hor_multi_find<kHorT, kHorL>), dim3(grid), dim3(kHorT), lds, stream, a, tr.first, tr.count);
    return hipGetLastError();
}

// api.cpp answers smartgpu_find_batch64 only once this unit is part of the program
namespace {
struct RegisterHorMultiFind {
    RegisterHorMultiFind() { g_hor_multi_find = &launch_hor_multi_find; }
} g_register_hor_multi_find;
}  // namespace

}  // namespace sg
