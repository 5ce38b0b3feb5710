// launch.hip — the dispatcher between the C-ABI layer (api.cpp) and the kernel families (k_*.hip): which launcher a plan's
// words lead to is decided ONCE, in route() (route.hpp) — launch_scan launches it, scan_kernel_name names it, group_key groups
// the patterns of a set in one grid by it (tests/test_dispatch.py holds them together); the tuning knobs.  No kernel here.
//
// Every kernel computes the same function
//     count(P,T) = |{ s in [s_begin, s_end) : T[s..s+m) == P }|
// (overlapping occurrences count) and differs in the per-lane scan strategy and in the tables it stages in LDS.
// Three families, each family's kernels in translation units of their own (dev_common.hpp says why):
//
//  1. LDS TILES — the skip algorithms HOR, BM, BNDM (k_hor.hip, k_bm.hip, k_bndm.hip, k_bndmx.hip).
//     The text is cut into tiles of TB = THREADS*L bytes on ABSOLUTE text offsets, so
//     every tile load is 16-byte aligned and coalesced (global_load_dwordx4 nt, 1 KiB
//     per wave-load); tile t+1 is prefetched into registers while the lanes walk tile
//     t.  Tiles are indexed by window END position e = s+m-1 with a BACK halo of
//     H = min(m-1, 16) bytes: the byte that drives the shift, T[e], is always in the
//     tile; a lane verifies right-to-left through the halo by itself and — only for
//     m-1 > H and only after H+1 bytes matched — parks the window for a
//     wave-cooperative comparison of the rest (wave_verify).
//  2. RUNS THROUGH LDS SLABS — the serial automata SO and KMP (k_so.hip, k_kmp.hip).
//     A lane owns a run of 2-4 KiB of start positions (128+ bytes on small texts); the wave
//     fetches the next 128-byte line of each of its 64 runs with coalesced non-temporal loads,
//     parks it in its own LDS slab one 64-byte half at a time and every lane reads its run
//     back.  No workgroup barrier after the table set-up.
//  3. PACKED — EPSM, and the short-pattern / tiny-shift regime of the skip algorithms
//     (k_packed.hip): every alignment is compared from registers, no LDS.
//
// Restarting an algorithm at a lane / tile / run / GPU boundary preserves the count
// (SURVEY.md §7 restart table): skip algorithms carry no state between windows, the
// automata restart in their initial state and re-scan w-1 bytes.  Per-lane hit
// counters are summed across the 64-lane wave and the workgroup; one 64-bit atomic per workgroup.
// A pattern set over a small text runs as ONE grid, gridDim.y = pattern (launch_scan_set).
// Earlier designs of the serial kernels (so_scan, kmp_scan, so_runs64, so_runs1, kmp_links_runs,
// kmp_runs1) live in kernels_ab.inc / k_ab.hip and only in the A/B build (make AB=1, smartgpu_tune).
#include "launch_common.hpp"
#include "route.hpp"

#include "../../include/smartgpu.h"

namespace sg {

thread_local BatchCtx g_batch = {nullptr, 1};

int g_tune[8] = {0, 0, 0, 0, 0, 0, 0, 0};

// Which smartgpu_tune settings this build can honour: the kernels behind the others are only in the A/B build.
bool tune_supported(int key, int value)
{
#ifdef SMARTGPU_AB
    (void)key; (void)value;
    return true;
#else
    switch (key) {
        case 0: return value == 0 || value == 1 || value == 3;  // 2: Horspool on the bank-private tiles
        case 3: return value == 0 || value == 5;                 // superseded KMP kernels (5: kmp_runs without its four-byte table; 6: round 3's one-workgroup form)
        case 6: return value == 0 || value == 5;                 // superseded SO kernels (5: so_runs without the four-symbol table)
        case 7: return value == 0 || (value >= 5 && value <= 9);   // packed load policies (9: EPSM without its packed-symbol modes; 8: m <= 4 without v_mqsad)
        default: return true;
    }
#endif
}

// skip algorithms use the packed matcher up to this m (crossovers measured on 1 GiB rand128
// with non-temporal tile loads, profiles/r01): HOR/TUNEDBM/RAITA 7, BM 8, BNDM 11, QS 14, HASH3/5/8 32/64/28
static constexpr uint32_t packed_max_m(int algo)
{
    return (algo == SMARTGPU_HOR || algo == SMARTGPU_TUNEDBM || algo == SMARTGPU_RAITA) ? 7u
         : algo == SMARTGPU_BM ? 7u : algo == SMARTGPU_BNDM ? 10u  // re-measured with five workgroups per CU below 16 bytes (session u)
         : algo == SMARTGPU_QS ? 14u     // three LDS reads per window (text byte, next byte, table): later crossover
         : algo == SMARTGPU_HASH3 ? 24u  // q text reads + hash + table per window, shifts of at most m-q+1: the
         : algo == SMARTGPU_HASH5 ? 32u  //   tiles pass the packed matcher's 78-81 % only here (with four workgroups
         : algo == SMARTGPU_HASH8 ? 80u  //   per CU; HASH8 own/packed: m=32 63/79, 64: 78/81, 96: 82/81 — session u)
         : 0u;
}

uint32_t short_pattern_max_m(int algo)
{
    if (algo == SMARTGPU_SBNDM || algo == SMARTGPU_BNDML) return packed_max_m(SMARTGPU_BNDM);  // they share bndm_scan's crossover
    if (algo == SMARTGPU_KR) return 15;  // below 16 bytes only the low m bits of the rolled hash can be compared (launch_scan)
    return packed_max_m(algo);
}

// Regimes of the skip algorithms (HOR, BM, BNDM).  For short patterns the window is a
// few dwords and a skip loop degenerates (a lane advances ~m bytes per two dependent
// LDS reads); the packed matcher tests every alignment at HBM speed instead — the
// "hybrid" SURVEY.md §7 describes; counts are identical.  Measured on 1 GiB rand128
// (profiles/r01): HOR m=4: flat tile 45 %, bank-private 55 %, packed 74 % of 8 TB/s.
// Thresholds per algorithm: packed_max_m().
static int hor_regime(uint32_t m, int algo = SMARTGPU_HOR)
{
    const int v = g_tune[0];  // 0 auto, 1 flat, 2 bank-private, 3 packed
    if (v == 3) return 3;
    if (v == 2) return m <= kHaloMax + 1 ? 2 : 1;  // the bank-private kernel keeps whole windows in LDS
    if (v == 1) return 1;
    return m <= packed_max_m(algo) ? 3 : 1;  // bank-private kernel: only on request
}

// The one decision tree: launch_scan launches what it returns, scan_kernel_name names it, group_key groups by it.
Route route(int algo, uint32_t m, const PlanWords& w, TextCodes codes)
{
    // A pattern over two or three symbols, 16 bytes or longer: no byte, pair or dword of it tells a
    // window from its neighbours, so the skip kernels move one or two bytes at a time and the packed
    // matcher tests all four fingerprint dwords at every alignment (33-45 % on rand2, all of them).
    // The branch-free bit-parallel runs kernel does not care what the bytes are (66-70 %): plans of
    // such patterns carry Shift-Or masks as well (api.cpp build_blob) and count with it.
    if (w.so_off != 0 && algo != SMARTGPU_SO && algo != SMARTGPU_SA && g_tune[0] == 0) return {Launcher::so_runs, 0};
    const bool pk = w.prefer_packed && g_tune[0] == 0;
    // a TEXT of at most four byte values: Horspool and Boyer-Moore on its grams (k_horg.hip, k_bmg.hip) — eight one-bit symbols from
    // 16 bytes on (two values), four two-bit symbols from 8; a window shorter than two grams cannot be shifted by more than its own
    // rule allows (m - Q + 1).  tune(2, 4): never (A/B).  Any other text: Horspool's q-gram (hash) table, or the byte tables.
    const int gram = g_tune[2] == 4 ? 0 : ((codes.one & 0xFFu) != 0xFFu && m >= 16) ? 1 : (codes.shift < 7 && m >= 8) ? 2 : 0;
    switch (algo) {
        case SMARTGPU_TUNEDBM:  // hor_scan<.., 0> is Tuned BM's loop (see the kernel's comment; tunedbm.c:38-62 is Horspool's
        case SMARTGPU_HOR: {    // shift behind an unrolled skip loop: on grams the same kernel)
            const int regime = pk ? 3 : hor_regime(m);
            if (regime == 3) return {Launcher::packed, SMARTGPU_HOR};
#ifdef SMARTGPU_AB
            if (regime == 2) return {Launcher::hor_bp, 0};
#endif
            if (gram) return {Launcher::hor_gram, gram};
            return {Launcher::hor, (int)hor_q(w)};  // q: the plan's q-gram table (api.cpp), 0: the byte table
        }
        case SMARTGPU_KR:
            // Short patterns, like the skip algorithms': the packed matcher (72-77 %).  Only the low m bits
            // of the rolled hash can be compared, so one window end in 2^m is confirmed (m = 8: 32 %,
            // m = 12: 50 % of 8 TB/s), and below 8 the rolling form needs the outgoing byte (15 %).
            if (m < 16 && g_tune[0] != 1) return {Launcher::packed, SMARTGPU_HOR};
            return {Launcher::kr, 0};
        case SMARTGPU_HASH3:
        case SMARTGPU_HASH5:
        case SMARTGPU_HASH8:
        case SMARTGPU_RAITA:
        case SMARTGPU_QS:  // the Horspool family on hor_scan's tiles; short patterns: packed regime as HOR
            if (pk || hor_regime(m, algo) == 3) return {Launcher::packed, SMARTGPU_HOR};
            return {Launcher::hor_var, algo};
        case SMARTGPU_BM:
            // m = 1 always: bm_scan reads the byte before the window's last along with it, and a one-byte
            // window has none (at a tile's first byte that read would leave the tile region)
            if (m == 1 || (m <= packed_max_m(SMARTGPU_BM) && g_tune[0] != 1) || pk) return {Launcher::packed, SMARTGPU_BM};
            if (gram) return {Launcher::bm_gram, gram};
            return {Launcher::bm, 0};
        case SMARTGPU_BNDML:
            if (m > 32) return pk ? Route{Launcher::packed, SMARTGPU_BNDM} : Route{Launcher::bndml, 0};  // multi-word vectors
            [[fallthrough]];  // m <= 32 is plain BNDM (bndml.c:44-75)
        case SMARTGPU_SBNDM:
        case SMARTGPU_BNDM:
            if (algo != SMARTGPU_SBNDM && (w.halo & kBndmGramWindow) && !pk) return {Launcher::bndm, 0};  // a one-gram window (api.cpp): bndm_scan at any length
            if ((m <= packed_max_m(SMARTGPU_BNDM) && g_tune[0] != 1) || pk) return {Launcher::packed, SMARTGPU_BNDM};
            return {algo == SMARTGPU_SBNDM ? Launcher::sbndm : Launcher::bndm, 0};
        case SMARTGPU_SA:  // Shift-And counts in the complemented, Shift-Or form (api.cpp build_blob); its own AND form
        case SMARTGPU_SO:  // (so_runs1<.., AND = true>, masks after the Shift-Or ones) is in the A/B build: tune(6,3)
            return {Launcher::so_runs, 0};
        case SMARTGPU_KMP: return {Launcher::kmp_runs, 0};  // per-lane runs streamed through LDS
    }
    return {Launcher::packed, SMARTGPU_EPSM};  // EPSM is the packed matcher
}

// The Route (so a regime that route() learns to tell apart never shares a grid) below the words themselves: sparse (tile_wgs),
// KMP's window, BNDM's q and gram mark, Horspool's q — and the packed and reroute flags as they stand, whatever g_tune makes of
// them, so that a set falls into the same groups under every setting (a mixed set ran every BNDM pattern with the
// first pattern's q, because the key of that time did not know that halo carries it).
uint64_t group_key(int algo, uint32_t m, const PlanWords& w, TextCodes codes)
{
    const Route r = route(algo, m, w, codes);
    const uint64_t pp = algo == SMARTGPU_KMP ? w.prefer_packed : (w.prefer_packed ? 1u : 0u);
    const uint64_t variant = (algo == SMARTGPU_BNDM || algo == SMARTGPU_BNDML) ? bndm_q_and_mark(w) : algo == SMARTGPU_HOR ? hor_q(w) : 0u;
    return (pp << 40) | (variant << 28) | (w.so_off ? 1ull << 21 : 0) | (w.sparse ? 1ull << 20 : 0) | ((uint64_t)r.to << 12) | (uint64_t)(r.arg & 0xFFF);
}

const char* scan_kernel_name(int algo, uint32_t m, bool prefer_packed, bool so_masks, uint32_t halo)
{
    if (algo < 0 || algo >= SMARTGPU_NUM_ALGOS) return "?";
    switch (route(algo, m, PlanWords{halo, prefer_packed, 0, so_masks}, TextCodes()).to) {  // (the gram launchers: their base kernel's name)
        case Launcher::so_runs:
#ifdef SMARTGPU_AB
            if (algo == SMARTGPU_SO) return g_tune[6] == 1 ? "so_scan" : g_tune[6] == 2 ? "so_runs64" : g_tune[6] == 4 ? "so_runs1" : "so_runs";
            if (algo == SMARTGPU_SA) return (g_tune[6] == 3 || g_tune[6] == 4) ? "so_runs1" : "so_runs";
            return g_tune[6] == 4 ? "so_runs1" : "so_runs";  // the rerouted patterns
#endif
            return "so_runs";
        case Launcher::kmp_runs:
#ifdef SMARTGPU_AB
            return (g_tune[3] == 1 && m <= 40) ? "kmp_scan" : g_tune[3] == 2 ? "kmp_links_runs" : g_tune[3] == 3 ? "kmp_runs1" : "kmp_runs";
#endif
            return "kmp_runs";
        case Launcher::packed: return "packed_scan";
        case Launcher::hor: case Launcher::hor_var: case Launcher::hor_gram: return "hor_scan";
        case Launcher::hor_bp: case Launcher::kr: return "hor_scan_bp";
        case Launcher::bm: case Launcher::bm_gram: return "bm_scan";
        case Launcher::bndm: return "bndm_scan";
        case Launcher::sbndm: return "sbndm_scan";
        case Launcher::bndml: return "bndml_scan";
    }
    return "?";
}

// What launch_scan fills in for the kernels before they run: where the packed matcher finds the fingerprint
// in this algorithm's blob, and the Shift-Or masks of SO / SA.  Applied to the by-value arguments of a single
// launch and, by the caller, to every element of a pattern set's argument array (launch_scan_set).
ScanArgs prepare_scan_args(int algo, ScanArgs a)
{
    const uint32_t m = a.m;
    switch (algo) {
        case SMARTGPU_KR: a.fp_off = kTableOff + 4; break;  // after the pattern's hash
        case SMARTGPU_BM: a.fp_off = kTableOff + ((1536 + 2 * (m + 1) + 3) & ~3u); break;  // after first, second, bc, gs, safe shift
        case SMARTGPU_BNDML:  // after the masks (W = 2) and the period / after B[256]
            a.fp_off = m > 32 ? kTableOff + 1024 * 2 + 4 : kTableOff + 1024;
            a.halo &= 0xFFu;
            break;
        case SMARTGPU_SBNDM:
        case SMARTGPU_BNDM:  // after B[256]; halo = bndm_scan's q, the plan's marks above it
            a.fp_off = kTableOff + 1024;
            a.halo &= 0xFFu;
            break;
        case SMARTGPU_EPSM: a.fp_off = kTableOff; break;
        case SMARTGPU_SO: a.so_off = kTableOff; break;
        case SMARTGPU_SA: a.so_off = g_tune[6] == 3 ? kTableOff + 1024 : kTableOff; break;
        case SMARTGPU_KMP: break;
        default:  // the Horspool family: the fingerprint after the u16 and u8 tables; halo = H (at most 32), Horspool's q above it
            a.fp_off = kTableOff + 768;
            a.halo &= 0xFFu;
            break;
    }
    return a;
}

hipError_t launch_scan(int algo, const ScanArgs& a_in, int num_cus, hipStream_t stream, TextCodes codes)
{
    if (a_in.s_end <= a_in.s_begin) return hipSuccess;
    if (algo < 0 || algo >= SMARTGPU_NUM_ALGOS) return hipErrorInvalidValue;
    const ScanArgs a = prepare_scan_args(algo, a_in);  // a.fp_off, a.so_off of SO / SA; a.halo without the plan's marks
    const Route r = route(algo, a.m, PlanWords{a_in.halo, a_in.prefer_packed, a_in.sparse, a_in.so_off}, codes);
    switch (r.to) {
        case Launcher::so_runs: {
#ifdef SMARTGPU_AB
            const bool own = algo == SMARTGPU_SO || algo == SMARTGPU_SA;  // else: a rerouted pattern, on so_runs1 too with tune(6,4)
            if (own || g_tune[6] == 4) {
                bool handled = false;
                const hipError_t e = launch_ab_so(own ? algo : SMARTGPU_HOR, a, num_cus, stream, &handled);
                if (handled) return e;
            }
#endif
            return launch_so_runs(a, false, num_cus, stream, codes);
        }
        case Launcher::kmp_runs: {
#ifdef SMARTGPU_AB
            bool handled = false;
            const hipError_t e = launch_ab_kmp(a, num_cus, stream, &handled);
            if (handled) return e;
#endif
            return launch_kmp_runs(a, num_cus, stream, codes);
        }
        case Launcher::packed: return launch_packed(r.arg, a, num_cus, stream, r.arg == SMARTGPU_EPSM ? codes : TextCodes());  // only EPSM's modes look at the text
        case Launcher::hor: return launch_hor(a, (uint32_t)r.arg, num_cus, stream);
        case Launcher::hor_var: return launch_hor_var(r.arg, a, num_cus, stream);
        case Launcher::hor_gram: return launch_hor_gram(a, r.arg, num_cus, stream);
        case Launcher::kr: return launch_kr(a, num_cus, stream);
        case Launcher::bm: return launch_bm(a, num_cus, stream);
        case Launcher::bm_gram: return launch_bm_gram(a, r.arg, num_cus, stream);
        case Launcher::bndm: return launch_bndm(a, num_cus, stream, codes);
        case Launcher::sbndm: return launch_sbndm(a, num_cus, stream);
        case Launcher::bndml: return launch_bndml(a, num_cus, stream);
#ifdef SMARTGPU_AB
        case Launcher::hor_bp: return launch_hor_bp(a, num_cus, stream);
#else
        case Launcher::hor_bp: break;  // Horspool on the bank-private tiles: only in the A/B build
#endif
    }
    return hipErrorInvalidValue;
}

hipError_t launch_scan_set(int algo, const ScanArgs& first, const BatchItem* device_items, uint32_t count, int num_cus,
                           hipStream_t stream, TextCodes codes)
{
    if (count == 0) return hipSuccess;
    g_batch = {device_items, count};
    const hipError_t e = launch_scan(algo, first, num_cus, stream, codes);
    g_batch = {nullptr, 1};
    return e;
}

}  // namespace sg
