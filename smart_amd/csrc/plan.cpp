// plan.cpp — the plan builder (plan.hpp).  build_blob takes the pattern's statistics once (pattern_stats), lays out the
// tables of the algorithm (one layout_* function per table layout, not per algorithm id) and decides whether the plan
// also carries Shift-Or masks and is counted by so_runs (so_reroute).  Compiled as host code only, like tables.cpp; twice,
// because the KMP layout differs in the A/B build.
#include "plan.hpp"

#include <algorithm>
#include <cstring>

#include "tables.hpp"

namespace sg {

const char* const kAlgoNames[SMARTGPU_NUM_ALGOS] = {"hor", "bm", "kmp", "so", "bndm", "epsm", "sa", "qs", "tunedbm", "raita",
                                                    "hash3", "hash5", "hash8", "sbndm", "kr", "bndml"};

uint32_t min_pattern(int algo)
{
    return (algo == SMARTGPU_RAITA || algo == SMARTGPU_SBNDM) ? 2u : algo == SMARTGPU_HASH3 ? 3u : algo == SMARTGPU_HASH5 ? 5u : algo == SMARTGPU_HASH8 ? 8u : 1u;
}

namespace {

using Blob = std::vector<uint8_t>;

void append(Blob& blob, const void* p, size_t bytes)
{
    const uint8_t* b = static_cast<const uint8_t*>(p);
    blob.insert(blob.end(), b, b + bytes);
}

void align_up(Blob& blob, size_t to) { blob.resize((blob.size() + to - 1) & ~(to - 1), 0); }

// first min(m,16) pattern bytes as 4 dwords + 4 byte masks (packed kernel)
void append_fingerprint(Blob& blob, const uint8_t* P, uint32_t m)
{
    uint32_t fp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint8_t* fb = reinterpret_cast<uint8_t*>(fp);
    const uint32_t F = std::min<uint32_t>(m, 16);
    for (uint32_t i = 0; i < F; ++i) {
        fb[i] = P[i];
        fb[16 + i] = 0xFF;
    }
    append(blob, fp, sizeof fp);
}

// ---- the pattern's statistics ------------------------------------------------------------------------------------------
struct PatternStats {
    uint32_t cnt[256] = {0};     // how often each symbol occurs in P
    uint32_t distinct = 0;       // symbols that occur in P
    uint64_t pairs = 0;          // ordered pairs of equal symbols in P: pairs / (m (m-1)) estimates P(two symbols are equal)
    bool repeats = false;
    bool repeats_short = false;  // 7 bytes or fewer with a symbol that occurs twice (a small alphabet, most likely)
};

// How often two text symbols are equal, if the text's symbols are distributed like the pattern's
// own (unbiased from its histogram: sum c(c-1) / m(m-1)).  Above 1/48 — binary and DNA-like
// alphabets, natural language (~1/15), rand32 — a skip loop meets a candidate every few windows,
// its lanes verify and diverge (English, m >= 64: BM 31-44 %, BNDM 31-36 %, HOR 63-69 %; rand32:
// 67-75 %), and the packed matcher, which does the same work whatever the bytes are, is the better
// regime (64-81 % on all of them).  Below it (rand64 and up) windows die on their first comparison
// and the skip kernels only stream (80-86 % on rand128 against 76-81 %).  Measured: DESIGN.md §8.
// The count does not depend on the choice.
PatternStats pattern_stats(const uint8_t* P, uint32_t m)
{
    PatternStats st;
    for (uint32_t i = 0; i < m; ++i) st.distinct += st.cnt[P[i]]++ == 0;
    for (uint32_t c = 0; c < 256; ++c) st.pairs += static_cast<uint64_t>(st.cnt[c]) * (st.cnt[c] > 0 ? st.cnt[c] - 1 : 0);
    // m < 32: too few symbols for the estimate; two equal pairs are taken as a sign (rand32, m = 16:
    // skip kernels 58-65 %, packed 76 %; on rand128 one pattern in four then goes packed, 76 % for 83 %)
    st.repeats = m > 7 && (st.pairs * 48 > static_cast<uint64_t>(m) * (m - 1) || (m < 32 && st.pairs >= 4));
    st.repeats_short = m <= 7 && st.pairs >= 2;
    return st;
}

// ---- table layouts -----------------------------------------------------------------------------------------------------
// What a layout chose that the reroute rule reads (by name, not through the plan's halo).
struct Chosen {
    uint32_t hor_q = 0;          // HOR: the q of its q-gram bad-character table (patterns over two to four symbols), 0: the byte table
    uint32_t bndm_q = 0;         // BNDM (and BNDML's m <= 32): bndm_scan's q, the plan's halo
    uint32_t bndm_q_wanted = 1;  // BNDM: the q its statistics ask for (the plan's q also has to divide the window)
};

// HASHq's u16 table (zero entry = flag | shift after a candidate); Horspool's q-gram table is the same
void qgram_table(const uint8_t* P, uint32_t m, uint32_t q, uint16_t tab[256])
{
    int32_t after = 1;
    const std::vector<int32_t> sh = qgram_hash_shifts(P, m, q, &after);
    for (int c = 0; c < 256; ++c)
        tab[c] = sh[c] == 0 ? static_cast<uint16_t>(0x8000u | after) : static_cast<uint16_t>(sh[c]);
}

// HOR's layout, which HASH3/5/8 and QS share: u16 table, 256 bytes (Horspool: plain u8 shifts; the others: spare), fingerprint
void layout_shift_table(Blob& blob, const uint16_t tab[256], const uint8_t* tab8, const uint8_t* P, uint32_t m)
{
    append(blob, tab, 512);
    const uint8_t spare[256] = {0};
    append(blob, tab8 ? tab8 : spare, 256);
    append_fingerprint(blob, P, m);  // packed regime
}

// HOR, TUNEDBM (tunedbm.c:38-40: the same table with a zero for P[m-1] — the flag bit below), RAITA (raita.c:43: the same
// table).  Returns the q of Horspool's q-gram table, 0: the byte table.
uint32_t layout_horspool(Blob& blob, int algo, const uint8_t* P, uint32_t m, const PatternStats& st)
{
    const std::vector<int32_t> bc = bad_char(P, m);
    uint16_t tab[256];
    for (int c = 0; c < 256; ++c)
        tab[c] = static_cast<uint16_t>(bc[c]) | (c == P[m - 1] ? 0x8000u : 0u);
    // Horspool over a pattern of two to four symbols (binary texts, DNA): the last BYTE says next to nothing — the
    // shift is the distance to its previous occurrence, a byte or two (hor_scan on rand2: 16 % of 8 TB/s at any m).
    // The bad-character rule on the window's last q BYTES instead (Horspool on the super-alphabet of q-grams, the
    // table indexed by their 8-bit hash sum T[e-k] 2^k — on a 0/1 text the q-gram itself — as Lecroq's hash3/5/8.c
    // do it): the shift is back at m - q + 1 for a gram that does not occur in P.  q = 8 for two symbols, 5 or 8 for
    // three and four; the kernel is hor_scan's HASHq instantiation, the table has Horspool's layout (zero entry =
    // flag | shift after a candidate).  Measured on 1 GiB, own kernel: rand2 m = 32 / 64 / 256+: 54 / 68 / 70 %
    // (byte table: 16 %), rand4 m = 16 / 32 / 64+: 60 / 73 / 74 % (45-50 %).  q travels in bits 8.. of the plan's halo.
    uint32_t q = 0;
    if (algo == SMARTGPU_HOR && st.distinct >= 2 && st.distinct <= 4 && m >= 16) {
        q = st.distinct <= 2 ? 8u : m < 48 ? 5u : 8u;
        qgram_table(P, m, q, tab);
    }
    uint8_t tab8[256];  // plain u8 shifts for the bank-private kernel (m <= 255)
    for (int c = 0; c < 256; ++c) tab8[c] = static_cast<uint8_t>(bc[c] > 255 ? 255 : bc[c]);
    layout_shift_table(blob, tab, tab8, P, m);
    return q;
}

// BM: u16 first[256], second[256], bc[256], gs[m], safe shift; fingerprint (4-byte aligned).  halo: the plan's back halo.
void layout_bm(Blob& blob, const uint8_t* P, uint32_t m, uint32_t halo)
{
    const std::vector<int32_t> bc = bad_char(P, m);
    const std::vector<int32_t> gs = good_suffix(P, m);
    std::vector<uint16_t> tab(768 + m + 1);
    for (int c = 0; c < 256; ++c) {
        // shift after a mismatch on the window's last byte (bm.c:89 with i = m-1), or the
        // "last byte matches" flag
        tab[c] = c == P[m - 1] ? 0x8000u : static_cast<uint16_t>(std::max(gs[m - 1], bc[c]));
        // the same for the byte before it (bm.c:89 with i = m-2: max(bmGs[m-2], bmBc[c] - 1)):
        // most windows that survive their last byte die here, and the kernel has this byte
        // in hand already.  m = 1 has no such byte: all flags, the walk finds nothing to do.
        tab[256 + c] = (m < 2 || c == P[m - 2]) ? 0x8000u
                                                : static_cast<uint16_t>(std::max(gs[m - 2], bc[c] - 1));
        tab[512 + c] = static_cast<uint16_t>(bc[c]);
    }
    for (uint32_t i = 0; i < m; ++i) tab[768 + i] = static_cast<uint16_t>(gs[i]);
    // gs[m]: a shift that is safe for a window whose last H+1 bytes matched, whatever
    // the remaining comparison says: min of gs over the unchecked positions (and gs[0],
    // the shift after a full match).  Used when the kernel parks the window.
    int32_t safe = gs[0];
    if (m - 1 > halo)
        for (uint32_t i = 0; i + 1 < m - halo; ++i) safe = std::min(safe, gs[i]);
    tab[768 + m] = static_cast<uint16_t>(safe);
    append(blob, tab.data(), tab.size() * 2);
    align_up(blob, 4);
    append_fingerprint(blob, P, m);  // packed regime
}

// KMP: i16 next[m+1], the compact table, the spread table where the plan carries one (kernels.hpp kmp_compact_off,
// kmp_spread_off).  Returns the window of the four-bytes-per-step table, which travels as the plan's prefer_packed; 0: none.
uint32_t layout_kmp(Blob& blob, const uint8_t* P, uint32_t m)
{
    const std::vector<int32_t> nx = kmp_next(P, m);
    std::vector<int16_t> tab(m + 1);
    for (uint32_t i = 0; i <= m; ++i) tab[i] = static_cast<int16_t>(nx[i]);
    append(blob, tab.data(), tab.size() * 2);
    align_up(blob, 16);  // the transition table is 16-byte aligned
    // kmp_runs<., false, COMPACT> (round 4; every text that is not a four-symbol text): the automaton over
    // kmp_compact_window(m) bytes — the pattern, or its 56-byte prefix — with an ABSORBING accept row Z (every transition
    // into the accept state w leads to Z, Z leads to Z; row id(w) holds the real delta(w, .)) and the table of the
    // four-bytes-at-a-time forms (tables.cpp), stored as the kernel keeps it: row s at s * 256.
    kmp_runs_tables(P, kmp_compact_window(m), blob, true);
    // A pattern over at most four symbols (DNA-like alphabets): on a text that itself holds at most four byte values
    // kmp_runs takes FOUR text bytes per table step (kmp_runs<., FOUR>; that table lives in the gaps of the SPREAD
    // byte table, whose ids are 4s up to 62 states, and is derived from it on the device) — the window is then the
    // pattern or its 62-byte prefix; its length travels as the plan's prefer_packed field (0: no such table).  Which
    // of the two kernels runs is decided at launch, from the TEXT (TextCodes): each finds its own table.
    const uint32_t w4 = std::min<uint32_t>(m, kKmpPrefix);
    uint32_t distinct4 = 0;
    {
        bool have[256] = {false};
        for (uint32_t i = 0; i < w4; ++i)
            if (!have[P[i]]) { have[P[i]] = true; ++distinct4; }
    }
    const bool has4 = m >= 2 && distinct4 <= 4;
#ifdef SMARTGPU_AB
    kmp_runs_tables(P, has4 ? w4 : kmp_window(m), blob);  // the A/B build: always (tune(3,6): round 3's one-workgroup form)
    {   // kmp_runs1 (A/B build): the automaton of P[0..w), w = min(m, 255); state s is row id(s) = rotl8(s, 2),
        // the accept state row 255 — or row 4w while the ids 4s do not wrap (w < 64) —, the largest id (its
        // running maximum needs that); row r XOR-swizzled by r
        const uint32_t w = std::min<uint32_t>(m, kKmpDfaMaxM);
        const std::vector<uint8_t> dfa = kmp_dfa(P, w);
        const uint32_t acc = w < 64 ? 4 * w : 255u;
        auto id = [w, acc](uint32_t st) { return st == w ? acc : ((st << 2) | (st >> 6)) & 255u; };
        std::vector<uint8_t> sw(256 * 256, 0);
        for (uint32_t st = 0; st <= w; ++st) {
            const uint32_t r = id(st);
            for (uint32_t c = 0; c < 256; ++c) sw[r * 256 + (c ^ r)] = static_cast<uint8_t>(id(dfa[st * 256 + c]));
        }
        append(blob, sw.data(), sw.size());
    }
#else
    if (has4) kmp_runs_tables(P, w4, blob);
#endif
    return has4 ? w4 : 0;
}

// BNDML from 33 bytes on (bndml.c:91-93): bit i of word i/32 of B[c] <=> P[w-1-i] == c, over w = min(m, kBndmlWindow) bytes;
// the period of P[0..w); fingerprint
void layout_bndml(Blob& blob, const uint8_t* P, uint32_t m)
{
    const uint32_t w = std::min<uint32_t>(m, kBndmlWindow);
    const uint32_t W = w <= 64 ? 2 : w <= 128 ? 4 : 8;
    std::vector<uint32_t> B(256 * W, 0u);
    for (uint32_t i = 0; i < w; ++i) B[P[w - 1 - i] * W + i / 32] |= 1u << (i % 32);
    append(blob, B.data(), B.size() * 4);
    const std::vector<int32_t> nx = kmp_next(P, w);  // nx[w] = longest proper border of P[0..w)
    const uint32_t period = w - static_cast<uint32_t>(nx[w]);
    append(blob, &period, 4);
    append_fingerprint(blob, P, m);  // packed regime (at kTableOff + 1024*W + 4)
}

// BNDM, SBNDM and BNDML up to 32 bytes (plain BNDM, bndml.c:44-75): u32 B[256], fingerprint; SBNDM: the period behind them
void layout_bndm(Blob& blob, int algo, const uint8_t* P, uint32_t m)
{
    const std::vector<uint32_t> B = bndm_masks(P, m);
    append(blob, B.data(), 1024);
    append_fingerprint(blob, P, m);  // packed regime
    if (algo == SMARTGPU_SBNDM) {  // sbndm.c:44-55: the shift after an occurrence = period of P[0..w)
        const uint32_t w = std::min<uint32_t>(m, 32);
        const std::vector<int32_t> nx = kmp_next(P, w);  // nx[w] = longest proper border of the prefix
        const uint32_t period = w - static_cast<uint32_t>(nx[w]);
        append(blob, &period, 4);
    }
}

// bndm_scan reads q bytes of a window per iteration: the smallest q of 1, 2, 4, 8 (at most half the
// window, and a divisor of it) for which a window rarely outlives its first iteration — the chance that the q-gram at its
// end occurs in P[0..w), (w-q+1) * p^q with p = P(two symbols are equal) estimated from the pattern
// itself, is below 0.3.  rand128: 1; English: 2; four symbols: 4; two: 8.  Travels as the plan's halo
// (bndm_scan's lane tiles always hold the 32 bytes before a segment).
void choose_bndm_q(uint32_t m, const PatternStats& st, Chosen& ch)
{
    const uint32_t w = std::min<uint32_t>(m, 32);
    double p = m > 1 ? std::max(static_cast<double>(st.pairs) / (static_cast<double>(m) * (m - 1)), 1.0 / 256) : 1.0;
    // (few symbols for the estimate: a pattern in which at most half of the symbols are distinct comes from
    // an alphabet of about that many — rand4, m = 8: the pair count says 0.05 .. 0.4, four symbols say 0.25)
    if (st.distinct * 2 <= m) p = std::max(p, 1.0 / st.distinct);
    uint32_t q = 1;
    while (q < 8 && 2 * q <= std::max(w / 2, 1u)) {
        double survive = static_cast<double>(w - q + 1);
        for (uint32_t i = 0; i < q; ++i) survive *= p;
        if (survive < 0.3) break;
        q *= 2;
    }
    ch.bndm_q_wanted = q;
    while (w % q) q /= 2;  // q | w: a window is read through in whole iterations
    ch.bndm_q = q;
}

// KR (kr.c:38-41): the pattern's hash; weights 2^(m-1-i) mod 2^32 vanish beyond 32 bytes
void layout_kr(Blob& blob, const uint8_t* P, uint32_t m)
{
    uint32_t hp = 0;
    for (uint32_t i = 0; i < m; ++i) hp = (hp << 1) + P[i];
    append(blob, &hp, 4);
    append_fingerprint(blob, P, m);  // packed regime (m < 16), at kTableOff + 4
}

// ---- the reroute to so_runs --------------------------------------------------------------------------------------------
enum class Reroute {
    none,         // the plan stays as the layout left it
    own,          // the algorithm's own kernel holds on a pattern so_runs would take: no masks, not the packed matcher either
    gram_window,  // the same, with bndm_scan's gram mark in the plan's halo
    so_runs       // the plan carries Shift-Or masks as well
};

// Patterns that are counted by the Shift-Or runs kernel whatever the algorithm (launch.hip route): their
// plans carry its masks as well.
//  * Symbols repeat (the rule above; or, for 7 bytes and fewer, some symbol occurs twice): small alphabets,
//    natural language, rand32.  Round 1 sent these to the packed matcher, which tests two or three fingerprint
//    dwords in most rows there (rand4 64-72 %, English below 32 bytes 70-73 %, rand32 short 72-76 %); so_runs
//    does the same work whatever the bytes are and since round 2 runs at 75-81 % on all of them (English from 32
//    bytes on: 79-80 % both).  On random text over a large alphabet symbols do not repeat and nothing changes.
//  * 8+ bytes whose first dword says next to nothing about where the pattern occurs (two to four symbols:
//    every lane of the packed matcher keeps a candidate through all four fingerprint dwords, every skip is a byte
//    or two): the chance that 4 text bytes drawn like the pattern's own equal P[0..4), times the 16 alignments a
//    lane tests, is 0.03 or more (8+ bytes; up to four symbols).
// SO and SA keep their own serial kernel, KMP its own from 9 bytes on — where its automaton can have the borderless
// states 0..4 that the four-bytes-at-a-time form for natural language and medium alphabets needs (kmp_runs: K + 4 < w).
// Below that kmp_runs has its state-0 form from 5 bytes and a lookup per byte otherwise, and counts frequent
// occurrences byte by byte: m = 8: 61-72 % against so_runs' 74-81 % on every corpus; m = 2: 54 % against 76-78 %.
// Karp-Rabin its own from 16 bytes on, EPSM its packed matcher (it IS that algorithm).
Reroute so_reroute(int algo, const uint8_t* P, uint32_t m, const PatternStats& st, const Chosen& ch)
{
    if ((algo == SMARTGPU_KMP && m >= 9) || algo == SMARTGPU_SO || algo == SMARTGPU_SA || (algo == SMARTGPU_KR && m >= 16)) return Reroute::none;
    const uint32_t distinct = st.distinct;
    // * Short patterns (below the algorithm's measured crossover with its own skip loop, launch.hip packed_max_m):
    //   the every-byte kernels win there; so_runs and the packed matcher are equal on rand128 (76-77 %), so_runs
    //   ahead on everything else (rand256, rand32, English at m = 2, 4: 78-81 % against 67-76 %).
    bool to_so = (algo == SMARTGPU_KR || algo == SMARTGPU_KMP) ? true : (st.repeats || st.repeats_short || m <= short_pattern_max_m(algo)) && algo != SMARTGPU_EPSM;
    // Round 3: where the algorithm's OWN kernel holds on such patterns, it keeps them (a configuration that
    // names Boyer-Moore or BNDM should not be a Shift-Or measurement).  bm_scan's flat loop: 72-74 % on English from 8
    // bytes on (so_runs 79-81 %); an alphabet of a few symbols shifts it by a byte or two (16-60 %): stays with so_runs.
    // bndm_scan with q-grams: 74-79 % on four symbols and 75-76 % on English from 16 bytes on, 66-71 % on two from 32
    // (q = 8); below those lengths it is iteration-bound.
    bool own_holds = false;
    // (hor_scan's flat form, VAR 9, for Horspool and Tuned BM: 68-70 % on English and rand32 from 8 bytes on)
    if (algo == SMARTGPU_BM || algo == SMARTGPU_HOR || algo == SMARTGPU_TUNEDBM)
        own_holds = m >= 8 && !(distinct <= 8 && 2 * distinct <= m);  // not: a few symbols, each several times
    // ... unless Horspool has its q-gram table for them and a window long enough for its shifts (within 5-10 points of so_runs)
    if (ch.hor_q) own_holds = distinct <= 2 ? m >= 64 : m >= 32;
    // ... and, round 4, Horspool on GRAMS (k_horg.hip: one exact gram lookup per window on a text of at most four byte values,
    // 0.7-0.8 of the roofline from 8 bytes on): like BNDM's gram form a bet that the text holds no more byte values than
    // the pattern (on any other text the launch falls back to the hash table above, or the byte table)
    // (own kernel, 1 GiB: two values m = 16 / 32 / 64+: 0.66 / 0.76 / 0.79-0.83, four values: 0.75 / 0.79 / 0.80-0.85; 8 bytes:
    // 0.37 / 0.63 — a window of one or two grams: those stay with so_runs)
    // (Boyer-Moore likewise, k_bmg.hip: its good-suffix rule joined with the gram's shift)
    // (two symbols, 16 bytes — a window of two grams —: 0.66-0.69 against so_runs' 0.77: those from 32 bytes on, 0.78-0.81)
    if ((algo == SMARTGPU_HOR || algo == SMARTGPU_BM || algo == SMARTGPU_TUNEDBM) && distinct >= 2 && distinct <= 4) own_holds = m >= (distinct <= 2 ? 32u : 16u);
    const bool bndm = algo == SMARTGPU_BNDM || (algo == SMARTGPU_BNDML && m <= 32);
    if (bndm) own_holds = ch.bndm_q == ch.bndm_q_wanted && (ch.bndm_q >= 8 ? m >= 32 : m >= 16);
    // BNDM over two to four symbols, 8+ bytes: on a text of at most four byte values bndm_scan's GRAM form decides every
    // window with one lookup (k_bndm.hip bndm_gram: 0.74-0.8 of the roofline on rand2 / rand4 at any such length; so_runs
    // 0.77).  The plan cannot see the text; a pattern of two to four symbols cut from it says what it most likely is
    // (on any other text the launch falls back to the mask loop — correct, and slow on such a pattern).
    const bool gram_window = bndm && m >= 8 && distinct >= 2 && distinct <= 4;
    if (gram_window) return Reroute::gram_window;
    if (own_holds && m > short_pattern_max_m(algo)) return Reroute::own;
    if (!to_so && m >= 8) {  // (8 bytes of distinct symbols estimate 16/8^4 = 0.004: below that the histogram says nothing)
        double pass = 16.0;
        for (uint32_t i = 0; i < 4; ++i) pass *= static_cast<double>(st.cnt[P[i]]) / m;
        // rand2: 1.0, rand3: 0.2, rand4: 0.06, rand8: 0.004.  Round 1 drew the line at 0.15 (so_runs then ran at
        // 63-68 %); at 75-81 % it also beats the packed matcher on rand4 (EPSM there: 59-67 %, a second
        // fingerprint dword in nearly every row), not on rand8 and up.
        to_so = pass >= 0.03;
        // EPSM keeps every pattern but the long ones over two symbols: its v_mqsad modes do the same work whatever the text holds
        // (k_packed.hip: 0.78-0.80 of the roofline on four byte values at any length; two values from 13 bytes on: 0.70-0.74, so_runs 0.77)
        if (algo == SMARTGPU_EPSM) to_so = distinct <= 2 && m >= 13;
    }
    return to_so ? Reroute::so_runs : Reroute::none;
}

// the algorithm's own tables behind the pattern slot; the plan words they decide
void layout_tables(Blob& blob, int algo, const uint8_t* P, uint32_t m, const PatternStats& st, PlanWords& pw, Chosen& ch)
{
    uint16_t tab[256];
    switch (algo) {
        case SMARTGPU_TUNEDBM:
        case SMARTGPU_RAITA:
        case SMARTGPU_HOR:
            ch.hor_q = layout_horspool(blob, algo, P, m, st);
            pw.halo |= ch.hor_q << 8;
            pw.prefer_packed = st.repeats;
            break;
        case SMARTGPU_BM:
            layout_bm(blob, P, m, pw.halo);
            pw.prefer_packed = st.repeats;
            break;
        case SMARTGPU_KMP:
            pw.halo = m - 1;  // forward halo: the automaton re-scans m-1 bytes
            pw.prefer_packed = layout_kmp(blob, P, m);
            break;
        case SMARTGPU_SA:
            // sa.c:52 is D = ((D << 1) | 1) & S[c]; with E = ~D that is E = (E << 1) | ~S[c] — Shift-Or's step
            // on Shift-Or's masks, and "bit w-1 of D set" is "bit w-1 of E clear": the same automaton in
            // complement.  The kernel runs that form (one VALU op per byte less: there is no shift-and-AND
            // instruction); the AND form stays selectable (smartgpu_tune(6,3)) on the masks that follow.
            append(blob, shift_or_masks(P, m).data(), 1024);
            append(blob, shift_and_masks(P, m).data(), 1024);
            break;
        case SMARTGPU_SO:
            append(blob, shift_or_masks(P, m).data(), 1024);
            break;
        case SMARTGPU_BNDML:
            if (m > 32) {
                layout_bndml(blob, P, m);
                pw.prefer_packed = st.repeats;
                break;
            }
            [[fallthrough]];  // m <= 32: plain BNDM (bndml.c:44-75)
        case SMARTGPU_SBNDM:
        case SMARTGPU_BNDM:
            layout_bndm(blob, algo, P, m);
            if (algo != SMARTGPU_SBNDM) {
                choose_bndm_q(m, st, ch);
                pw.halo = ch.bndm_q;
            }
            pw.prefer_packed = st.repeats;
            break;
        case SMARTGPU_EPSM:
            append_fingerprint(blob, P, m);
            break;
        case SMARTGPU_KR:
            layout_kr(blob, P, m);
            pw.halo = std::min<uint32_t>(m - 1, 32);  // bytes confirmed in LDS (and the hash's reach) behind a window end
            break;
        case SMARTGPU_HASH3:
        case SMARTGPU_HASH5:
        case SMARTGPU_HASH8:  // same layout as HOR: u16 table (zero entry = flag | shift after a candidate)
            qgram_table(P, m, algo == SMARTGPU_HASH3 ? 3 : algo == SMARTGPU_HASH5 ? 5 : 8, tab);
            layout_shift_table(blob, tab, nullptr, P, m);
            pw.prefer_packed = st.repeats;
            break;
        case SMARTGPU_QS: {  // same layout as HOR: u16 table, 256 spare bytes, fingerprint
            const std::vector<int32_t> qs = quick_search_shifts(P, m);
            for (int c = 0; c < 256; ++c) tab[c] = static_cast<uint16_t>(qs[c]);
            layout_shift_table(blob, tab, nullptr, P, m);
            pw.prefer_packed = st.repeats;
            break;
        }
    }
}

}  // namespace

PlanWords build_blob(std::vector<uint8_t>& blob, int algo, const uint8_t* P, uint32_t m)
{
    PlanWords pw;
    blob.clear();
    blob.resize(kPatternBytes, 0);
    std::memcpy(blob.data(), P, m);
    const PatternStats st = pattern_stats(P, m);
    // The opposite case: symbols do not repeat (random text over a large alphabet).  Windows then die on
    // their first comparison and a skip kernel only streams; it runs best with FEWER workgroups per CU
    // (tile_wgs in launch_common.hpp, measured).  Patterns with repeating symbols that still run on a tile
    // kernel (tune(0,1), KR) keep the lanes busy verifying: more workgroups hide that.  How many exactly
    // depends on m and the kernel: tile_wgs() in launch_common.hpp.
    // (An earlier form — >= 80 % of the first min(m,64) symbols distinct — missed rand128 at m = 64,
    // 50 distinct symbols expected: HOR 80 %, BM 76 %, BNDM 71 % there against 84-87 % at m = 32 and 128.)
    pw.sparse = m >= 8 && !st.repeats;
    pw.halo = std::min<uint32_t>(m - 1, kHaloMax);
    Chosen ch;
    layout_tables(blob, algo, P, m, st, pw, ch);
    switch (so_reroute(algo, P, m, st, ch)) {
        case Reroute::none:
            break;
        case Reroute::gram_window:
            pw.halo |= kBndmGramWindow;
            [[fallthrough]];
        case Reroute::own:
            pw.prefer_packed = 0;
            break;
        case Reroute::so_runs:
            align_up(blob, 16);
            pw.so_off = static_cast<uint32_t>(blob.size());
            append(blob, shift_or_masks(P, m).data(), 1024);
            break;
    }
    align_up(blob, 256);
    return pw;
}

}  // namespace sg
