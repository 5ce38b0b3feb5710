// dispatch_driver.cpp — tests/test_dispatch.py builds this with plan.cpp, launch.hip and tables.cpp, for the product and
// for the A/B build, under AddressSanitizer and UBSan: the launchers of launch_common.hpp as STUBS that record what they were
// called with, and a main that drives launch_scan over a grid of (algorithm, pattern length, pattern, text codes,
// smartgpu_tune setting).  No GPU, no HIP call.
//
//   dispatch_driver <english text file> [--dump | --blobs]
//
// Checks, per plan: the layout facts of its blob that the kernels rely on without checking (check_blob).  Per grid point:
// launch_scan made exactly one launch, and scan_kernel_name names the kernel it launched (the gram
// launchers count as their base kernel).  Per pair of plans of one algorithm and length: an equal group_key means an equal
// launcher, argument and launcher-read words (what a pattern set in one grid relies on).  --dump prints every grid point.
// --blobs prints one line per plan — its words, the blob's size and a 64-bit FNV-1a hash of its bytes — and skips the grid:
// two trees build the same plans if their outputs are equal.
#include "../smart_amd/csrc/plan.hpp"  // build_blob, min_pattern: the plan builder itself, not a copy
#include "../smart_amd/csrc/launch_common.hpp"
#include "../smart_amd/csrc/tables.hpp"

#include <array>
#include <cstdio>
#include <cstring>
#include <string>

namespace sg {

struct Call { int n = 0; const char* launcher = ""; const char* kernel = ""; long extra = 0; ScanArgs a = {}; TextCodes codes; };
static Call g_call;
static hipError_t record(const char* launcher, const char* kernel, long extra, const ScanArgs& a, TextCodes codes = TextCodes())
{
    ++g_call.n;
    g_call.launcher = launcher;
    g_call.kernel = kernel;
    g_call.extra = extra;
    g_call.a = a;
    g_call.codes = codes;
    return hipSuccess;
}

hipError_t launch_hor(const ScanArgs& a, uint32_t q, int, hipStream_t) { return record("launch_hor", "hor_scan", q, a); }
hipError_t launch_hor_var(int algo, const ScanArgs& a, int, hipStream_t) { return record("launch_hor_var", "hor_scan", algo, a); }
hipError_t launch_kr(const ScanArgs& a, int, hipStream_t) { return record("launch_kr", "hor_scan_bp", 0, a); }
hipError_t launch_hor_gram(const ScanArgs& a, int gram, int, hipStream_t) { return record("launch_hor_gram", "hor_scan", gram, a); }
hipError_t launch_bm_gram(const ScanArgs& a, int gram, int, hipStream_t) { return record("launch_bm_gram", "bm_scan", gram, a); }
hipError_t launch_bm(const ScanArgs& a, int, hipStream_t) { return record("launch_bm", "bm_scan", 0, a); }
hipError_t launch_bndm(const ScanArgs& a, int, hipStream_t, TextCodes c) { return record("launch_bndm", "bndm_scan", 0, a, c); }
hipError_t launch_sbndm(const ScanArgs& a, int, hipStream_t) { return record("launch_sbndm", "sbndm_scan", 0, a); }
hipError_t launch_bndml(const ScanArgs& a, int, hipStream_t) { return record("launch_bndml", "bndml_scan", 0, a); }
hipError_t launch_so_runs(const ScanArgs& a, bool shift_and, int, hipStream_t, TextCodes c) { return record("launch_so_runs", "so_runs", shift_and, a, c); }
hipError_t launch_kmp_runs(const ScanArgs& a, int, hipStream_t, TextCodes c) { return record("launch_kmp_runs", "kmp_runs", 0, a, c); }
hipError_t launch_packed(int kind, const ScanArgs& a, int, hipStream_t, TextCodes c) { return record("launch_packed", "packed_scan", kind, a, c); }
#ifdef SMARTGPU_AB
hipError_t launch_hor_bp(const ScanArgs& a, int, hipStream_t) { return record("launch_hor_bp", "hor_scan_bp", 0, a); }
// the superseded kernels: which of them a setting selects, as k_ab.hip's launchers decide it
hipError_t launch_ab_so(int algo, const ScanArgs& a, int, hipStream_t, bool* handled)
{
    const char* k = (g_tune[6] == 2 && algo == SMARTGPU_SO) ? "so_runs64" : (g_tune[6] == 1 && algo == SMARTGPU_SO) ? "so_scan"
                  : ((algo == SMARTGPU_SA && g_tune[6] == 3) || g_tune[6] == 4) ? "so_runs1" : nullptr;
    *handled = k != nullptr;
    return k ? record("launch_ab_so", k, algo, a) : hipSuccess;
}
hipError_t launch_ab_kmp(const ScanArgs& a, int, hipStream_t, bool* handled)
{
    const char* k = (g_tune[3] == 1 && a.m <= 40) ? "kmp_scan" : g_tune[3] == 2 ? "kmp_links_runs" : g_tune[3] == 3 ? "kmp_runs1" : nullptr;
    *handled = k != nullptr;
    return k ? record("launch_ab_kmp", k, 0, a) : hipSuccess;
}
#endif

}  // namespace sg

// Bytes from kTableOff on that the algorithm's kernels find at places kernels.hpp states (sizes only: what the tables
// hold is tables.cpp's and the parity tests' matter).
static size_t own_table_bytes(int algo, uint32_t m, const sg::PlanWords& w)
{
    const size_t fp = 32;  // the fingerprint: u32 fp[4], u32 fpmask[4]
    switch (algo) {
        case SMARTGPU_BM: return ((2 * (768 + size_t(m) + 1) + 3) & ~size_t(3)) + fp;
        case SMARTGPU_KMP: {
            size_t end = sg::kmp_spread_off(m);  // next[m+1] and the compact table lie below it
            bool spread = w.prefer_packed != 0;
#ifdef SMARTGPU_AB
            spread = true;
#endif
            if (spread) end += sg::kmp_runs_table_bytes(w.prefer_packed ? w.prefer_packed : sg::kmp_window(m)) + sg::kKmpQBytes;
#ifdef SMARTGPU_AB
            end += 256 * 256;  // kmp_runs1's table follows it
#endif
            return end - sg::kTableOff;
        }
        case SMARTGPU_SO: return 1024;
        case SMARTGPU_SA: return 2048;
        case SMARTGPU_SBNDM: return 1024 + fp + 4;
        case SMARTGPU_BNDML:
            if (m > 32) return 1024 * (std::min(m, sg::kBndmlWindow) <= 64 ? 2 : std::min(m, sg::kBndmlWindow) <= 128 ? 4 : 8) + 4 + fp;
            return 1024 + fp;
        case SMARTGPU_BNDM: return 1024 + fp;
        case SMARTGPU_EPSM: return fp;
        case SMARTGPU_KR: return 4 + fp;
        default: return 512 + 256 + fp;  // HOR's layout: TUNEDBM, RAITA, HASH3/5/8, QS
    }
}

// What the kernels rely on without checking; `blob` is the vector the driver reuses for every plan.  Returns the failures.
static int check_blob(int algo, const uint8_t* P, uint32_t m, const char* corpus, const std::vector<uint8_t>& blob, const sg::PlanWords& w)
{
    int bad = 0;
    auto fail = [&](const char* what) { printf("BLOB MISMATCH %s m=%u %s: %s (size %zu, so_off %u)\n", sg::kAlgoNames[algo], m, corpus, what, blob.size(), w.so_off); ++bad; };
    if (blob.size() % 256 || blob.size() < sg::kPatternBytes) { fail("size is no multiple of 256 or below the pattern slot"); return bad; }
    if (std::memcmp(blob.data(), P, m)) fail("bytes [0, m) are not the pattern");
    for (uint32_t i = m; i < sg::kPatternBytes; ++i)
        if (blob[i]) { fail("a byte of [m, kPatternBytes) is not zero"); break; }
    size_t tables_end = blob.size();
    if (w.so_off) {
        if (w.so_off % 16 || w.so_off < sg::kPatternBytes || size_t(w.so_off) + 1024 > blob.size()) { fail("so_off is unaligned, inside the pattern slot or its masks end outside the blob"); return bad; }
        const std::vector<uint32_t> S = sg::shift_or_masks(P, m);
        if (std::memcmp(blob.data() + w.so_off, S.data(), 1024)) fail("the dwords at so_off are not the Shift-Or masks");
        tables_end = w.so_off;
    }
    if (sg::kTableOff + own_table_bytes(algo, m, w) > tables_end) fail("the algorithm's own tables do not fit below so_off / the blob's end");
    std::vector<uint8_t> fresh;
    const sg::PlanWords f = sg::build_blob(fresh, algo, P, m);
    if (fresh != blob || f.halo != w.halo || f.prefer_packed != w.prefer_packed || f.sparse != w.sparse || f.so_off != w.so_off) fail("a build into a fresh vector differs from the build into the reused one");
    return bad;
}

static unsigned long long fnv1a(const std::vector<uint8_t>& v)
{
    unsigned long long h = 14695981039346656037ull;
    for (uint8_t b : v) h = (h ^ b) * 1099511628211ull;
    return h;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <english text file> [--dump | --blobs]\n", argv[0]); return 2; }
    const bool dump = argc > 2 && std::string(argv[2]) == "--dump";
    const bool blobs = argc > 2 && std::string(argv[2]) == "--blobs";
    std::vector<uint32_t> ms;
    for (uint32_t m = 1; m <= 40; ++m) ms.push_back(m);
    for (uint32_t m : {47u, 48u, 63u, 64u, 65u, 255u, 256u, 4096u}) ms.push_back(m);
    // the corpora patterns are cut from: rand2, rand4, English, rand128
    const char* corpus_names[4] = {"rand2", "rand4", "english", "rand128"};
    std::vector<uint8_t> corpus[4];
    {
        unsigned long long x = 88172645463325252ull;
        auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
        const int sigma[4] = {2, 4, 0, 128};
        for (int c = 0; c < 4; ++c)
            for (int i = 0; sigma[c] && i < 32768; ++i) corpus[c].push_back(static_cast<uint8_t>((sigma[c] <= 4 ? 'a' : 0) + rnd() % sigma[c]));
        FILE* f = fopen(argv[1], "rb");
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        corpus[2].resize(32768);
        const size_t got = fread(corpus[2].data(), 1, corpus[2].size(), f);
        fclose(f);
        if (got != corpus[2].size()) { fprintf(stderr, "%s is shorter than 32768 bytes\n", argv[1]); return 2; }
    }
    // the text's codes: none, four byte values, two byte values (a two-value text has two-bit codes as well)
    sg::TextCodes codes[3];
    codes[1].shift = 0; codes[1].symtab = 0x64636261u;
    codes[2].shift = 0; codes[2].symtab = 0xFFFF6261u; codes[2].one = 0u | ('a' << 8) | ('b' << 16);
    // every combination of the settings launch.hip reads that this build accepts
    std::vector<std::array<int, 4>> tunes;
    for (int t0 : {0, 1, 2, 3})
        for (int t2 : {0, 4})
            for (int t3 : {0, 1, 2, 3, 5, 6})
                for (int t6 : {0, 1, 2, 3, 4, 5})
                    if (sg::tune_supported(0, t0) && sg::tune_supported(2, t2) && sg::tune_supported(3, t3) && sg::tune_supported(6, t6)) tunes.push_back({t0, t2, t3, t6});
    std::vector<uint8_t> blob;
    unsigned long long points = 0, pairs = 0, bad = 0;
    for (int algo = 0; algo < SMARTGPU_NUM_ALGOS; ++algo)
        for (uint32_t m : ms) {
            if (m < sg::min_pattern(algo)) continue;  // the algorithm does not apply to this length
            sg::PlanWords words[4];
            for (int c = 0; c < 4; ++c) {
                const uint8_t* P = corpus[c].data() + 1000 + 3 * m;
                const sg::PlanWords w = words[c] = sg::build_blob(blob, algo, P, m);
                bad += check_blob(algo, P, m, corpus_names[c], blob, w);
                if (blobs) printf("%s m=%u %s words=%x,%u,%u,%u size=%zu fnv1a=%016llx\n", sg::kAlgoNames[algo], m, corpus_names[c], w.halo, w.prefer_packed, w.sparse, w.so_off, blob.size(), fnv1a(blob));
            }
            if (blobs) continue;
            for (const auto& t : tunes) {
                sg::g_tune[0] = t[0]; sg::g_tune[2] = t[1]; sg::g_tune[3] = t[2]; sg::g_tune[6] = t[3];
                for (int tc = 0; tc < 3; ++tc) {
                    sg::Call calls[4];
                    uint64_t keys[4];
                    for (int c = 0; c < 4; ++c) {
                        const sg::PlanWords& w = words[c];
                        sg::ScanArgs a = {};
                        a.s_end = 1u << 20;
                        a.m = m;
                        a.halo = w.halo; a.prefer_packed = w.prefer_packed; a.sparse = w.sparse; a.so_off = w.so_off;
                        sg::g_call = sg::Call();
                        const hipError_t e = sg::launch_scan(algo, a, 256, nullptr, codes[tc]);
                        const char* name = sg::scan_kernel_name(algo, m, w.prefer_packed != 0, w.so_off != 0, w.halo);
                        const sg::Call& k = sg::g_call;
                        calls[c] = k;
                        keys[c] = sg::group_key(algo, m, w, codes[tc]);
                        ++points;
                        const bool ok = e == hipSuccess && k.n == 1 && std::strcmp(name, k.kernel) == 0;
                        if (dump || !ok)
                            printf("%s%s m=%u %s codes=%d tune=%d,%d,%d,%d words=%x,%u,%u,%u name=%s -> %s(%ld) %s x%d halo=%u fp_off=%u pp=%u sparse=%u so_off=%u codes=%u,%x,%x\n",
                                   ok ? "" : "MISMATCH ", sg::kAlgoNames[algo], m, corpus_names[c], tc, t[0], t[1], t[2], t[3], w.halo, w.prefer_packed, w.sparse, w.so_off,
                                   name, k.launcher, k.extra, k.kernel, k.n, k.a.halo, k.a.fp_off, k.a.prefer_packed, k.a.sparse, k.a.so_off, k.codes.shift, k.codes.symtab, k.codes.one);
                        bad += !ok;
                    }
                    for (int x = 0; x < 4; ++x)
                        for (int y = x + 1; y < 4; ++y) {
                            ++pairs;
                            if (keys[x] != keys[y]) continue;
                            const sg::Call &p = calls[x], &q = calls[y];
                            if (p.launcher == q.launcher && p.kernel == q.kernel && p.extra == q.extra && p.a.halo == q.a.halo && p.a.prefer_packed == q.a.prefer_packed && p.a.sparse == q.a.sparse) continue;
                            printf("GROUP MISMATCH %s m=%u %s / %s codes=%d tune=%d,%d,%d,%d: one key, %s(%ld) and %s(%ld)\n", sg::kAlgoNames[algo], m, corpus_names[x], corpus_names[y],
                                   tc, t[0], t[1], t[2], t[3], p.launcher, p.extra, q.launcher, q.extra);
                            ++bad;
                        }
                }
            }
        }
    fprintf(dump || blobs ? stderr : stdout, "%llu grid points, %llu pairs, %zu tune settings, %llu failures\n", points, pairs, tunes.size(), bad);
    return bad ? 1 : 0;
}
