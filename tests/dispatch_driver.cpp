// dispatch_driver.cpp — tests/test_dispatch.py builds this with launch.hip and tables.cpp, for the product and for the A/B
// build: the launchers of launch_common.hpp as STUBS that record what they were called with, and a main that drives
// launch_scan over a grid of (algorithm, pattern length, pattern, text codes, smartgpu_tune setting).  No GPU, no HIP call.
//
//   dispatch_driver <english text file> [--dump]
//
// Checks, per grid point: launch_scan made exactly one launch, and scan_kernel_name names the kernel it launched (the gram
// launchers count as their base kernel).  Per pair of plans of one algorithm and length: an equal group_key means an equal
// launcher, argument and launcher-read words (what a pattern set in one grid relies on).  --dump prints every grid point.
#include "../smart_amd/csrc/api.cpp"  // build_blob, check_pattern: the plan builder itself, not a copy
#include "../smart_amd/csrc/launch_common.hpp"

#include <array>

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
// what else api.cpp links against; never called here
hipError_t launch_find(const ScanArgs&, unsigned long long*, unsigned long long, int, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_generate(uint8_t*, uint64_t, int, uint64_t, uint64_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_tile_fill(uint8_t*, const uint8_t*, uint64_t, uint64_t, uint64_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_text_alphabet(const uint8_t*, uint64_t, uint32_t*, int, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_probe_read(const uint8_t*, uint64_t, unsigned long long*, int, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_planes_pack(const uint8_t*, uint64_t, uint32_t*, uint32_t*, int, const uint8_t[3], hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_planes_scan(const PlaneArgs&, int, int, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_planes_find(const PlaneArgs&, unsigned long long*, unsigned long long, int, int, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_planes_sets_scan(const PlaneSetArgs&, int, int, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_planes_sets_find(const PlaneSetArgs&, unsigned long long*, unsigned long long, int, int, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_planes_mis_scan(const PlaneMisArgs&, int, int, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_planes_mis_find(const PlaneMisArgs&, unsigned long long*, unsigned long long, int, int, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_planes_sets_mis_scan(const PlaneSetMisArgs&, int, int, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_planes_sets_mis_find(const PlaneSetMisArgs&, unsigned long long*, unsigned long long, int, int, hipStream_t) { return hipErrorNotSupported; }

}  // namespace sg

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <english text file> [--dump]\n", argv[0]); return 2; }
    const bool dump = argc > 2 && std::string(argv[2]) == "--dump";
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
            const uint8_t* P0 = corpus[0].data() + 1000 + 3 * m;
            if (check_pattern(algo, P0, m) != SMARTGPU_OK) continue;  // the algorithm does not apply to this length
            sg::PlanWords words[4];
            for (int c = 0; c < 4; ++c) words[c] = build_blob(blob, algo, corpus[c].data() + 1000 + 3 * m, m);
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
                                   ok ? "" : "MISMATCH ", kAlgoNames[algo], m, corpus_names[c], tc, t[0], t[1], t[2], t[3], w.halo, w.prefer_packed, w.sparse, w.so_off,
                                   name, k.launcher, k.extra, k.kernel, k.n, k.a.halo, k.a.fp_off, k.a.prefer_packed, k.a.sparse, k.a.so_off, k.codes.shift, k.codes.symtab, k.codes.one);
                        bad += !ok;
                    }
                    for (int x = 0; x < 4; ++x)
                        for (int y = x + 1; y < 4; ++y) {
                            ++pairs;
                            if (keys[x] != keys[y]) continue;
                            const sg::Call &p = calls[x], &q = calls[y];
                            if (p.launcher == q.launcher && p.kernel == q.kernel && p.extra == q.extra && p.a.halo == q.a.halo && p.a.prefer_packed == q.a.prefer_packed && p.a.sparse == q.a.sparse) continue;
                            printf("GROUP MISMATCH %s m=%u %s / %s codes=%d tune=%d,%d,%d,%d: one key, %s(%ld) and %s(%ld)\n", kAlgoNames[algo], m, corpus_names[x], corpus_names[y],
                                   tc, t[0], t[1], t[2], t[3], p.launcher, p.extra, q.launcher, q.extra);
                            ++bad;
                        }
                }
            }
        }
    fprintf(dump ? stderr : stdout, "%llu grid points, %llu pairs, %zu tune settings, %llu failures\n", points, pairs, tunes.size(), bad);
    return bad ? 1 : 0;
}
