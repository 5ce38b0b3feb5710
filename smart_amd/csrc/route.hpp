// route.hpp — which launcher a plan leads to: ONE decision (route, launch.hip) behind launch_scan, scan_kernel_name and the
// groups of a pattern set in one grid (group_key).  Host-only; included by launch.hip, plan.hpp and api.cpp, by no kernel unit.
#pragma once
#include "kernels.hpp"

namespace sg {

// The four words a plan carries besides its tables, as plan.cpp build_blob encodes them (ScanArgs holds the same four):
//  halo           bits 0-7: the skip kernels' back halo H = min(m-1, kHaloMax) (KR: min(m-1, 32); KMP: m-1, forward) — for
//                 BNDM / BNDML (m <= 32) bndm_scan's q instead, with kBndmGramWindow (bit 8) beside it;
//                 bits 8-15, HOR only: the q of Horspool's q-gram table (0: the byte table)
//  prefer_packed  a flag: the pattern's symbols repeat, the packed matcher beats the skip loop — for KMP instead the window
//                 of its four-bytes-per-step table (0: the plan carries none)
//  sparse         a flag: symbols do not repeat, a skip kernel only streams (fewer workgroups per CU: tile_wgs)
//  so_off         blob offset of Shift-Or masks: != 0 for a pattern of another algorithm that so_runs counts (the reroute)
struct PlanWords { uint32_t halo = 0, prefer_packed = 0, sparse = 0, so_off = 0; };
inline uint32_t hor_q(const PlanWords& w) { return (w.halo >> 8) & 0xFFu; }
inline uint32_t bndm_q_and_mark(const PlanWords& w) { return w.halo & (0xFFu | kBndmGramWindow); }

// the launchers of launch_common.hpp that launch_scan can reach
enum class Launcher { so_runs, packed, hor, hor_var, hor_bp, hor_gram, kr, bm, bm_gram, bndm, sbndm, bndml, kmp_runs };
struct Route {
    Launcher to;
    int arg;  // hor: q; hor_gram, bm_gram: gram; packed: kind; hor_var: the algorithm; else 0
};
// A pure function of its arguments and g_tune; the only place that holds the decision tree.
Route route(int algo, uint32_t m, const PlanWords& w, TextCodes codes);
// Patterns of one set (one algorithm, one length, one text) whose keys are equal may share a grid: their Route and every
// word a launcher reads for template arguments or grid are equal.
uint64_t group_key(int algo, uint32_t m, const PlanWords& w, TextCodes codes);

}  // namespace sg
