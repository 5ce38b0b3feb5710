// plan.hpp — the plan builder (plan.cpp): which kernel a pattern runs on, and the tables that kernel reads laid out as the
// blob the device gets.  Host only: no HIP call, no device state, no error reporting — api.cpp checks patterns, reports
// and knows texts; tests/dispatch_driver.cpp links plan.cpp without api.cpp.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/smartgpu.h"
#include "route.hpp"

#pragma GCC visibility push(hidden)  // as when these lived in api.cpp: no symbol of the library's
namespace sg {

extern const char* const kAlgoNames[SMARTGPU_NUM_ALGOS];

// shortest pattern an algorithm applies to (the reference returns -1 below it: raita.c:37, hash3.c:31, ...)
uint32_t min_pattern(int algo);

// Build the device blob (pattern + tables) for (algo, P, m) in `blob` (cleared first; a caller that builds many
// reuses one vector: fresh memory for every blob of a pattern set cost more in page faults than the tables in work).
// 0 <= algo < SMARTGPU_NUM_ALGOS, min_pattern(algo) <= m <= SMARTGPU_XSIZE: the caller has checked.
PlanWords build_blob(std::vector<uint8_t>& blob, int algo, const uint8_t* P, uint32_t m);

}  // namespace sg
#pragma GCC visibility pop
