// palignl_calls.cpp — the C ABI's align calls on packed texts for LONG patterns (m <= 256, k <= 31; palignl.hpp, k_palignl.hip):
// the two exported functions.  Their host path is the align calls' one path, align_run of align_calls.cpp, reached through
// palignl_run; as everywhere in the C ABI there is no CPU path: a kernel that is not linked is an error, never a fall-back.
#include "../../include/smartgpu.h"

#include "call_host.hpp"
#include "palignl.hpp"

extern "C" {

int smartgpu_palign_editl64(const uint8_t* P, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                            const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    return palignl_run({"palign_editl64", P, false, false, m, k, 0, text, off, n}, ends, count, starts, distances, ops);
}

int smartgpu_palign_sets_editl64(const uint8_t* sets, uint32_t m, uint32_t k, const smartgpu_ptext* text, uint64_t off, uint64_t n,
                                 const uint64_t* ends, uint64_t count, uint64_t* starts, uint8_t* distances, uint64_t* ops)
{
    return palignl_run({"palign_sets_editl64", sets, true, false, m, k, 0, text, off, n}, ends, count, starts, distances, ops);
}

}  // extern "C"
