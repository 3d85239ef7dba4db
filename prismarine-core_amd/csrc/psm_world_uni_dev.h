// psm_world_uni_dev.h -- what the brick walks over a world share (world_grid.hip, world_grid_dist.hip): a
// wave-uniform value as the scalar it is, and the pointers of a table row read as constant memory. Moved here from
// world_grid.hip as they were; world_grid.hip's kernels compile to the same instructions as with the pieces in their own file
// (tools/kernel_diff.py).
#pragma once
#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"

namespace psm {

namespace {

// a value every lane holds alike, as the scalar the compiler may not know it to be
PSM_D uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
// The pointers a row holds are integers a lane loaded: the compiler knows neither that the kernel's stores leave what they point
// to alone nor which address space they mean, and fetches through them with flat vector loads. They point to records, triangles
// and hierarchy constants that no store of these kernels touches: read as constant memory, they come through scalar loads, as
// grid.hip's do
#define PSM_CONST __attribute__((address_space(4)))
PSM_D const PSM_CONST uint32_t* uni_ptr(uint32_t lo, uint32_t hi) { return (const PSM_CONST uint32_t*)(((uint64_t)uni(hi) << 32) | uni(lo)); }
// (word by word: the vector types copy from generic memory alone; the compiler makes one s_load_dwordx4 / x8 of the words)
PSM_D uint4 words4(const PSM_CONST uint32_t* p) { return make_uint4(p[0], p[1], p[2], p[3]); }
PSM_D v3 floats3(const PSM_CONST uint32_t* p) { return mk3(u2f(p[0]), u2f(p[1]), u2f(p[2])); }

}  // namespace

}  // namespace psm
