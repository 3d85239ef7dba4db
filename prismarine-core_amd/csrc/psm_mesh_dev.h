// psm_mesh_dev.h -- what a mesh query (mesh.hip, and world_mesh.hip over a world; include/psm_hip.h "mesh queries") adds in front of the triangle
// queries' candidate test: which (pose, leaf) a launch's query i is, and the query triangle of a stored leaf at a pose. Both also
// compile for the host: a stand-alone program defines PSM_MESH_FN (and PSM_TRI_FN, PSM_WORLD_BOX_FN) as a host function's
// decoration before it includes this file (tests/cpp/mesh_pose_host.cpp), and the CPU test holds what they compute against
// tests/mesh_query_model.py record for record.
#pragma once
#include "psm_common.h"
#include "psm_internal.h"
#include "psm_world_box_dev.h"   // fwd_point, fwd_vec
#include "psm_tri_dev.h"         // tri_tri

#ifndef PSM_MESH_FN
#define PSM_MESH_FN PSM_D
#endif

namespace psm {

// the most answers (poses x triangles) of one call, over a hierarchy or a world: the kernels index them with 32 bits (mesh_split
// is exact up to 2^37); mesh.hip's mesh_answers_fit() is the one check
constexpr uint64_t MESH_QUERIES_MAX = (uint64_t)1 << 32;

// The multiplier of mesh_split for L leaves, 1 <= L < 2^27: ceil(2^64 / L), and 0 for L = 1 (2^64 has no 64-bit form).
inline uint64_t mesh_magic(uint32_t L) { return L <= 1u ? 0u : ~(uint64_t)0 / L + 1u; }

namespace {

// Query i of a launch over p poses and L leaves: pose q = i / L and leaf j = i % L, without a division (the kernels hold
// none). With M = ceil(2^64 / L) = (2^64 + e) / L, 0 <= e < L, the high word of i M is floor(i / L + i e / (2^64 L)), and the second
// term is below 1 / L while i e < 2^64: for every i < 2^37, L < 2^27 (i < MESH_QUERIES_MAX = 2^32 here).
PSM_MESH_FN void mesh_split(uint64_t i, uint32_t L, uint64_t magic, uint64_t& q, uint32_t& j) {
#if defined(__HIP_DEVICE_COMPILE__)
    q = magic ? __umul64hi(i, magic) : i;
#else
    q = magic ? (uint64_t)(((unsigned __int128)i * magic) >> 64) : i;
#endif
    j = (uint32_t)(i - q * L);
}

// The query triangle of a stored leaf (v0, e1, e2) at the pose m (row-major [R | T], 12 floats): a = fwd_point(m, v0),
// b = a + fwd_vec(m, e1), c = a + fwd_vec(m, e2), float32 with one rounding per operation
PSM_MESH_FN void mesh_query_tri(const float* m, v3 v0, v3 e1, v3 e2, v3& a, v3& b, v3& c) {
    a = fwd_point(m, v0);
    b = a + fwd_vec(m, e1);
    c = a + fwd_vec(m, e2);
}

}  // namespace

}  // namespace psm
