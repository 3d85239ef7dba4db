// psm_mesh_dist_key.h -- the word a pose's lanes share in the mesh clearance query (mesh_dist.hip; include/psm_hip.h "mesh
// clearance"): key = (bits(dist) << 32) | t, dist the float32 distance of a pair that counts and t the load-order
// id of other's triangle. A distance that counts is never negative and never NaN (it passed sqrtf(d2) <= rmax), so its bits
// order as the float does -- +0 lowest (sqrtf gives no -0 for a d2 that is a sum of squares), then the denormals, the normal
// numbers and +inf = 0x7f800000 -- and the unsigned order of the word is the order of (dist, t). All-ones is "none": its
// high half is a NaN's bits, which no key holds. Compiles for the host too: a stand-alone program defines PSM_KEY_FN as a host
// function's decoration before it includes this file (tests/cpp/mesh_dist_key_host.cpp).
#pragma once
#include <cstdint>
#include <cstring>

#ifndef PSM_KEY_FN
#define PSM_KEY_FN __device__ __forceinline__
#endif

namespace psm {

constexpr uint64_t MESH_KEY_NONE = ~(uint64_t)0;

PSM_KEY_FN uint64_t mesh_key(float dist, uint32_t t) {
    uint32_t bits;
    memcpy(&bits, &dist, sizeof bits);
    return ((uint64_t)bits << 32) | t;
}

// the dist of a key that is not MESH_KEY_NONE, and its triangle
PSM_KEY_FN float mesh_key_dist(uint64_t key) {
    const uint32_t bits = (uint32_t)(key >> 32);
    float d;
    memcpy(&d, &bits, sizeof d);
    return d;
}
PSM_KEY_FN uint32_t mesh_key_tri(uint64_t key) { return (uint32_t)key; }

}  // namespace psm
