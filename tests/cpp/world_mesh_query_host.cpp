#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
#include <cstddef>
// compile-only: the mesh queries of an instance world in the header layer (not in the reference) against the C ABI's
// declarations (tests/test_world_mesh_cpu.py); never run against a device
static_assert(PSM_QUERY_K_MAX == 16, "PSM_QUERY_K_MAX");
int meshes(psm::InstanceWorld & world, psm::TriangleHierarchy & other, const glm::mat4 * poses, size_t p, uint8_t * d_hit, uint32_t * d_count,
           int32_t * d_tri, int32_t * d_inst) {
    int rc = world.overlapsMesh(&other, poses, p, -1, d_hit);
    if (rc == PSM_OK) rc = world.countOnMesh(&other, poses, p, -1, d_count);
    if (rc == PSM_OK) rc = world.countOnMesh(&other, poses, p, 0, d_count);   // instance 0 left out
    if (rc == PSM_OK) rc = world.trianglesOnMesh(&other, poses, p, 3, 4, d_tri, d_inst, d_count);
    return rc != PSM_OK ? rc : world.trianglesOnMesh(&other, poses, p, -1, PSM_QUERY_K_MAX, d_tri, d_inst, d_count);
}
int main() { return 0; }
