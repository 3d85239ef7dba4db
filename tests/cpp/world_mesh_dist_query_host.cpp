#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
#include <cstddef>
// compile-only: mesh clearance over an instance world in the header layer (not in the reference) against the C ABI's
// declarations (tests/test_world_mesh_dist_cpu.py); never run against a device
static_assert(sizeof(psm_mesh_hit) == 32 && sizeof(psm_tri_hit) == 32, "two 16-byte stores each");
int clearance(psm::InstanceWorld & world, psm::TriangleHierarchy & other, const glm::mat4 * poses, size_t p, psm_tri_hit * d_hits,
              psm_mesh_hit * d_pairs, int32_t * d_inst, uint8_t * d_flag) {
    int rc = world.closestToMesh(&other, poses, p, -1, 2.5f, d_hits, d_inst);
    if (rc == PSM_OK) rc = world.withinOfMesh(&other, poses, p, -1, 0.002f, d_flag);
    if (rc == PSM_OK) rc = world.withinOfMesh(&other, poses, p, 3, 0.002f, d_flag);   // instance 3 left out
    return rc != PSM_OK ? rc : world.clearanceToMesh(&other, poses, p, 0, 1e30f, d_pairs, d_inst);
}
int main() { return 0; }
