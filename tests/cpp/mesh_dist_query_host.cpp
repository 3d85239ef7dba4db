#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
#include <cstddef>
// compile-only: mesh clearance of the header layer (not in the reference) against the C ABI's declarations
static_assert(sizeof(psm_mesh_hit) == 32, "psm_mesh_hit: two 16-byte stores");
static_assert(offsetof(psm_mesh_hit, dist) == offsetof(psm_tri_hit, dist) && offsetof(psm_mesh_hit, tri) == offsetof(psm_tri_hit, tri) &&
                  offsetof(psm_mesh_hit, s) == offsetof(psm_tri_hit, s) && offsetof(psm_mesh_hit, t) == offsetof(psm_tri_hit, t) &&
                  offsetof(psm_mesh_hit, other) == 24,
              "psm_mesh_hit: a psm_tri_hit with the other mesh's triangle where its first zero is");
int clearance(psm::TriangleHierarchy & th, psm::TriangleHierarchy & other, const glm::mat4 * poses, size_t p, psm_tri_hit * d_hits,
              psm_mesh_hit * d_pairs, uint8_t * d_flag) {
    int rc = th.meshClosest(&other, poses, p, 0.5f, d_hits);
    if (rc == PSM_OK) rc = th.meshWithin(&other, poses, p, 0.002f, d_flag);
    if (rc == PSM_OK) rc = th.meshClearance(&th, poses, p, 1e30f, d_pairs);   // a self-query
    return rc != PSM_OK ? rc : th.meshClearance(&other, poses, p, 0.5f, d_pairs);
}
int main() { return 0; }
