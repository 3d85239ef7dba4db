#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
#include <cstddef>
// compile-only: the mesh queries of the header layer (not in the reference) against the C ABI's declarations
static_assert(PSM_QUERY_K_MAX == 16, "PSM_QUERY_K_MAX");
int meshes(psm::TriangleHierarchy & th, psm::TriangleHierarchy & other, const glm::mat4 * poses, size_t p, uint8_t * d_hit, int32_t * d_ids,
           uint32_t * d_count) {
    int rc = th.meshOverlaps(&other, poses, p, d_hit);
    if (rc == PSM_OK) rc = th.meshCount(&other, poses, p, d_count);
    if (rc == PSM_OK) rc = th.meshCount(&th, poses, p, d_count);   // a self-query
    return rc != PSM_OK ? rc : th.meshTriangles(&other, poses, p, PSM_QUERY_K_MAX, d_ids, d_count);
}
int main() { return 0; }
