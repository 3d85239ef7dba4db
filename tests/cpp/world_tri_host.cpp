#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
// compile-only: the triangle queries of an instance world in the header layer (not in the reference) against the C ABI's
// declarations (tests/test_world_tri_cpu.py); never run against a device
static_assert(PSM_QUERY_K_MAX == 16, "PSM_QUERY_K_MAX");
static_assert(sizeof(psm_tri_query) == 48, "psm_tri_query");
int triangles(psm::InstanceWorld & world, const psm_tri_query * d_tris, size_t n, uint8_t * d_hit, uint32_t * d_count, int32_t * d_tri,
              int32_t * d_inst) {
    int rc = world.overlapsTriangle(d_tris, n, d_hit);
    if (rc == PSM_OK) rc = world.countOnTriangle(d_tris, n, d_count);
    if (rc == PSM_OK) rc = world.trianglesOnTriangle(d_tris, n, 4, d_tri, d_inst, d_count);
    return rc != PSM_OK ? rc : world.trianglesOnTriangle(d_tris, n, PSM_QUERY_K_MAX, d_tri, d_inst, d_count);
}
int main() { return 0; }
