#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
// compile-only: the box queries of an instance world in the header layer (not in the reference) against the C ABI's
// declarations (tests/test_world_box_cpu.py); never run against a device
static_assert(PSM_QUERY_K_MAX == 16, "PSM_QUERY_K_MAX");
static_assert(sizeof(psm_box_query) == 32, "psm_box_query");
int boxes(psm::InstanceWorld & world, const psm_box_query * d_boxes, size_t n, uint8_t * d_hit, uint32_t * d_count, int32_t * d_tri,
          int32_t * d_inst) {
    int rc = world.overlapsBox(d_boxes, n, d_hit);
    if (rc == PSM_OK) rc = world.countInBox(d_boxes, n, d_count);
    if (rc == PSM_OK) rc = world.trianglesInBox(d_boxes, n, 4, d_tri, d_inst, d_count);
    return rc != PSM_OK ? rc : world.trianglesInBox(d_boxes, n, PSM_QUERY_K_MAX, d_tri, d_inst, d_count);
}
int main() { return 0; }
