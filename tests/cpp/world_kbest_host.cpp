#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
// compile-only: the k-best queries of an instance world in the header layer (not in the reference) against the C ABI's
// declarations (tests/test_world_kbest_cpu.py); never run against a device
static_assert(PSM_QUERY_K_MAX == 16, "PSM_QUERY_K_MAX");
int lists(psm::InstanceWorld & world, const psm_query_ray * d_rays, const psm_point_query * d_points, size_t n, psm_hit * d_hits,
          int32_t * d_inst, uint32_t * d_count) {
    const int rc = world.firstHits(d_rays, n, 4, d_hits, d_inst, d_count);
    return rc != PSM_OK ? rc : world.nearest(d_points, n, PSM_QUERY_K_MAX, d_hits, d_inst, d_count);
}
int main() { return 0; }
