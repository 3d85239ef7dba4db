#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
// compile-only: the ray queries of the header layer (not in the reference) against the C ABI's declarations
static_assert(sizeof(psm_query_ray) == 32, "psm_query_ray: two 16-byte loads");
static_assert(sizeof(psm_hit) == 16, "psm_hit: one 16-byte store");
int trace(psm::TriangleHierarchy & th, const psm_query_ray * d_rays, size_t n, psm_hit * d_hits, uint8_t * d_shadow) {
    const int rc = th.intersect(d_rays, n, d_hits);
    return rc != PSM_OK ? rc : th.occluded(d_rays, n, d_shadow);
}
int main() { return 0; }
