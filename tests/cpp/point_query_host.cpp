#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
// compile-only: the point queries of the header layer (not in the reference) against the C ABI's declarations
static_assert(sizeof(psm_point_query) == 16, "psm_point_query: one 16-byte load");
static_assert(sizeof(psm_hit) == 16, "psm_hit: one 16-byte store");
int nearest(psm::TriangleHierarchy & th, const psm_point_query * d_points, size_t n, psm_hit * d_hits, uint8_t * d_near) {
    const int rc = th.closestPoint(d_points, n, d_hits);
    return rc != PSM_OK ? rc : th.within(d_points, n, d_near);
}
int main() { return 0; }
