#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
// compile-only: the hit-count, inside and signed-distance queries of the header layer (not in the reference) against the C ABI's
// declarations, and the direction table as the header writes it
static const float directions[PSM_INSIDE_MAX_SAMPLES][3] = PSM_INSIDE_DIRECTIONS;
static_assert(sizeof(directions) == 5 * 3 * sizeof(float), "PSM_INSIDE_DIRECTIONS: five rows of three floats");
int field(psm::TriangleHierarchy & th, const psm_query_ray * d_rays, const psm_point_query * d_points, size_t n, uint32_t * d_count,
          uint8_t * d_inside, psm_hit * d_hits) {
    int rc = th.countHits(d_rays, n, d_count);
    if (rc == PSM_OK) rc = th.inside(d_points, n, d_inside);
    if (rc == PSM_OK) rc = th.inside(d_points, n, d_inside, 5);
    return rc != PSM_OK ? rc : th.signedDistance(d_points, n, d_hits, 1);
}
int main() { return directions[0][0] > 0.f ? 0 : 1; }
