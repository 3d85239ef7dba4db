#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
// compile-only: the scene queries of the header layer (psm::QueryScene; not in the reference) against the C ABI's declarations
static_assert(PSM_SCENE_MAX_GEOMETRIES == 32, "the per-geometry table is 32 x four pointers = 1 KB of kernel arguments");
int all(psm::TriangleHierarchy & fixed, psm::TriangleHierarchy & moving, const psm_query_ray * d_rays, const psm_point_query * d_points,
        size_t n, psm_hit * d_hits, int32_t * d_geom, uint8_t * d_flag, uint32_t * d_count) {
    psm::QueryScene scene({&fixed});
    if (scene.add(&moving) != 1 || scene.size() != 2) return PSM_ERR_INVALID;
    int rc = scene.intersect(d_rays, n, d_hits, d_geom);
    if (rc == PSM_OK) rc = scene.occluded(d_rays, n, d_flag);
    if (rc == PSM_OK) rc = scene.countHits(d_rays, n, d_count);
    if (rc == PSM_OK) rc = scene.closestPoint(d_points, n, d_hits, d_geom);
    if (rc == PSM_OK) rc = scene.within(d_points, n, d_flag);
    if (rc == PSM_OK) rc = scene.inside(d_points, n, d_flag);
    if (rc == PSM_OK) rc = scene.inside(d_points, n, d_flag, 5);
    return rc != PSM_OK ? rc : scene.signedDistance(d_points, n, d_hits, d_geom, 1);
}
int main() { return 0; }
