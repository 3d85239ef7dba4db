// Prismarine/QueryScene.inl -- implementation of psm::QueryScene over the C ABI (psm_scene_*_dev): thin checked wrappers, as
// TriangleHierarchy's queries are.
#include "QueryScene.hpp"

namespace NSM {

    inline std::vector<psm_bvh *> QueryScene::handles() const {
        std::vector<psm_bvh *> h(geometries.size());
        for (size_t g = 0; g < geometries.size(); g++) h[g] = geometries[g] ? geometries[g]->handle() : nullptr;
        return h;
    }
    inline int QueryScene::intersect(const psm_query_ray * d_rays, size_t n, psm_hit * d_hits, int32_t * d_geom) {
        const std::vector<psm_bvh *> h = handles();
        const int rc = psm_scene_intersect_dev(h.data(), uint32_t(h.size()), d_rays, n, d_hits, d_geom);
        check(rc, "QueryScene::intersect");
        return rc;
    }
    inline int QueryScene::occluded(const psm_query_ray * d_rays, size_t n, uint8_t * d_hit) {
        const std::vector<psm_bvh *> h = handles();
        const int rc = psm_scene_occluded_dev(h.data(), uint32_t(h.size()), d_rays, n, d_hit);
        check(rc, "QueryScene::occluded");
        return rc;
    }
    inline int QueryScene::countHits(const psm_query_ray * d_rays, size_t n, uint32_t * d_count) {
        const std::vector<psm_bvh *> h = handles();
        const int rc = psm_scene_count_hits_dev(h.data(), uint32_t(h.size()), d_rays, n, d_count);
        check(rc, "QueryScene::countHits");
        return rc;
    }
    inline int QueryScene::closestPoint(const psm_point_query * d_points, size_t n, psm_hit * d_hits, int32_t * d_geom) {
        const std::vector<psm_bvh *> h = handles();
        const int rc = psm_scene_closest_point_dev(h.data(), uint32_t(h.size()), d_points, n, d_hits, d_geom);
        check(rc, "QueryScene::closestPoint");
        return rc;
    }
    inline int QueryScene::within(const psm_point_query * d_points, size_t n, uint8_t * d_hit) {
        const std::vector<psm_bvh *> h = handles();
        const int rc = psm_scene_within_dev(h.data(), uint32_t(h.size()), d_points, n, d_hit);
        check(rc, "QueryScene::within");
        return rc;
    }
    inline int QueryScene::inside(const psm_point_query * d_points, size_t n, uint8_t * d_inside, uint32_t samples) {
        const std::vector<psm_bvh *> h = handles();
        const int rc = psm_scene_inside_dev(h.data(), uint32_t(h.size()), d_points, n, samples, d_inside);
        check(rc, "QueryScene::inside");
        return rc;
    }
    inline int QueryScene::signedDistance(const psm_point_query * d_points, size_t n, psm_hit * d_hits, int32_t * d_geom, uint32_t samples) {
        const std::vector<psm_bvh *> h = handles();
        const int rc = psm_scene_signed_distance_dev(h.data(), uint32_t(h.size()), d_points, n, samples, d_hits, d_geom);
        check(rc, "QueryScene::signedDistance");
        return rc;
    }
}
