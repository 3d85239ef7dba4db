// Prismarine/InstancedScene.inl -- implementation of psm::InstancedScene over the C ABI (psm_instances_*_dev): thin checked
// wrappers, as QueryScene's are.
#include "InstancedScene.hpp"

namespace NSM {

    // the list as the C ABI takes it; empty when a pose's last row is not 0 0 0 1 (the calls then refuse)
    inline std::vector<psm_instance> InstancedScene::instances() const {
        std::vector<psm_instance> v(geometries.size());
        for (size_t g = 0; g < geometries.size(); g++) {
            const glm::mat4 &m = poses[g];
            if (m[0][3] != 0.0f || m[1][3] != 0.0f || m[2][3] != 0.0f || m[3][3] != 1.0f) return std::vector<psm_instance>();
            v[g].bvh = geometries[g] ? geometries[g]->handle() : nullptr;
            for (int row = 0; row < 3; row++)
                for (int col = 0; col < 4; col++) v[g].world_from_object[4 * row + col] = m[col][row];
        }
        return v;
    }
    inline int InstancedScene::intersect(const psm_query_ray * d_rays, size_t n, psm_hit * d_hits, int32_t * d_inst) {
        const std::vector<psm_instance> v = instances();
        const int rc = v.size() != geometries.size() ? int(PSM_ERR_INVALID) : psm_instances_intersect_dev(v.data(), uint32_t(v.size()), d_rays, n, d_hits, d_inst);
        check(rc, "InstancedScene::intersect");
        return rc;
    }
    inline int InstancedScene::occluded(const psm_query_ray * d_rays, size_t n, uint8_t * d_hit) {
        const std::vector<psm_instance> v = instances();
        const int rc = v.size() != geometries.size() ? int(PSM_ERR_INVALID) : psm_instances_occluded_dev(v.data(), uint32_t(v.size()), d_rays, n, d_hit);
        check(rc, "InstancedScene::occluded");
        return rc;
    }
    inline int InstancedScene::countHits(const psm_query_ray * d_rays, size_t n, uint32_t * d_count) {
        const std::vector<psm_instance> v = instances();
        const int rc = v.size() != geometries.size() ? int(PSM_ERR_INVALID) : psm_instances_count_hits_dev(v.data(), uint32_t(v.size()), d_rays, n, d_count);
        check(rc, "InstancedScene::countHits");
        return rc;
    }
    inline int InstancedScene::closestPoint(const psm_point_query * d_points, size_t n, psm_hit * d_hits, int32_t * d_inst) {
        const std::vector<psm_instance> v = instances();
        const int rc = v.size() != geometries.size() ? int(PSM_ERR_INVALID) : psm_instances_closest_point_dev(v.data(), uint32_t(v.size()), d_points, n, d_hits, d_inst);
        check(rc, "InstancedScene::closestPoint");
        return rc;
    }
    inline int InstancedScene::within(const psm_point_query * d_points, size_t n, uint8_t * d_hit) {
        const std::vector<psm_instance> v = instances();
        const int rc = v.size() != geometries.size() ? int(PSM_ERR_INVALID) : psm_instances_within_dev(v.data(), uint32_t(v.size()), d_points, n, d_hit);
        check(rc, "InstancedScene::within");
        return rc;
    }
    inline int InstancedScene::inside(const psm_point_query * d_points, size_t n, uint8_t * d_inside, uint32_t samples) {
        const std::vector<psm_instance> v = instances();
        const int rc = v.size() != geometries.size() ? int(PSM_ERR_INVALID) : psm_instances_inside_dev(v.data(), uint32_t(v.size()), d_points, n, samples, d_inside);
        check(rc, "InstancedScene::inside");
        return rc;
    }
    inline int InstancedScene::signedDistance(const psm_point_query * d_points, size_t n, psm_hit * d_hits, int32_t * d_inst, uint32_t samples) {
        const std::vector<psm_instance> v = instances();
        const int rc = v.size() != geometries.size() ? int(PSM_ERR_INVALID) : psm_instances_signed_distance_dev(v.data(), uint32_t(v.size()), d_points, n, samples, d_hits, d_inst);
        check(rc, "InstancedScene::signedDistance");
        return rc;
    }
}
