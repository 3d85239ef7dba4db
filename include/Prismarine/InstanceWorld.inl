// Prismarine/InstanceWorld.inl -- implementation of psm::InstanceWorld over the C ABI (psm_world_*): thin checked wrappers.
#include "InstanceWorld.hpp"

namespace NSM {

    inline int InstanceWorld::commit() {
        const std::vector<psm_instance> v = instances();
        const int rc = v.size() != geometries.size() ? int(PSM_ERR_INVALID) : psm_world_set_instances(world, v.data(), uint32_t(v.size()));
        check(rc, "InstanceWorld::commit");
        return rc;
    }
    inline int InstanceWorld::setTransforms(size_t first, const glm::mat4 * m, size_t count) {
        std::vector<float> m12(12 * count);
        for (size_t k = 0; k < count; k++) {
            if (m[k][0][3] != 0.0f || m[k][1][3] != 0.0f || m[k][2][3] != 0.0f || m[k][3][3] != 1.0f) return int(PSM_ERR_INVALID);
            for (int row = 0; row < 3; row++)
                for (int col = 0; col < 4; col++) m12[12 * k + 4 * row + col] = m[k][col][row];
        }
        const int rc = psm_world_set_transforms(world, uint32_t(first), uint32_t(count), m12.data());
        check(rc, "InstanceWorld::setTransforms");
        for (size_t k = 0; rc == PSM_OK && k < count; k++) poses.at(first + k) = m[k];
        return rc;
    }
    inline int InstanceWorld::intersect(const psm_query_ray * d_rays, size_t n, psm_hit * d_hits, int32_t * d_inst) {
        const int rc = psm_world_intersect_dev(world, d_rays, n, d_hits, d_inst);
        check(rc, "InstanceWorld::intersect");
        return rc;
    }
    inline int InstanceWorld::occluded(const psm_query_ray * d_rays, size_t n, uint8_t * d_hit) {
        const int rc = psm_world_occluded_dev(world, d_rays, n, d_hit);
        check(rc, "InstanceWorld::occluded");
        return rc;
    }
    inline int InstanceWorld::countHits(const psm_query_ray * d_rays, size_t n, uint32_t * d_count) {
        const int rc = psm_world_count_hits_dev(world, d_rays, n, d_count);
        check(rc, "InstanceWorld::countHits");
        return rc;
    }
    inline int InstanceWorld::closestPoint(const psm_point_query * d_points, size_t n, psm_hit * d_hits, int32_t * d_inst) {
        const int rc = psm_world_closest_point_dev(world, d_points, n, d_hits, d_inst);
        check(rc, "InstanceWorld::closestPoint");
        return rc;
    }
    inline int InstanceWorld::within(const psm_point_query * d_points, size_t n, uint8_t * d_hit) {
        const int rc = psm_world_within_dev(world, d_points, n, d_hit);
        check(rc, "InstanceWorld::within");
        return rc;
    }
    inline int InstanceWorld::inside(const psm_point_query * d_points, size_t n, uint8_t * d_inside, uint32_t samples) {
        const int rc = psm_world_inside_dev(world, d_points, n, samples, d_inside);
        check(rc, "InstanceWorld::inside");
        return rc;
    }
    inline int InstanceWorld::signedDistance(const psm_point_query * d_points, size_t n, psm_hit * d_hits, int32_t * d_inst, uint32_t samples) {
        const int rc = psm_world_signed_distance_dev(world, d_points, n, samples, d_hits, d_inst);
        check(rc, "InstanceWorld::signedDistance");
        return rc;
    }
    inline int InstanceWorld::firstHits(const psm_query_ray * d_rays, size_t n, uint32_t k, psm_hit * d_hits, int32_t * d_inst, uint32_t * d_count) {
        const int rc = psm_world_first_hits_dev(world, d_rays, n, k, d_hits, d_inst, d_count);
        check(rc, "InstanceWorld::firstHits");
        return rc;
    }
    inline int InstanceWorld::nearest(const psm_point_query * d_points, size_t n, uint32_t k, psm_hit * d_hits, int32_t * d_inst, uint32_t * d_count) {
        const int rc = psm_world_nearest_dev(world, d_points, n, k, d_hits, d_inst, d_count);
        check(rc, "InstanceWorld::nearest");
        return rc;
    }
    inline int InstanceWorld::overlapsBox(const psm_box_query * d_boxes, size_t n, uint8_t * d_hit) {
        const int rc = psm_world_box_overlaps_dev(world, d_boxes, n, d_hit);
        check(rc, "InstanceWorld::overlapsBox");
        return rc;
    }
    inline int InstanceWorld::countInBox(const psm_box_query * d_boxes, size_t n, uint32_t * d_count) {
        const int rc = psm_world_box_count_dev(world, d_boxes, n, d_count);
        check(rc, "InstanceWorld::countInBox");
        return rc;
    }
    inline int InstanceWorld::trianglesInBox(const psm_box_query * d_boxes, size_t n, uint32_t k, int32_t * d_tri, int32_t * d_inst, uint32_t * d_count) {
        const int rc = psm_world_box_triangles_dev(world, d_boxes, n, k, d_tri, d_inst, d_count);
        check(rc, "InstanceWorld::trianglesInBox");
        return rc;
    }
    inline int InstanceWorld::sphereCast(const psm_sweep_query * d_sweeps, size_t n, psm_hit * d_hits, int32_t * d_inst) {
        const int rc = psm_world_sweep_sphere_dev(world, d_sweeps, n, d_hits, d_inst);
        check(rc, "InstanceWorld::sphereCast");
        return rc;
    }
    inline int InstanceWorld::sphereCastOccluded(const psm_sweep_query * d_sweeps, size_t n, uint8_t * d_hit) {
        const int rc = psm_world_sweep_occluded_dev(world, d_sweeps, n, d_hit);
        check(rc, "InstanceWorld::sphereCastOccluded");
        return rc;
    }
    inline int InstanceWorld::overlapsTriangle(const psm_tri_query * d_tris, size_t n, uint8_t * d_hit) {
        const int rc = psm_world_tri_overlaps_dev(world, d_tris, n, d_hit);
        check(rc, "InstanceWorld::overlapsTriangle");
        return rc;
    }
    inline int InstanceWorld::countOnTriangle(const psm_tri_query * d_tris, size_t n, uint32_t * d_count) {
        const int rc = psm_world_tri_count_dev(world, d_tris, n, d_count);
        check(rc, "InstanceWorld::countOnTriangle");
        return rc;
    }
    inline int InstanceWorld::trianglesOnTriangle(const psm_tri_query * d_tris, size_t n, uint32_t k, int32_t * d_tri, int32_t * d_inst, uint32_t * d_count) {
        const int rc = psm_world_tri_triangles_dev(world, d_tris, n, k, d_tri, d_inst, d_count);
        check(rc, "InstanceWorld::trianglesOnTriangle");
        return rc;
    }
    inline int InstanceWorld::closestToTriangle(const psm_tri_dist_query * d_tris, size_t n, psm_tri_hit * d_hits, int32_t * d_inst) {
        const int rc = psm_world_tri_closest_dev(world, d_tris, n, d_hits, d_inst);
        check(rc, "InstanceWorld::closestToTriangle");
        return rc;
    }
    inline int InstanceWorld::withinOfTriangle(const psm_tri_dist_query * d_tris, size_t n, uint8_t * d_hit) {
        const int rc = psm_world_tri_within_dev(world, d_tris, n, d_hit);
        check(rc, "InstanceWorld::withinOfTriangle");
        return rc;
    }
    inline int InstanceWorld::overlapsMesh(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, int skip, uint8_t * d_hit) {
        const std::vector<float> m12 = detail::meshPoses(poses, p);   // (TriangleHierarchy.inl)
        const int rc = psm_world_mesh_overlaps_dev(world, other ? other->handle() : nullptr, m12.data(), p, int32_t(skip), d_hit);
        check(rc, "InstanceWorld::overlapsMesh");
        return rc;
    }
    inline int InstanceWorld::countOnMesh(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, int skip, uint32_t * d_count) {
        const std::vector<float> m12 = detail::meshPoses(poses, p);
        const int rc = psm_world_mesh_count_dev(world, other ? other->handle() : nullptr, m12.data(), p, int32_t(skip), d_count);
        check(rc, "InstanceWorld::countOnMesh");
        return rc;
    }
    inline int InstanceWorld::trianglesOnMesh(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, int skip, uint32_t k, int32_t * d_tri, int32_t * d_inst, uint32_t * d_count) {
        const std::vector<float> m12 = detail::meshPoses(poses, p);
        const int rc = psm_world_mesh_triangles_dev(world, other ? other->handle() : nullptr, m12.data(), p, int32_t(skip), k, d_tri, d_inst, d_count);
        check(rc, "InstanceWorld::trianglesOnMesh");
        return rc;
    }
    inline int InstanceWorld::closestToMesh(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, int skip, float rmax, psm_tri_hit * d_hits, int32_t * d_inst) {
        const std::vector<float> m12 = detail::meshPoses(poses, p);
        const int rc = psm_world_mesh_closest_dev(world, other ? other->handle() : nullptr, m12.data(), p, int32_t(skip), rmax, d_hits, d_inst);
        check(rc, "InstanceWorld::closestToMesh");
        return rc;
    }
    inline int InstanceWorld::withinOfMesh(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, int skip, float r, uint8_t * d_flag) {
        const std::vector<float> m12 = detail::meshPoses(poses, p);
        const int rc = psm_world_mesh_within_dev(world, other ? other->handle() : nullptr, m12.data(), p, int32_t(skip), r, d_flag);
        check(rc, "InstanceWorld::withinOfMesh");
        return rc;
    }
    inline int InstanceWorld::clearanceToMesh(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, int skip, float rmax, psm_mesh_hit * d_hits, int32_t * d_inst) {
        const std::vector<float> m12 = detail::meshPoses(poses, p);
        const int rc = psm_world_mesh_clearance_dev(world, other ? other->handle() : nullptr, m12.data(), p, int32_t(skip), rmax, d_hits, d_inst);
        check(rc, "InstanceWorld::clearanceToMesh");
        return rc;
    }
    // (gridReadBack: TriangleHierarchy.inl -- one call into a device buffer, read back into the vector)
    inline int InstanceWorld::voxelize(const psm_grid & grid, std::vector<uint64_t> & bricks) {
        return gridReadBack<uint64_t>((size_t)psm_grid_brick_count(&grid), bricks, "InstanceWorld::voxelize",
                                      [&](uint64_t * d) { return psm_grid_world_surface_dev(world, &grid, d); });
    }
    inline int InstanceWorld::voxelizeSolid(const psm_grid & grid, uint32_t samples, std::vector<uint64_t> & bricks) {
        return gridReadBack<uint64_t>((size_t)psm_grid_brick_count(&grid), bricks, "InstanceWorld::voxelizeSolid",
                                      [&](uint64_t * d) { return psm_grid_world_solid_dev(world, &grid, samples, d); });
    }
    inline int InstanceWorld::voxelCounts(const psm_grid & grid, std::vector<uint32_t> & counts) {
        const size_t cells = psm_grid_brick_count(&grid) ? (size_t)grid.dims[0] * grid.dims[1] * grid.dims[2] : 0;
        return gridReadBack<uint32_t>(cells, counts, "InstanceWorld::voxelCounts",
                                      [&](uint32_t * d) { return psm_grid_world_counts_dev(world, &grid, d); });
    }
    inline int InstanceWorld::voxelInstances(const psm_grid & grid, std::vector<int32_t> & labels) {
        const size_t cells = psm_grid_brick_count(&grid) ? (size_t)grid.dims[0] * grid.dims[1] * grid.dims[2] : 0;
        return gridReadBack<int32_t>(cells, labels, "InstanceWorld::voxelInstances",
                                     [&](int32_t * d) { return psm_grid_world_instances_dev(world, &grid, d); });
    }
    // (distanceReadBack: TriangleHierarchy.inl -- dist, tri and inst in one device buffer, read back and split)
    inline int InstanceWorld::distanceField(const psm_grid & grid, float rmax, std::vector<float> & dist, std::vector<int32_t> * tri,
                                            std::vector<int32_t> * inst) {
        return distanceReadBack(grid, dist, tri, inst, "InstanceWorld::distanceField",
                                [&](float * d, int32_t * t, int32_t * i) { return psm_grid_world_distance_dev(world, &grid, rmax, d, t, i); });
    }
    inline int InstanceWorld::signedDistanceField(const psm_grid & grid, float rmax, uint32_t samples, std::vector<float> & dist,
                                                  std::vector<int32_t> * tri, std::vector<int32_t> * inst) {
        return distanceReadBack(grid, dist, tri, inst, "InstanceWorld::signedDistanceField", [&](float * d, int32_t * t, int32_t * i) {
            return psm_grid_world_signed_distance_dev(world, &grid, rmax, samples, d, t, i);
        });
    }
}
