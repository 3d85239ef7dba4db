#pragma once
// Prismarine/InstanceWorld.hpp -- psm::InstanceWorld (not in the reference): InstancedScene's seven queries over up to
// PSM_WORLD_MAX_INSTANCES instances under a top-level tree on the device (psm_world_*, include/psm_hip.h "instance worlds").
// A query enters only the instances it can reach; the answers are those of an InstancedScene over the same list. The list is
// uploaded by commit(); setTransform() moves bodies without rebuilding a hierarchy. Poses are glm::mat4 as in InstancedScene.

#include "InstancedScene.hpp"

namespace NSM {

    class InstanceWorld : public InstancedScene {
    protected:
        psm_world * world = nullptr;

    public:
        explicit InstanceWorld(uint32_t capacity = PSM_WORLD_MAX_INSTANCES) { world = psm_world_create(context(), capacity); }
        ~InstanceWorld() { if (world) psm_world_destroy(world); }
        InstanceWorld(const InstanceWorld &) = delete;
        InstanceWorld & operator=(const InstanceWorld &) = delete;
        psm_world * handle() const { return world; }

        // upload the list built with add() / clear(): table, boxes and tree (psm_world_set_instances)
        int commit();
        // place instances first .. first + count - 1 anew, on the host list and on the device (psm_world_set_transforms)
        int setTransforms(size_t first, const glm::mat4 * worldFromObject, size_t count);
        int setTransform(size_t i, const glm::mat4 &worldFromObject) { return setTransforms(i, &worldFromObject, 1); }
        // after a member hierarchy was refitted: boxes and tree from the triangles as they now are
        int refresh() { return poses.empty() ? int(PSM_OK) : setTransforms(0, poses.data(), poses.size()); }
        uint32_t count() const { return psm_world_count(world); }

        int intersect(const psm_query_ray * d_rays, size_t n, psm_hit * d_hits, int32_t * d_inst);
        int occluded(const psm_query_ray * d_rays, size_t n, uint8_t * d_hit);
        int countHits(const psm_query_ray * d_rays, size_t n, uint32_t * d_count);
        int closestPoint(const psm_point_query * d_points, size_t n, psm_hit * d_hits, int32_t * d_inst);
        int within(const psm_point_query * d_points, size_t n, uint8_t * d_hit);
        int inside(const psm_point_query * d_points, size_t n, uint8_t * d_inside, uint32_t samples = 3);
        int signedDistance(const psm_point_query * d_points, size_t n, psm_hit * d_hits, int32_t * d_inst, uint32_t samples = 3);
        // the first k hits of n rays in the order (t, inst, tri) / the k nearest triangles of n points in the order (d2, inst, tri)
        // over the whole world, 1 <= k <= PSM_QUERY_K_MAX: d_hits and d_inst [n][k], d_count [n] = the slots filled, the rest are
        // misses with inst = -1 (psm_world_first_hits_dev / psm_world_nearest_dev); the flat lists have no such query
        int firstHits(const psm_query_ray * d_rays, size_t n, uint32_t k, psm_hit * d_hits, int32_t * d_inst, uint32_t * d_count);
        int nearest(const psm_point_query * d_points, size_t n, uint32_t k, psm_hit * d_hits, int32_t * d_inst, uint32_t * d_count);
        // whether / how many / which (instance, triangle) pairs overlap each of n axis-aligned WORLD boxes (closed: touching
        // counts): the box is never moved, each candidate triangle is posed forward and judged by the single hierarchy's box test;
        // trianglesInBox: 1 <= k <= PSM_QUERY_K_MAX, d_tri and d_inst [n][k] = the lowest (inst, tri) that count, ascending, then
        // -1 in both, d_count [n] = the slots filled (psm_world_box_overlaps_dev / psm_world_box_count_dev /
        // psm_world_box_triangles_dev); the flat lists have no such query
        int overlapsBox(const psm_box_query * d_boxes, size_t n, uint8_t * d_hit);
        int countInBox(const psm_box_query * d_boxes, size_t n, uint32_t * d_count);
        int trianglesInBox(const psm_box_query * d_boxes, size_t n, uint32_t k, int32_t * d_tri, int32_t * d_inst, uint32_t * d_count);
        // where a sphere that moves along each of n WORLD lines first touches a triangle of a posed instance (d_hits: the winning
        // instance's object-space {u, v, t, tri}, d_inst its index, -1 on a miss; the smallest t, on a bit-equal t the lowest
        // (inst, tri)), and whether it touches one (psm_world_sweep_sphere_dev / psm_world_sweep_occluded_dev): the sweep is
        // moved into each instance as a ray is and judged by the single hierarchy's sweep test; the flat lists have no such query
        int sphereCast(const psm_sweep_query * d_sweeps, size_t n, psm_hit * d_hits, int32_t * d_inst);
        int sphereCastOccluded(const psm_sweep_query * d_sweeps, size_t n, uint8_t * d_hit);
        // whether / how many / which (instance, triangle) pairs meet each of n WORLD triangles (closed: touching counts): the query
        // triangle is never moved, each candidate triangle is posed forward and judged by the single hierarchy's triangle test;
        // trianglesOnTriangle: 1 <= k <= PSM_QUERY_K_MAX, d_tri and d_inst [n][k] = the lowest (inst, tri) that count, ascending,
        // then -1 in both, d_count [n] = the slots filled (psm_world_tri_overlaps_dev / psm_world_tri_count_dev /
        // psm_world_tri_triangles_dev); the flat lists have no such query
        int overlapsTriangle(const psm_tri_query * d_tris, size_t n, uint8_t * d_hit);
        int countOnTriangle(const psm_tri_query * d_tris, size_t n, uint32_t * d_count);
        int trianglesOnTriangle(const psm_tri_query * d_tris, size_t n, uint32_t k, int32_t * d_tri, int32_t * d_inst, uint32_t * d_count);
        // which (instance, triangle) pair is nearest to each of n WORLD triangles within its rmax, how far and at which two points
        // (d_hits: {u, v, dist, tri, s, t, 0, 0}, (u, v) weights of the stored = the posed triangle's edges, (s, t) of the
        // query's; d_inst the instance, -1 on a miss; the smallest float32 d2, on a bit-equal d2 the lowest (inst, tri)), and
        // whether any pair is within it: the query triangle is never moved, each candidate triangle is posed forward and judged
        // by the single hierarchy's clearance test, so dist == 0 exactly where overlapsTriangle counts the pair
        // (psm_world_tri_closest_dev / psm_world_tri_within_dev); the flat lists have no such query
        int closestToTriangle(const psm_tri_dist_query * d_tris, size_t n, psm_tri_hit * d_hits, int32_t * d_inst);
        int withinOfTriangle(const psm_tri_dist_query * d_tris, size_t n, uint8_t * d_hit);
        // whether / how many / which (instance, triangle) pairs meet each stored triangle of ANOTHER built hierarchy at each of p
        // rigid poses that take its object space into WORLD space (glm::mat4, last row 0 0 0 1), in one call: each query triangle
        // is posed on the device and answered bit for bit as the three queries above answer it. skip: an instance that is left
        // out (the other indices kept), -1 for none. d_hit [p]; d_count [p][T], T other's loaded triangle count; trianglesOnMesh:
        // d_tri and d_inst [p][T][k], d_count [p][T]. The poses are host memory read at the call, which waits once for their
        // upload and cannot be captured into a graph (psm_world_mesh_overlaps_dev / psm_world_mesh_count_dev /
        // psm_world_mesh_triangles_dev); the flat lists have no such query
        int overlapsMesh(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, int skip, uint8_t * d_hit);
        int countOnMesh(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, int skip, uint32_t * d_count);
        int trianglesOnMesh(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, int skip, uint32_t k, int32_t * d_tri, int32_t * d_inst, uint32_t * d_count);
        // how close each stored triangle of ANOTHER built hierarchy comes to the world's (instance, triangle) pairs at each of p
        // rigid poses within rmax (closestToMesh: d_hits [p][T] psm_tri_hit, d_inst [p][T], each bit for bit closestToTriangle's
        // answer for the posed triangle), whether any comes within r (withinOfMesh: d_flag [p]) and the ONE nearest pair of each
        // pose (clearanceToMesh: d_hits [p] psm_mesh_hit, d_inst [p]: the smallest dist, then the lowest triangle of other, then
        // closestToTriangle's (inst, tri)). poses, skip, the one wait and no graph capture as overlapsMesh
        // (psm_world_mesh_closest_dev / psm_world_mesh_within_dev / psm_world_mesh_clearance_dev)
        int closestToMesh(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, int skip, float rmax, psm_tri_hit * d_hits, int32_t * d_inst);
        int withinOfMesh(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, int skip, float r, uint8_t * d_flag);
        int clearanceToMesh(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, int skip, float rmax, psm_mesh_hit * d_hits, int32_t * d_inst);
        // the voxels of a regular WORLD grid that a posed triangle of some instance overlaps (one 64-bit word per 4 x 4 x 4 brick,
        // TriangleHierarchy::voxelize's layout), the same with the inside filled by the vote of `samples` (1, 3 or 5) rays of
        // inside() from each voxel's centre, the number of (instance, triangle) pairs per voxel and the lowest instance that has a
        // triangle in it (-1: none), both dense [nz][ny][nx]; each voxel answered as overlapsBox / countInBox / trianglesInBox(k =
        // 1) answer its box (psm_hip.h "voxel grids over a world"; psm_grid_world_surface_dev / psm_grid_world_solid_dev /
        // psm_grid_world_counts_dev / psm_grid_world_instances_dev). The result is read back into the vector (the call waits for
        // it; a refused call leaves the vector empty); the flat lists have no grids
        int voxelize(const psm_grid & grid, std::vector<uint64_t> & bricks);
        int voxelizeSolid(const psm_grid & grid, uint32_t samples, std::vector<uint64_t> & bricks);
        int voxelCounts(const psm_grid & grid, std::vector<uint32_t> & counts);
        int voxelInstances(const psm_grid & grid, std::vector<int32_t> & labels);
        // the distance from every voxel centre of a regular WORLD grid to the nearest posed triangle of any instance within rmax
        // (+inf: none), that triangle's id and its instance (-1: none; on a bit-equal squared distance the lowest (instance,
        // triangle)), and the same with the sign of inside(centre, samples); dense [nz][ny][nx], each voxel as
        // closestPoint / signedDistance answer its centre (psm_hip.h "voxel grids over a world: distance fields";
        // psm_grid_world_distance_dev / psm_grid_world_signed_distance_dev). tri, inst: NULL when not wanted. Read back as
        // TriangleHierarchy::distanceField's; a refused call leaves the vectors empty
        int distanceField(const psm_grid & grid, float rmax, std::vector<float> & dist, std::vector<int32_t> * tri = nullptr,
                          std::vector<int32_t> * inst = nullptr);
        int signedDistanceField(const psm_grid & grid, float rmax, uint32_t samples, std::vector<float> & dist, std::vector<int32_t> * tri = nullptr,
                                std::vector<int32_t> * inst = nullptr);
    };
}
