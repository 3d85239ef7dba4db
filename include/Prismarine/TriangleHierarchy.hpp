#pragma once
// Prismarine/TriangleHierarchy.hpp -- psm::TriangleHierarchy, same public surface as the reference
// (Include/Prismarine/TriangleHierarchy.hpp:75-94): geometry store + HLBVH build.

#include "Utils.hpp"
#include "VertexInstance.hpp"
#include "Radix.hpp"

namespace NSM {

    class TriangleHierarchy : public BaseClass {
    protected:
        friend class Pipeline;
        RadixSort * sorter = nullptr;
        bool dirty = false;
        uint32_t maxt = 1024 * 128 * 1;
        psm_bvh * bvh = nullptr;
        void init();

    public:
        TriangleHierarchy() { init(); }
        ~TriangleHierarchy();

        int32_t materialID = 0;
        size_t triangleCount = 0;

        void syncUniforms() {}
        void allocate(const size_t &count);
        void setMaterialID(int32_t id);
        void bindUniforms() {}
        void bind() {}
        void bindBVH() {}
        void bindLeafs() {}
        void clearTribuffer();
        void loadMesh(TriangleArrayInstance * gobject);
        // direct ingestion of a world-space triangle soup (9 floats per triangle; normals / material ids optional)
        void loadTriangles(const float * positions, const float * normals, const int32_t * materials, size_t count, const float * texcoords = nullptr);
        bool isDirty() const;
        void markDirty();
        void resolve();
        void build(const glm::dmat4 &optimization = glm::dmat4(1.0));
        void configureIntersection(bool clearDepth);
        void refit();                     // not in the reference: boxes only, for triangles reloaded in place; the tree is the last build's
        void setBuildGraph(bool enable);  // not in the reference: replay rebuilds as one captured hipGraph (default on)
        // not in the reference: closest hit / any hit of n rays over device arrays (psm_bvh_intersect_dev / psm_bvh_occluded_dev),
        // stream-ordered on the context; returns the psm_status
        int intersect(const psm_query_ray * d_rays, size_t n, psm_hit * d_hits);
        int occluded(const psm_query_ray * d_rays, size_t n, uint8_t * d_hit);
        // not in the reference: closest point within rmax / any triangle within rmax of n points over device arrays
        // (psm_bvh_closest_point_dev / psm_bvh_within_dev), stream-ordered on the context; returns the psm_status
        int closestPoint(const psm_point_query * d_points, size_t n, psm_hit * d_hits);
        int within(const psm_point_query * d_points, size_t n, uint8_t * d_hit);
        // not in the reference: crossings of n rays inside their windows / inside-outside of n points by the parity vote of
        // `samples` (1, 3 or 5) rays / closest point with the sign bit of t set inside (psm_bvh_count_hits_dev / psm_bvh_inside_dev
        // / psm_bvh_signed_distance_dev), stream-ordered on the context; returns the psm_status
        int countHits(const psm_query_ray * d_rays, size_t n, uint32_t * d_count);
        int inside(const psm_point_query * d_points, size_t n, uint8_t * d_inside, uint32_t samples = 3);
        int signedDistance(const psm_point_query * d_points, size_t n, psm_hit * d_hits, uint32_t samples = 3);
        // not in the reference: the first k hits of n rays in the order (t, tri) / the k nearest triangles of n points in the order
        // (d2, tri), 1 <= k <= PSM_QUERY_K_MAX: d_hits [n][k] records, d_count [n] = the slots of a row that hold one, the rest
        // are misses (psm_bvh_first_hits_dev / psm_bvh_nearest_dev), stream-ordered on the context; returns the psm_status
        int firstHits(const psm_query_ray * d_rays, size_t n, uint32_t k, psm_hit * d_hits, uint32_t * d_count);
        int nearest(const psm_point_query * d_points, size_t n, uint32_t k, psm_hit * d_hits, uint32_t * d_count);
        // not in the reference: whether / how many / which triangles overlap each of n axis-aligned boxes (closed: touching counts);
        // boxTriangles: 1 <= k <= PSM_QUERY_K_MAX, d_tris [n][k] = the lowest ids that count, ascending, then -1, d_count [n] = the
        // slots that hold one (psm_bvh_box_overlaps_dev / psm_bvh_box_count_dev / psm_bvh_box_triangles_dev), stream-ordered on
        // the context; returns the psm_status
        int boxOverlaps(const psm_box_query * d_boxes, size_t n, uint8_t * d_hit);
        int boxCount(const psm_box_query * d_boxes, size_t n, uint32_t * d_count);
        int boxTriangles(const psm_box_query * d_boxes, size_t n, uint32_t k, int32_t * d_tris, uint32_t * d_count);
        // not in the reference: the voxels of a regular grid that a triangle overlaps, as one 64-bit word per 4 x 4 x 4 brick (bit
        // (z & 3) * 16 + (y & 3) * 4 + (x & 3) of brick (bz * nby + by) * nbx + bx), the same with the inside of a closed mesh
        // filled by the vote of `samples` (1, 3 or 5) rays from each voxel's centre, and the number of triangles per voxel, dense
        // [nz][ny][nx]; each voxel answered as boxOverlaps / boxCount answer its box (psm_hip.h "voxel grids"; psm_grid_surface_dev
        // / psm_grid_solid_dev / psm_grid_counts_dev). The result is read back into the vector (the call waits for it; a refused
        // call leaves the vector empty); returns the psm_status
        int voxelize(const psm_grid & grid, std::vector<uint64_t> & bricks);
        int voxelizeSolid(const psm_grid & grid, uint32_t samples, std::vector<uint64_t> & bricks);
        int voxelCounts(const psm_grid & grid, std::vector<uint32_t> & counts);
        // not in the reference: the distance from every voxel centre of a regular grid to the nearest triangle within rmax (>= 0
        // or +inf; +inf in the field where there is none), dense [nz][ny][nx], and with tri the nearest triangle's id (-1 where
        // there is none); signed: with the sign of the vote of `samples` (1, 3 or 5) rays from the centre. Each voxel answered as
        // closestPoint / signedDistance answer its centre (psm_hip.h "voxel grids: distance fields"; psm_grid_distance_dev /
        // psm_grid_signed_distance_dev). Read back into the vectors as voxelize does; returns the psm_status
        int distanceField(const psm_grid & grid, float rmax, std::vector<float> & dist, std::vector<int32_t> * tri = nullptr);
        int signedDistanceField(const psm_grid & grid, float rmax, uint32_t samples, std::vector<float> & dist, std::vector<int32_t> * tri = nullptr);
        // not in the reference: the same for the non-empty 4 x 4 x 4 bricks alone (psm_hip.h "voxel grids: sparse"): ids = the
        // ascending brick indices (bz * nby + by) * nbx + bx whose surface word is non-zero (sparseVoxelize) or that hold a voxel
        // centre within rmax of a triangle (the two distance forms), words [n] = voxelize's words of those bricks, dist / tri
        // [n][64] = distanceField's / signedDistanceField's answers of their voxels in lane order (z & 3) * 16 + (y & 3) * 4 +
        // (x & 3), +inf / -1 for a voxel outside dims. Each lists (the count is read back: one wait), fills and reads back into
        // the vectors (a refused call leaves them empty); returns the psm_status
        int sparseVoxelize(const psm_grid & grid, std::vector<uint32_t> & ids, std::vector<uint64_t> & words);
        int sparseDistanceField(const psm_grid & grid, float rmax, std::vector<uint32_t> & ids, std::vector<float> & dist, std::vector<int32_t> * tri = nullptr);
        int sparseSignedDistanceField(const psm_grid & grid, float rmax, uint32_t samples, std::vector<uint32_t> & ids, std::vector<float> & dist,
                                      std::vector<int32_t> * tri = nullptr);
        // not in the reference: whether / how many / which triangles meet each of n query triangles (closed: touching counts; a
        // separating-axis test in float32, psm_hip.h "triangle queries"); triTriangles: 1 <= k <= PSM_QUERY_K_MAX, d_ids [n][k] =
        // the lowest ids that count, ascending, then -1, d_count [n] = the slots that hold one (psm_bvh_tri_overlaps_dev /
        // psm_bvh_tri_count_dev / psm_bvh_tri_triangles_dev), stream-ordered on the context; returns the psm_status
        int triOverlaps(const psm_tri_query * d_tris, size_t n, uint8_t * d_hit);
        int triCount(const psm_tri_query * d_tris, size_t n, uint32_t * d_count);
        int triTriangles(const psm_tri_query * d_tris, size_t n, uint32_t k, int32_t * d_ids, uint32_t * d_count);
        // not in the reference: the nearest triangle to each of n query triangles within its rmax -- d_hits [n] = {u, v, dist, tri,
        // s, t, 0, 0}, (u, v) on the stored triangle and (s, t) on the query's, a miss {0, 0, +inf, -1, 0, 0, 0, 0} -- and whether
        // any is within it, d_flag [n] (fifteen vertex-face and edge-edge features in float32, 0 where the triangles meet; psm_hip.h
        // "clearance queries"; psm_bvh_tri_closest_dev / psm_bvh_tri_within_dev), stream-ordered on the context; returns the
        // psm_status
        int triClosest(const psm_tri_dist_query * d_queries, size_t n, psm_tri_hit * d_hits);
        int triWithin(const psm_tri_dist_query * d_queries, size_t n, uint8_t * d_flag);
        // not in the reference: whether / how many / which triangles meet each stored triangle of another built hierarchy `other`
        // (of the same context) at each of p rigid poses (glm's convention, as InstancedScene's: a point of other's object space
        // goes to m * x in this hierarchy's), posed in float32 on the device and answered as triOverlaps / triCount / triTriangles
        // answer it (psm_hip.h "mesh queries"). With T = other->triangleCount: d_hit [p], d_count [p][T], d_ids [p][T][k],
        // 1 <= k <= PSM_QUERY_K_MAX, indexed by other's load-order triangle id (psm_bvh_mesh_overlaps_dev / psm_bvh_mesh_count_dev
        // / psm_bvh_mesh_triangles_dev). The poses are host memory read at the call, which waits once for their upload; the
        // kernel is stream-ordered on the context; returns the psm_status
        int meshOverlaps(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, uint8_t * d_hit);
        int meshCount(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, uint32_t * d_count);
        int meshTriangles(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, uint32_t k, int32_t * d_ids, uint32_t * d_count);
        // not in the reference: how close `other` comes at each of p poses (poses, T and indexing as meshCount) -- meshClosest:
        // d_hits [p][T], the record triClosest writes for each posed triangle of other under the one rmax; meshClearance: d_hits
        // [p], the one nearest pair of each pose {u, v, dist, tri, s, t, other, 0}: the smallest dist, on an equal dist the
        // lowest triangle of other, a miss {0, 0, +inf, -1, 0, 0, -1, 0}; meshWithin: d_flag [p], whether any pair is within r
        // (psm_hip.h "mesh clearance"; psm_bvh_mesh_closest_dev / psm_bvh_mesh_within_dev / psm_bvh_mesh_clearance_dev). The
        // call waits once for its pose upload; the kernels are stream-ordered on the context; returns the psm_status
        int meshClosest(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, float rmax, psm_tri_hit * d_hits);
        int meshWithin(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, float r, uint8_t * d_flag);
        int meshClearance(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, float rmax, psm_mesh_hit * d_hits);
        // not in the reference: where a sphere that moves along a line first touches the triangles (t = the distance its centre
        // travels, 0 when it touches where it starts; a miss is {0, 0, +inf, -1}), and whether it touches any within tmax
        // (psm_bvh_sweep_sphere_dev / psm_bvh_sweep_occluded_dev), stream-ordered on the context; returns the psm_status
        int sweepSphere(const psm_sweep_query * d_sweeps, size_t n, psm_hit * d_hits);
        int sweepOccluded(const psm_sweep_query * d_sweeps, size_t n, uint8_t * d_hit);
        psm_bvh * handle() { return bvh; }
    };
}
