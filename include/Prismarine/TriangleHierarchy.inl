#include "TriangleHierarchy.hpp"

// Implementation of psm::TriangleHierarchy over the C ABI. Replaces the GL orchestration of the
// reference's Include/Prismarine/TriangleHierarchy.inl (init :49-75, allocate :77-112, loadMesh
// :173-192, build :206-329): every stage runs in libpsm_hip.so on the context's stream.

namespace NSM {

    inline TriangleHierarchy::~TriangleHierarchy() {
        if (bvh) psm_bvh_destroy(bvh);
        delete sorter;
    }

    inline void TriangleHierarchy::init() {
        sorter = new RadixSort();
    }

    // allocate(count): the reference sizes every buffer for 2*count triangles (:78)
    inline void TriangleHierarchy::allocate(const size_t &count) {
        maxt = (uint32_t)(count * 2);
        if (bvh) { psm_bvh_destroy(bvh); bvh = nullptr; }
        check(psm_bvh_create(context(), maxt, &bvh), "TriangleHierarchy::allocate");
        clearTribuffer();
    }

    inline void TriangleHierarchy::setMaterialID(int32_t id) { materialID = id; }

    inline void TriangleHierarchy::clearTribuffer() {
        markDirty();
        if (bvh) check(psm_bvh_clear(bvh), "TriangleHierarchy::clearTribuffer");
        triangleCount = 0;
    }

    inline void TriangleHierarchy::refit() { if (bvh) { check(psm_bvh_refit(bvh), "TriangleHierarchy::refit"); this->resolve(); } }
    inline int TriangleHierarchy::intersect(const psm_query_ray * d_rays, size_t n, psm_hit * d_hits) {
        const int rc = psm_bvh_intersect_dev(bvh, d_rays, n, d_hits);
        check(rc, "TriangleHierarchy::intersect");
        return rc;
    }
    inline int TriangleHierarchy::occluded(const psm_query_ray * d_rays, size_t n, uint8_t * d_hit) {
        const int rc = psm_bvh_occluded_dev(bvh, d_rays, n, d_hit);
        check(rc, "TriangleHierarchy::occluded");
        return rc;
    }
    inline int TriangleHierarchy::closestPoint(const psm_point_query * d_points, size_t n, psm_hit * d_hits) {
        const int rc = psm_bvh_closest_point_dev(bvh, d_points, n, d_hits);
        check(rc, "TriangleHierarchy::closestPoint");
        return rc;
    }
    inline int TriangleHierarchy::within(const psm_point_query * d_points, size_t n, uint8_t * d_hit) {
        const int rc = psm_bvh_within_dev(bvh, d_points, n, d_hit);
        check(rc, "TriangleHierarchy::within");
        return rc;
    }
    inline int TriangleHierarchy::countHits(const psm_query_ray * d_rays, size_t n, uint32_t * d_count) {
        const int rc = psm_bvh_count_hits_dev(bvh, d_rays, n, d_count);
        check(rc, "TriangleHierarchy::countHits");
        return rc;
    }
    inline int TriangleHierarchy::inside(const psm_point_query * d_points, size_t n, uint8_t * d_inside, uint32_t samples) {
        const int rc = psm_bvh_inside_dev(bvh, d_points, n, samples, d_inside);
        check(rc, "TriangleHierarchy::inside");
        return rc;
    }
    inline int TriangleHierarchy::signedDistance(const psm_point_query * d_points, size_t n, psm_hit * d_hits, uint32_t samples) {
        const int rc = psm_bvh_signed_distance_dev(bvh, d_points, n, samples, d_hits);
        check(rc, "TriangleHierarchy::signedDistance");
        return rc;
    }
    inline int TriangleHierarchy::firstHits(const psm_query_ray * d_rays, size_t n, uint32_t k, psm_hit * d_hits, uint32_t * d_count) {
        const int rc = psm_bvh_first_hits_dev(bvh, d_rays, n, k, d_hits, d_count);
        check(rc, "TriangleHierarchy::firstHits");
        return rc;
    }
    inline int TriangleHierarchy::nearest(const psm_point_query * d_points, size_t n, uint32_t k, psm_hit * d_hits, uint32_t * d_count) {
        const int rc = psm_bvh_nearest_dev(bvh, d_points, n, k, d_hits, d_count);
        check(rc, "TriangleHierarchy::nearest");
        return rc;
    }
    inline int TriangleHierarchy::boxOverlaps(const psm_box_query * d_boxes, size_t n, uint8_t * d_hit) {
        const int rc = psm_bvh_box_overlaps_dev(bvh, d_boxes, n, d_hit);
        check(rc, "TriangleHierarchy::boxOverlaps");
        return rc;
    }
    inline int TriangleHierarchy::boxCount(const psm_box_query * d_boxes, size_t n, uint32_t * d_count) {
        const int rc = psm_bvh_box_count_dev(bvh, d_boxes, n, d_count);
        check(rc, "TriangleHierarchy::boxCount");
        return rc;
    }
    // one grid call into a device buffer of `count` words of T, read back into `out` (emptied first; left empty on a refusal)
    template<class T, class Call>
    inline int gridReadBack(size_t count, std::vector<T> & out, const char * what, Call call) {
        out.clear();
        if (count == 0) { check(PSM_ERR_INVALID, what); return PSM_ERR_INVALID; }   // (an invalid grid: no bricks)
        GLuint h = allocateBuffer<T>(count);
        void * d_out = nullptr;
        size_t bytes = 0;
        int rc = psm_buf_ptr(context(), h, &d_out, &bytes);
        if (rc == PSM_OK) rc = call((T *)d_out);
        check(rc, what);
        if (rc == PSM_OK) {
            out.resize(count);
            getBufferSubData(h, 0, strided<T>(count), out.data());
        }
        deleteBuffer(h);
        return rc;
    }
    inline int TriangleHierarchy::voxelize(const psm_grid & grid, std::vector<uint64_t> & bricks) {
        return gridReadBack<uint64_t>((size_t)psm_grid_brick_count(&grid), bricks, "TriangleHierarchy::voxelize",
                                      [&](uint64_t * d) { return psm_grid_surface_dev(bvh, &grid, d); });
    }
    inline int TriangleHierarchy::voxelizeSolid(const psm_grid & grid, uint32_t samples, std::vector<uint64_t> & bricks) {
        return gridReadBack<uint64_t>((size_t)psm_grid_brick_count(&grid), bricks, "TriangleHierarchy::voxelizeSolid",
                                      [&](uint64_t * d) { return psm_grid_solid_dev(bvh, &grid, samples, d); });
    }
    inline int TriangleHierarchy::voxelCounts(const psm_grid & grid, std::vector<uint32_t> & counts) {
        const size_t cells = psm_grid_brick_count(&grid) ? (size_t)grid.dims[0] * grid.dims[1] * grid.dims[2] : 0;
        return gridReadBack<uint32_t>(cells, counts, "TriangleHierarchy::voxelCounts",
                                      [&](uint32_t * d) { return psm_grid_counts_dev(bvh, &grid, d); });
    }
    // the distance fields of a hierarchy and of a world (InstanceWorld.inl): dist and, when asked for, tri and inst behind it in one
    // device buffer of 4-byte entries, read back and split (a hierarchy's call has no inst: NULL)
    template <class Call>
    inline int distanceReadBack(const psm_grid & grid, std::vector<float> & dist, std::vector<int32_t> * tri, std::vector<int32_t> * inst,
                                const char * what, Call call) {
        const size_t cells = psm_grid_brick_count(&grid) ? (size_t)grid.dims[0] * grid.dims[1] * grid.dims[2] : 0;
        if (tri) tri->clear();
        if (inst) inst->clear();
        const size_t tri_at = cells, inst_at = cells * (tri ? 2 : 1);
        std::vector<float> all;
        const int rc = gridReadBack<float>(cells * (1 + (tri ? 1 : 0) + (inst ? 1 : 0)), all, what, [&](float * d) {
            return call(d, tri ? (int32_t *)(d + tri_at) : nullptr, inst ? (int32_t *)(d + inst_at) : nullptr);
        });
        dist.clear();
        if (rc != PSM_OK) return rc;
        dist.assign(all.begin(), all.begin() + cells);
        if (tri) {
            tri->resize(cells);
            std::memcpy(tri->data(), all.data() + tri_at, cells * sizeof(int32_t));
        }
        if (inst) {
            inst->resize(cells);
            std::memcpy(inst->data(), all.data() + inst_at, cells * sizeof(int32_t));
        }
        return rc;
    }
    inline int TriangleHierarchy::distanceField(const psm_grid & grid, float rmax, std::vector<float> & dist, std::vector<int32_t> * tri) {
        return distanceReadBack(grid, dist, tri, nullptr, "TriangleHierarchy::distanceField",
                                [&](float * d, int32_t * t, int32_t *) { return psm_grid_distance_dev(bvh, &grid, rmax, d, t); });
    }
    inline int TriangleHierarchy::signedDistanceField(const psm_grid & grid, float rmax, uint32_t samples, std::vector<float> & dist,
                                                      std::vector<int32_t> * tri) {
        return distanceReadBack(grid, dist, tri, nullptr, "TriangleHierarchy::signedDistanceField",
                                [&](float * d, int32_t * t, int32_t *) { return psm_grid_signed_distance_dev(bvh, &grid, rmax, samples, d, t); });
    }
    // the sparse grids: the count is read back first (the one wait before the fill), then the list and `per` 4-byte entries of
    // answer a brick go into one device buffer -- the ids, the count, the answers from an even entry on -- read back and split
    template <class List, class Fill>
    inline int sparseReadBack(size_t per, std::vector<uint32_t> & ids, std::vector<uint32_t> & answers, const char * what, List list, Fill fill) {
        ids.clear();
        answers.clear();
        std::vector<uint32_t> all;
        int rc = gridReadBack<uint32_t>(4, all, what, [&](uint32_t * d) { return list(0u, (uint32_t *)nullptr, d); });
        if (rc != PSM_OK || all[0] == 0u) return rc;
        const uint32_t n = all[0];
        const size_t at = ((size_t)n + 2) & ~(size_t)1;
        rc = gridReadBack<uint32_t>(at + per * n, all, what, [&](uint32_t * d) {
            const int listed = list(n, d, d + n);
            return listed == PSM_OK ? fill(d, n, d + at) : listed;
        });
        if (rc != PSM_OK) return rc;
        ids.assign(all.begin(), all.begin() + n);
        answers.assign(all.begin() + at, all.end());
        return rc;
    }
    inline int sparseDistanceSplit(int rc, const std::vector<uint32_t> & answers, size_t n, std::vector<float> & dist, std::vector<int32_t> * tri) {
        dist.clear();
        if (tri) tri->clear();
        if (rc != PSM_OK) return rc;
        dist.resize(64 * n);
        std::memcpy(dist.data(), answers.data(), 64 * n * sizeof(float));
        if (tri) {
            tri->resize(64 * n);
            std::memcpy(tri->data(), answers.data() + 64 * n, 64 * n * sizeof(int32_t));
        }
        return rc;
    }
    inline int TriangleHierarchy::sparseVoxelize(const psm_grid & grid, std::vector<uint32_t> & ids, std::vector<uint64_t> & words) {
        std::vector<uint32_t> answers;
        words.clear();
        const int rc = sparseReadBack(2, ids, answers, "TriangleHierarchy::sparseVoxelize",
                                      [&](uint32_t capacity, uint32_t * d_ids, uint32_t * d_count) { return psm_grid_sparse_surface_bricks_dev(bvh, &grid, capacity, d_ids, d_count); },
                                      [&](const uint32_t * d_ids, uint32_t n, uint32_t * d) { return psm_grid_sparse_surface_dev(bvh, &grid, d_ids, n, (uint64_t *)d); });
        if (rc != PSM_OK) return rc;
        words.resize(ids.size());
        std::memcpy(words.data(), answers.data(), ids.size() * sizeof(uint64_t));
        return rc;
    }
    inline int TriangleHierarchy::sparseDistanceField(const psm_grid & grid, float rmax, std::vector<uint32_t> & ids, std::vector<float> & dist,
                                                      std::vector<int32_t> * tri) {
        std::vector<uint32_t> answers;
        const int rc = sparseReadBack(tri ? 128 : 64, ids, answers, "TriangleHierarchy::sparseDistanceField",
                                      [&](uint32_t capacity, uint32_t * d_ids, uint32_t * d_count) { return psm_grid_sparse_distance_bricks_dev(bvh, &grid, rmax, capacity, d_ids, d_count); },
                                      [&](const uint32_t * d_ids, uint32_t n, uint32_t * d) {
                                          return psm_grid_sparse_distance_dev(bvh, &grid, rmax, d_ids, n, (float *)d, tri ? (int32_t *)(d + (size_t)64 * n) : nullptr);
                                      });
        return sparseDistanceSplit(rc, answers, ids.size(), dist, tri);
    }
    inline int TriangleHierarchy::sparseSignedDistanceField(const psm_grid & grid, float rmax, uint32_t samples, std::vector<uint32_t> & ids,
                                                            std::vector<float> & dist, std::vector<int32_t> * tri) {
        std::vector<uint32_t> answers;
        const int rc = sparseReadBack(tri ? 128 : 64, ids, answers, "TriangleHierarchy::sparseSignedDistanceField",
                                      [&](uint32_t capacity, uint32_t * d_ids, uint32_t * d_count) { return psm_grid_sparse_distance_bricks_dev(bvh, &grid, rmax, capacity, d_ids, d_count); },
                                      [&](const uint32_t * d_ids, uint32_t n, uint32_t * d) {
                                          return psm_grid_sparse_signed_distance_dev(bvh, &grid, rmax, samples, d_ids, n, (float *)d, tri ? (int32_t *)(d + (size_t)64 * n) : nullptr);
                                      });
        return sparseDistanceSplit(rc, answers, ids.size(), dist, tri);
    }
    inline int TriangleHierarchy::boxTriangles(const psm_box_query * d_boxes, size_t n, uint32_t k, int32_t * d_tris, uint32_t * d_count) {
        const int rc = psm_bvh_box_triangles_dev(bvh, d_boxes, n, k, d_tris, d_count);
        check(rc, "TriangleHierarchy::boxTriangles");
        return rc;
    }
    inline int TriangleHierarchy::triOverlaps(const psm_tri_query * d_tris, size_t n, uint8_t * d_hit) {
        const int rc = psm_bvh_tri_overlaps_dev(bvh, d_tris, n, d_hit);
        check(rc, "TriangleHierarchy::triOverlaps");
        return rc;
    }
    inline int TriangleHierarchy::triCount(const psm_tri_query * d_tris, size_t n, uint32_t * d_count) {
        const int rc = psm_bvh_tri_count_dev(bvh, d_tris, n, d_count);
        check(rc, "TriangleHierarchy::triCount");
        return rc;
    }
    inline int TriangleHierarchy::triTriangles(const psm_tri_query * d_tris, size_t n, uint32_t k, int32_t * d_ids, uint32_t * d_count) {
        const int rc = psm_bvh_tri_triangles_dev(bvh, d_tris, n, k, d_ids, d_count);
        check(rc, "TriangleHierarchy::triTriangles");
        return rc;
    }
    inline int TriangleHierarchy::triClosest(const psm_tri_dist_query * d_queries, size_t n, psm_tri_hit * d_hits) {
        const int rc = psm_bvh_tri_closest_dev(bvh, d_queries, n, d_hits);
        check(rc, "TriangleHierarchy::triClosest");
        return rc;
    }
    inline int TriangleHierarchy::triWithin(const psm_tri_dist_query * d_queries, size_t n, uint8_t * d_flag) {
        const int rc = psm_bvh_tri_within_dev(bvh, d_queries, n, d_flag);
        check(rc, "TriangleHierarchy::triWithin");
        return rc;
    }
    namespace detail {
    // psm_hip.h wants row-major 3 x 4 [R | T] matrices: m12[4 * row + col] = m[col][row], glm's last row dropped
    inline std::vector<float> meshPoses(const glm::mat4 * m, size_t p) {
        std::vector<float> m12(12 * p);
        for (size_t q = 0; q < p; q++)
            for (int row = 0; row < 3; row++)
                for (int col = 0; col < 4; col++) m12[12 * q + 4 * row + col] = m[q][col][row];
        return m12;
    }
    }
    inline int TriangleHierarchy::meshOverlaps(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, uint8_t * d_hit) {
        const std::vector<float> m12 = detail::meshPoses(poses, p);
        const int rc = psm_bvh_mesh_overlaps_dev(bvh, other ? other->bvh : nullptr, m12.data(), p, d_hit);
        check(rc, "TriangleHierarchy::meshOverlaps");
        return rc;
    }
    inline int TriangleHierarchy::meshCount(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, uint32_t * d_count) {
        const std::vector<float> m12 = detail::meshPoses(poses, p);
        const int rc = psm_bvh_mesh_count_dev(bvh, other ? other->bvh : nullptr, m12.data(), p, d_count);
        check(rc, "TriangleHierarchy::meshCount");
        return rc;
    }
    inline int TriangleHierarchy::meshTriangles(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, uint32_t k, int32_t * d_ids, uint32_t * d_count) {
        const std::vector<float> m12 = detail::meshPoses(poses, p);
        const int rc = psm_bvh_mesh_triangles_dev(bvh, other ? other->bvh : nullptr, m12.data(), p, k, d_ids, d_count);
        check(rc, "TriangleHierarchy::meshTriangles");
        return rc;
    }
    inline int TriangleHierarchy::meshClosest(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, float rmax, psm_tri_hit * d_hits) {
        const std::vector<float> m12 = detail::meshPoses(poses, p);
        const int rc = psm_bvh_mesh_closest_dev(bvh, other ? other->bvh : nullptr, m12.data(), p, rmax, d_hits);
        check(rc, "TriangleHierarchy::meshClosest");
        return rc;
    }
    inline int TriangleHierarchy::meshWithin(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, float r, uint8_t * d_flag) {
        const std::vector<float> m12 = detail::meshPoses(poses, p);
        const int rc = psm_bvh_mesh_within_dev(bvh, other ? other->bvh : nullptr, m12.data(), p, r, d_flag);
        check(rc, "TriangleHierarchy::meshWithin");
        return rc;
    }
    inline int TriangleHierarchy::meshClearance(TriangleHierarchy * other, const glm::mat4 * poses, size_t p, float rmax, psm_mesh_hit * d_hits) {
        const std::vector<float> m12 = detail::meshPoses(poses, p);
        const int rc = psm_bvh_mesh_clearance_dev(bvh, other ? other->bvh : nullptr, m12.data(), p, rmax, d_hits);
        check(rc, "TriangleHierarchy::meshClearance");
        return rc;
    }
    inline int TriangleHierarchy::sweepSphere(const psm_sweep_query * d_sweeps, size_t n, psm_hit * d_hits) {
        const int rc = psm_bvh_sweep_sphere_dev(bvh, d_sweeps, n, d_hits);
        check(rc, "TriangleHierarchy::sweepSphere");
        return rc;
    }
    inline int TriangleHierarchy::sweepOccluded(const psm_sweep_query * d_sweeps, size_t n, uint8_t * d_hit) {
        const int rc = psm_bvh_sweep_occluded_dev(bvh, d_sweeps, n, d_hit);
        check(rc, "TriangleHierarchy::sweepOccluded");
        return rc;
    }
    inline void TriangleHierarchy::setBuildGraph(bool enable) { if (bvh) check(psm_bvh_set_build_graph(bvh, enable ? 1 : 0), "TriangleHierarchy::setBuildGraph"); }
    inline void TriangleHierarchy::configureIntersection(bool clearDepth) { (void)clearDepth; }  // ignored by the reference's shaders too

    inline void TriangleHierarchy::loadTriangles(const float * positions, const float * normals, const int32_t * materials, size_t count, const float * texcoords) {
        if (!bvh || count == 0) return;
        int rc = psm_bvh_load_triangles(bvh, positions, normals, materials, count, materialID);
        check(rc, "TriangleHierarchy::loadTriangles");
        if (rc == PSM_OK && texcoords) check(psm_bvh_set_texcoords(bvh, triangleCount, texcoords, count), "TriangleHierarchy::loadTriangles(texcoords)");
        if (rc == PSM_OK) triangleCount += count;
        markDirty();
    }

    // loadMesh(gobject), TriangleHierarchy.inl:173-192: the accessor / buffer-view description is resolved by
    // the HIP gather kernel behind psm_bvh_load_mesh (vertex/loader.comp:32-152); no host round trip.
    inline void TriangleHierarchy::loadMesh(TriangleArrayInstance * gobject) {
        if (!gobject || gobject->meshUniformData.nodeCount <= 0 || !bvh) return;
        if (!gobject->accessorSet || !gobject->bufferViewSet) return;
        const MeshUniformStruct & mu = gobject->meshUniformData;
        psm_mesh_desc d;
        std::memset(&d, 0, sizeof(d));
        void * vptr = nullptr; size_t vbytes = 0, ibytes = 0;
        if (gobject->vbo_triangle_ssbo == GLuint(-1) || psm_buf_ptr(context(), gobject->vbo_triangle_ssbo, &vptr, &vbytes) != PSM_OK) return;
        d.d_vertices = (const float *)vptr; d.vertex_floats = vbytes / 4;
        if (mu.isIndexed && gobject->vebo_triangle_ssbo != GLuint(-1)) {
            void * iptr = nullptr;
            if (psm_buf_ptr(context(), gobject->vebo_triangle_ssbo, &iptr, &ibytes) == PSM_OK) { d.d_indices = (const uint32_t *)iptr; d.index_words = ibytes / 4; }
        }
        std::vector<psm_accessor> acc;
        for (const VirtualAccessor & a : gobject->accessorSet->data) acc.push_back(psm_accessor{a.offset4, (int32_t)(a.components & 3), a.bufferView});
        std::vector<psm_buffer_view> views;
        for (const VirtualBufferView & v : gobject->bufferViewSet->data) views.push_back(psm_buffer_view{v.offset4, v.stride4});
        d.accessors = acc.data(); d.accessor_count = (uint32_t)acc.size();
        d.views = views.data(); d.view_count = (uint32_t)views.size();
        d.vertex_accessor = mu.vertexAccessor; d.normal_accessor = mu.normalAccessor;
        d.texcoord_accessor = mu.texcoordAccessor; d.modifier_accessor = mu.modifierAccessor;
        glm::mat4 T = gobject->hasTransform ? gobject->transform : glm::mat4(1.0f);
        glm::mat4 Ti = glm::inverse(T);
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { d.transform[4 * r + c] = T[c][r]; d.transform_inv[4 * r + c] = Ti[c][r]; }
        d.material_id = mu.materialID; d.is_indexed = mu.isIndexed; d.index16 = gobject->index16bit ? 1 : 0;
        d.node_count = mu.nodeCount; d.primitive_type = mu.primitiveType; d.loading_offset = mu.loadingOffset;
        int rc = psm_bvh_load_mesh(bvh, &d);
        check(rc, "TriangleHierarchy::loadMesh");
        if (rc == PSM_OK) triangleCount += (size_t)mu.nodeCount * (mu.primitiveType == 1 ? 2 : 1);
        markDirty();
    }

    inline bool TriangleHierarchy::isDirty() const { return dirty; }
    inline void TriangleHierarchy::markDirty() { dirty = true; }
    inline void TriangleHierarchy::resolve() { dirty = false; }

    // build(optimization), TriangleHierarchy.inl:206-329
    inline void TriangleHierarchy::build(const glm::dmat4 &optimization) {
        if (this->triangleCount <= 0 || !dirty || !bvh) return;   // :214
        double opt[16];
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) opt[4 * r + c] = optimization[c][r];  // glm is column-major
        check(psm_bvh_build(bvh, opt), "TriangleHierarchy::build");
        this->resolve();
    }
}
