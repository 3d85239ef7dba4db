#pragma once
// Prismarine/QueryScene.hpp -- psm::QueryScene (not in the reference): TriangleHierarchy's seven queries over several
// hierarchies at once (psm_scene_*_dev, include/psm_hip.h "scene queries"): an ordered list of 1 .. PSM_SCENE_MAX_GEOMETRIES
// hierarchies, a candidate being (geom = index in the list, tri = that hierarchy's triangle id).

#include <vector>

#include "Utils.hpp"
#include "TriangleHierarchy.hpp"

namespace NSM {

    class QueryScene : public BaseClass {
    protected:
        std::vector<TriangleHierarchy *> geometries;   // not owned; their handles are read at every call (a rebuilt one is used as it then is)
        std::vector<psm_bvh *> handles() const;

    public:
        QueryScene() {}
        explicit QueryScene(const std::vector<TriangleHierarchy *> &hierarchies) : geometries(hierarchies) {}

        void clear() { geometries.clear(); }
        // returns the geometry's index in the scene (what d_geom reports)
        int32_t add(TriangleHierarchy * hierarchy) { geometries.push_back(hierarchy); return int32_t(geometries.size()) - 1; }
        size_t size() const { return geometries.size(); }

        // as the TriangleHierarchy methods of the same names, over the scene; stream-ordered on the context; return the psm_status.
        // d_geom[i]: the winning geometry's index, -1 on a miss
        int intersect(const psm_query_ray * d_rays, size_t n, psm_hit * d_hits, int32_t * d_geom);
        int occluded(const psm_query_ray * d_rays, size_t n, uint8_t * d_hit);
        int countHits(const psm_query_ray * d_rays, size_t n, uint32_t * d_count);
        int closestPoint(const psm_point_query * d_points, size_t n, psm_hit * d_hits, int32_t * d_geom);
        int within(const psm_point_query * d_points, size_t n, uint8_t * d_hit);
        int inside(const psm_point_query * d_points, size_t n, uint8_t * d_inside, uint32_t samples = 3);
        int signedDistance(const psm_point_query * d_points, size_t n, psm_hit * d_hits, int32_t * d_geom, uint32_t samples = 3);
    };
}
