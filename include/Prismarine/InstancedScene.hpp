#pragma once
// Prismarine/InstancedScene.hpp -- psm::InstancedScene (not in the reference): QueryScene's seven queries over instances, a
// built hierarchy and a rigid pose each (psm_instances_*_dev, include/psm_hip.h "instanced scene queries"). Moving a body is
// setTransform(): nothing is rebuilt, the next call reads the new matrix; one hierarchy may stand at many poses.
// The pose is a glm::mat4 in glm's convention, as everywhere in these headers: column-major m[col][row], world = m * object, the
// translation in column 3. psm_instance wants the row-major 3 x 4 [R | T]: world_from_object[4 * row + col] = m[col][row], a
// transposed copy of the upper three rows (no arithmetic). The last row must be 0 0 0 1 and R rigid; the library refuses others.

#include <vector>

#include "Utils.hpp"
#include "TriangleHierarchy.hpp"

namespace NSM {

    class InstancedScene : public BaseClass {
    protected:
        std::vector<TriangleHierarchy *> geometries;   // not owned; their handles are read at every call
        std::vector<glm::mat4> poses;

    public:
        InstancedScene() {}

        // the list as the C ABI takes it (what every call passes); empty when a pose's last row is not 0 0 0 1
        std::vector<psm_instance> instances() const;

        void clear() { geometries.clear(); poses.clear(); }
        // returns the instance's index in the scene (what d_inst reports)
        int32_t add(TriangleHierarchy * hierarchy, const glm::mat4 &worldFromObject = glm::mat4(1.0f)) {
            geometries.push_back(hierarchy);
            poses.push_back(worldFromObject);
            return int32_t(geometries.size()) - 1;
        }
        void setTransform(size_t i, const glm::mat4 &worldFromObject) { poses.at(i) = worldFromObject; }
        const glm::mat4 &transform(size_t i) const { return poses.at(i); }
        size_t size() const { return geometries.size(); }

        // as the QueryScene methods of the same names; psm_hit holds the winning instance's object-space values, d_inst[i] its
        // index (-1 on a miss). A pose whose last row is not 0 0 0 1 is refused here with PSM_ERR_INVALID, before the library is called
        int intersect(const psm_query_ray * d_rays, size_t n, psm_hit * d_hits, int32_t * d_inst);
        int occluded(const psm_query_ray * d_rays, size_t n, uint8_t * d_hit);
        int countHits(const psm_query_ray * d_rays, size_t n, uint32_t * d_count);
        int closestPoint(const psm_point_query * d_points, size_t n, psm_hit * d_hits, int32_t * d_inst);
        int within(const psm_point_query * d_points, size_t n, uint8_t * d_hit);
        int inside(const psm_point_query * d_points, size_t n, uint8_t * d_inside, uint32_t samples = 3);
        int signedDistance(const psm_point_query * d_points, size_t n, psm_hit * d_hits, int32_t * d_inst, uint32_t samples = 3);
    };
}
