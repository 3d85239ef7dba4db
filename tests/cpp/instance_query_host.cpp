#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
// the instanced scene queries of the header layer (psm::InstancedScene; not in the reference) against the C ABI's
// declarations (compile and link only: all()), the layout the kernels' table is sized by, and -- run, no device needed -- the copy
// of a glm::mat4 into psm_instance's row-major 3 x 4 (main())
static_assert(sizeof(psm_instance) == sizeof(void *) + 12 * sizeof(float), "psm_instance: a handle and a row-major 3 x 4 matrix");
static_assert(PSM_SCENE_MAX_GEOMETRIES * (4 * sizeof(void *) + 12 * sizeof(float)) == 2560, "the instance table: 2560 B of kernel arguments");
int all(psm::TriangleHierarchy & fixed, psm::TriangleHierarchy & moving, const psm_query_ray * d_rays, const psm_point_query * d_points,
        size_t n, psm_hit * d_hits, int32_t * d_inst, uint8_t * d_flag, uint32_t * d_count) {
    psm::InstancedScene scene;
    if (scene.add(&fixed) != 0 || scene.add(&moving, glm::translate(glm::vec3(1.0f, 2.0f, 3.0f))) != 1 || scene.size() != 2) return PSM_ERR_INVALID;
    scene.setTransform(1, glm::translate(glm::vec3(0.0f, 0.5f, 0.0f)));   // the same hierarchy twice, at two poses
    if (scene.add(&moving, scene.transform(0)) != 2) return PSM_ERR_INVALID;
    int rc = scene.intersect(d_rays, n, d_hits, d_inst);
    if (rc == PSM_OK) rc = scene.occluded(d_rays, n, d_flag);
    if (rc == PSM_OK) rc = scene.countHits(d_rays, n, d_count);
    if (rc == PSM_OK) rc = scene.closestPoint(d_points, n, d_hits, d_inst);
    if (rc == PSM_OK) rc = scene.within(d_points, n, d_flag);
    if (rc == PSM_OK) rc = scene.inside(d_points, n, d_flag);
    if (rc == PSM_OK) rc = scene.inside(d_points, n, d_flag, 5);
    if (rc == PSM_OK) rc = scene.signedDistance(d_points, n, d_hits, d_inst, 1);
    scene.clear();
    return rc;
}
// 0 when the poses arrive as [R | T] row by row; otherwise the number of the check that failed
int main() {
    psm::InstancedScene scene;
    scene.add(nullptr, glm::translate(glm::vec3(1.0f, 2.0f, 3.0f)));
    glm::mat4 turn(1.0f);                    // a quarter turn about z: x -> y, y -> -x (columns are the images of the axes), then T
    turn[0] = glm::vec4(0.0f, 1.0f, 0.0f, 0.0f);
    turn[1] = glm::vec4(-1.0f, 0.0f, 0.0f, 0.0f);
    turn[3] = glm::vec4(5.0f, 6.0f, 7.0f, 1.0f);
    scene.add(nullptr, turn);
    const std::vector<psm_instance> v = scene.instances();
    if (v.size() != 2 || v[0].bvh != nullptr) return 1;
    const float shift[12] = {1, 0, 0, 1, 0, 1, 0, 2, 0, 0, 1, 3};
    const float quarter[12] = {0, -1, 0, 5, 1, 0, 0, 6, 0, 0, 1, 7};
    for (int k = 0; k < 12; k++) {
        if (v[0].world_from_object[k] != shift[k]) return 2;
        if (v[1].world_from_object[k] != quarter[k]) return 3;
    }
    // world = R * object + T with these 12 floats is glm's m * (object, 1)
    const float * m = v[1].world_from_object;
    for (int row = 0; row < 3; row++) {
        const float w = turn[0][row] * 1.0f + turn[1][row] * 2.0f + turn[2][row] * 3.0f + turn[3][row];   // (m * (1, 2, 3, 1)).row
        if (m[4 * row] * 1.0f + m[4 * row + 1] * 2.0f + m[4 * row + 2] * 3.0f + m[4 * row + 3] != w) return 4;
    }
    glm::mat4 bad(1.0f);
    bad[1][3] = 0.5f;                        // a last row that is not 0 0 0 1: no list
    scene.setTransform(0, bad);
    if (!scene.instances().empty()) return 5;   // (every query method then returns PSM_ERR_INVALID through check())
    return 0;
}
