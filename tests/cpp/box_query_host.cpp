#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
// compile-only: the box queries of the header layer (not in the reference) against the C ABI's declarations
static_assert(PSM_QUERY_K_MAX == 16, "PSM_QUERY_K_MAX");
static_assert(sizeof(psm_box_query) == 32, "psm_box_query: two 16-byte loads");
int boxes(psm::TriangleHierarchy & th, const psm_box_query * d_boxes, size_t n, uint8_t * d_hit, int32_t * d_tris, uint32_t * d_count) {
    int rc = th.boxOverlaps(d_boxes, n, d_hit);
    if (rc == PSM_OK) rc = th.boxCount(d_boxes, n, d_count);
    return rc != PSM_OK ? rc : th.boxTriangles(d_boxes, n, PSM_QUERY_K_MAX, d_tris, d_count);
}
int main() { return 0; }
