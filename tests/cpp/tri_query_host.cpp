#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
#include <cstddef>
// compile-only: the triangle queries of the header layer (not in the reference) against the C ABI's declarations
static_assert(PSM_QUERY_K_MAX == 16, "PSM_QUERY_K_MAX");
static_assert(sizeof(psm_tri_query) == 48, "psm_tri_query: three 16-byte loads");
static_assert(offsetof(psm_tri_query, b) == 16 && offsetof(psm_tri_query, c) == 32, "psm_tri_query: a vertex per float4");
int triangles(psm::TriangleHierarchy & th, const psm_tri_query * d_tris, size_t n, uint8_t * d_hit, int32_t * d_ids, uint32_t * d_count) {
    int rc = th.triOverlaps(d_tris, n, d_hit);
    if (rc == PSM_OK) rc = th.triCount(d_tris, n, d_count);
    return rc != PSM_OK ? rc : th.triTriangles(d_tris, n, PSM_QUERY_K_MAX, d_ids, d_count);
}
int main() { return 0; }
