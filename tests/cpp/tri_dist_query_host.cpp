#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
#include <cstddef>
// compile-only: the clearance queries of the header layer (not in the reference) against the C ABI's declarations
static_assert(sizeof(psm_tri_dist_query) == 48, "psm_tri_dist_query: three 16-byte loads");
static_assert(offsetof(psm_tri_dist_query, rmax) == 12 && offsetof(psm_tri_dist_query, b) == 16 && offsetof(psm_tri_dist_query, c) == 32,
              "psm_tri_dist_query: psm_tri_query's layout with rmax where the first pad is");
static_assert(sizeof(psm_tri_hit) == 32, "psm_tri_hit: two 16-byte stores");
static_assert(offsetof(psm_tri_hit, dist) == offsetof(psm_hit, t) && offsetof(psm_tri_hit, tri) == offsetof(psm_hit, tri) && offsetof(psm_tri_hit, s) == 16,
              "psm_tri_hit: a psm_hit, then the query's weights");
int clearance(psm::TriangleHierarchy & th, const psm_tri_dist_query * d_queries, size_t n, psm_tri_hit * d_hits, uint8_t * d_flag) {
    const int rc = th.triClosest(d_queries, n, d_hits);
    return rc != PSM_OK ? rc : th.triWithin(d_queries, n, d_flag);
}
int main() { return 0; }
