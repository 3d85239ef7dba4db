#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
// compile-only: the sphere sweeps of the header layer (not in the reference) against the C ABI's declarations
static_assert(sizeof(psm_sweep_query) == 32, "psm_sweep_query: two 16-byte loads, where a query ray's are");
static_assert(sizeof(psm_sweep_query) == sizeof(psm_query_ray), "psm_sweep_query travels where psm_query_ray does");
int sweeps(psm::TriangleHierarchy & th, const psm_sweep_query * d_sweeps, size_t n, psm_hit * d_hits, uint8_t * d_hit) {
    const int rc = th.sweepSphere(d_sweeps, n, d_hits);
    return rc != PSM_OK ? rc : th.sweepOccluded(d_sweeps, n, d_hit);
}
int main() { return 0; }
