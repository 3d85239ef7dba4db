#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
// compile-only: the sphere sweeps of an instance world in the header layer (not in the reference) against the C ABI's
// declarations (tests/test_world_sweep_cpu.py); never run against a device
static_assert(sizeof(psm_sweep_query) == 32, "psm_sweep_query");
static_assert(sizeof(psm_hit) == 16, "psm_hit");
int sweeps(psm::InstanceWorld & world, const psm_sweep_query * d_sweeps, size_t n, psm_hit * d_hits, int32_t * d_inst, uint8_t * d_hit) {
    const int rc = world.sphereCast(d_sweeps, n, d_hits, d_inst);
    return rc != PSM_OK ? rc : world.sphereCastOccluded(d_sweeps, n, d_hit);
}
int main() { return 0; }
