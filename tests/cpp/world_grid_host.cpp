#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
// The voxel grids of a world in the header layer (not in the reference) on a GPU: world_grid_host <in> <out>.
// <in>: int32 n; n x 9 float32 triangle positions (one hierarchy); int32 p; p x 16 float32 poses (glm::mat4, column-major: an
// instance of the hierarchy each); psm_grid (3 float32 origin, 3 float32 cell, 3 uint32 dims); uint32 samples.
// <out>: uint64 B, B surface words, B solid words; uint64 V, V uint32 counts, V int32 labels. tests/test_gpu_world_grid.py holds
// them to Python's.
#include <cstdio>
#include <vector>

static_assert(sizeof(psm_grid) == 36, "psm_grid: nine 4-byte numbers");

int main(int argc, char ** argv) {
    if (argc != 3) return 2;
    FILE * in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    int32_t n = 0, p = 0;
    psm_grid grid;
    uint32_t samples = 0;
    if (std::fread(&n, sizeof n, 1, in) != 1 || n <= 0) return 4;
    std::vector<float> pos((size_t)n * 9);
    if (std::fread(pos.data(), sizeof(float), pos.size(), in) != pos.size()) return 4;
    if (std::fread(&p, sizeof p, 1, in) != 1 || p <= 0) return 4;
    std::vector<float> m16((size_t)p * 16);
    if (std::fread(m16.data(), sizeof(float), m16.size(), in) != m16.size()) return 4;
    if (std::fread(&grid, sizeof grid, 1, in) != 1 || std::fread(&samples, sizeof samples, 1, in) != 1) return 4;
    std::fclose(in);

    psm::TriangleHierarchy th;
    th.allocate((size_t)n);
    th.loadTriangles(pos.data(), nullptr, nullptr, (size_t)n);
    th.build();
    psm::InstanceWorld world((uint32_t)p);
    for (int32_t k = 0; k < p; k++) {
        glm::mat4 m(1.0f);
        for (int col = 0; col < 4; col++)
            for (int row = 0; row < 4; row++) m[col][row] = m16[16 * (size_t)k + 4 * (size_t)col + (size_t)row];
        world.add(&th, m);
    }
    if (world.commit() != PSM_OK) return 5;
    std::vector<uint64_t> surface, solid, none;
    std::vector<uint32_t> counts;
    std::vector<int32_t> labels;
    if (world.voxelize(grid, surface) != PSM_OK || world.voxelizeSolid(grid, samples, solid) != PSM_OK) return 5;
    if (world.voxelCounts(grid, counts) != PSM_OK || world.voxelInstances(grid, labels) != PSM_OK) return 5;
    if (surface.size() != psm_grid_brick_count(&grid) || solid.size() != surface.size()) return 6;
    if (counts.size() != (size_t)grid.dims[0] * grid.dims[1] * grid.dims[2] || labels.size() != counts.size()) return 6;
    // a refusal leaves the vector empty and says why
    psm_grid bad = grid;
    bad.cell[1] = 0.0f;
    none.assign(3, 7u);
    if (world.voxelize(bad, none) != PSM_ERR_INVALID || !none.empty()) return 7;
    none.assign(3, 7u);
    if (world.voxelizeSolid(grid, 2u, none) != PSM_ERR_INVALID || !none.empty()) return 7;

    FILE * out = std::fopen(argv[2], "wb");
    if (!out) return 3;
    const uint64_t B = surface.size(), V = counts.size();
    std::fwrite(&B, sizeof B, 1, out);
    std::fwrite(surface.data(), sizeof(uint64_t), surface.size(), out);
    std::fwrite(solid.data(), sizeof(uint64_t), solid.size(), out);
    std::fwrite(&V, sizeof V, 1, out);
    std::fwrite(counts.data(), sizeof(uint32_t), counts.size(), out);
    std::fwrite(labels.data(), sizeof(int32_t), labels.size(), out);
    std::fclose(out);
    return 0;
}
