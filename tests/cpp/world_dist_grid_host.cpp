#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
// The distance fields of a world in the header layer (not in the reference) on a GPU: world_dist_grid_host <in> <out>.
// <in>: int32 n; n x 9 float32 triangle positions (one hierarchy); int32 p; p x 16 float32 poses (glm::mat4, column-major: an
// instance of the hierarchy each); psm_grid (3 float32 origin, 3 float32 cell, 3 uint32 dims); float32 rmax; uint32 samples.
// <out>: uint64 V; V float32 dist, V int32 tri, V int32 inst (unsigned); V float32 dist without ids; V float32 dist, V int32
// inst without tri; V float32 dist, V int32 tri, V int32 inst (signed). tests/test_gpu_world_dist_grid.py holds them to Python's.
#include <cstdio>
#include <vector>

static_assert(sizeof(psm_grid) == 36, "psm_grid: nine 4-byte numbers");

int main(int argc, char ** argv) {
    if (argc != 3) return 2;
    FILE * in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    int32_t n = 0, p = 0;
    psm_grid grid;
    float rmax = 0.0f;
    uint32_t samples = 0;
    if (std::fread(&n, sizeof n, 1, in) != 1 || n <= 0) return 4;
    std::vector<float> pos((size_t)n * 9);
    if (std::fread(pos.data(), sizeof(float), pos.size(), in) != pos.size()) return 4;
    if (std::fread(&p, sizeof p, 1, in) != 1 || p <= 0) return 4;
    std::vector<float> m16((size_t)p * 16);
    if (std::fread(m16.data(), sizeof(float), m16.size(), in) != m16.size()) return 4;
    if (std::fread(&grid, sizeof grid, 1, in) != 1 || std::fread(&rmax, sizeof rmax, 1, in) != 1 ||
        std::fread(&samples, sizeof samples, 1, in) != 1) return 4;
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
    std::vector<float> dist, alone, owned, sdist, none;
    std::vector<int32_t> tri, inst, oinst, stri, sinst, ids, owners;
    if (world.distanceField(grid, rmax, dist, &tri, &inst) != PSM_OK || world.distanceField(grid, rmax, alone) != PSM_OK ||
        world.distanceField(grid, rmax, owned, nullptr, &oinst) != PSM_OK ||
        world.signedDistanceField(grid, rmax, samples, sdist, &stri, &sinst) != PSM_OK) return 5;
    const size_t cells = (size_t)grid.dims[0] * grid.dims[1] * grid.dims[2];
    if (dist.size() != cells || tri.size() != cells || inst.size() != cells || alone.size() != cells || owned.size() != cells ||
        oinst.size() != cells || sdist.size() != cells || stri.size() != cells || sinst.size() != cells) return 6;
    // a refusal leaves the vectors empty and says why
    psm_grid bad = grid;
    bad.cell[1] = 0.0f;
    none.assign(3, 7.0f);
    ids.assign(3, 7);
    owners.assign(3, 7);
    if (world.distanceField(bad, rmax, none, &ids, &owners) != PSM_ERR_INVALID || !none.empty() || !ids.empty() || !owners.empty()) return 7;
    none.assign(3, 7.0f);
    if (world.distanceField(grid, -1.0f, none) != PSM_ERR_INVALID || !none.empty()) return 7;
    none.assign(3, 7.0f);
    owners.assign(3, 7);
    if (world.signedDistanceField(grid, rmax, 2u, none, nullptr, &owners) != PSM_ERR_INVALID || !none.empty() || !owners.empty()) return 7;

    FILE * out = std::fopen(argv[2], "wb");
    if (!out) return 3;
    const uint64_t V = cells;
    std::fwrite(&V, sizeof V, 1, out);
    std::fwrite(dist.data(), sizeof(float), cells, out);
    std::fwrite(tri.data(), sizeof(int32_t), cells, out);
    std::fwrite(inst.data(), sizeof(int32_t), cells, out);
    std::fwrite(alone.data(), sizeof(float), cells, out);
    std::fwrite(owned.data(), sizeof(float), cells, out);
    std::fwrite(oinst.data(), sizeof(int32_t), cells, out);
    std::fwrite(sdist.data(), sizeof(float), cells, out);
    std::fwrite(stri.data(), sizeof(int32_t), cells, out);
    std::fwrite(sinst.data(), sizeof(int32_t), cells, out);
    std::fclose(out);
    return 0;
}
