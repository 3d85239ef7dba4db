#include "Prismarine/Prismarine.hpp"
#include "Prismarine/Implementations.hpp"   // as the reference: one translation unit of the application includes the bodies
// The sparse grids of the header layer (not in the reference) on a GPU: sparse_grid_host <in> <out>.
// <in>: int32 n; n x 9 float32 triangle positions; psm_grid (3 float32 origin, 3 float32 cell, 3 uint32 dims); float32 rmax;
// uint32 samples.
// <out>: four blocks, each uint64 N, N uint32 ids, then the block's answers: N uint64 words (sparseVoxelize); 64 N float32 dist,
// 64 N int32 tri (sparseDistanceField); 64 N float32 dist (the same without ids); 64 N float32 dist, 64 N int32 tri
// (sparseSignedDistanceField). tests/test_gpu_sparse_grid.py holds them to Python's.
#include <cstdio>
#include <vector>

static_assert(sizeof(psm_grid) == 36, "psm_grid: nine 4-byte numbers");

template <class T>
static void put(FILE * out, const std::vector<T> & v) {
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), out);
}

int main(int argc, char ** argv) {
    if (argc != 3) return 2;
    FILE * in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    int32_t n = 0;
    psm_grid grid;
    float rmax = 0.0f;
    uint32_t samples = 0;
    if (std::fread(&n, sizeof n, 1, in) != 1 || n <= 0) return 4;
    std::vector<float> pos((size_t)n * 9);
    if (std::fread(pos.data(), sizeof(float), pos.size(), in) != pos.size()) return 4;
    if (std::fread(&grid, sizeof grid, 1, in) != 1 || std::fread(&rmax, sizeof rmax, 1, in) != 1 ||
        std::fread(&samples, sizeof samples, 1, in) != 1) return 4;
    std::fclose(in);

    psm::TriangleHierarchy th;
    th.allocate((size_t)n);
    th.loadTriangles(pos.data(), nullptr, nullptr, (size_t)n);
    th.build();
    std::vector<uint32_t> wids, dids, aids, sids, none_ids;
    std::vector<uint64_t> words, none_words;
    std::vector<float> dist, alone, sdist, none;
    std::vector<int32_t> tri, stri, none_tri;
    if (th.sparseVoxelize(grid, wids, words) != PSM_OK || th.sparseDistanceField(grid, rmax, dids, dist, &tri) != PSM_OK ||
        th.sparseDistanceField(grid, rmax, aids, alone) != PSM_OK ||
        th.sparseSignedDistanceField(grid, rmax, samples, sids, sdist, &stri) != PSM_OK) return 5;
    if (words.size() != wids.size() || dist.size() != 64 * dids.size() || tri.size() != dist.size() || alone.size() != 64 * aids.size() ||
        sdist.size() != 64 * sids.size() || stri.size() != sdist.size()) return 6;
    // a band that reaches nothing is an empty list, not a refusal
    psm_grid far = grid;
    far.origin[0] += 1000.0f;
    none_ids.assign(3, 7u);
    none.assign(3, 7.0f);
    none_tri.assign(3, 7);
    if (th.sparseDistanceField(far, rmax, none_ids, none, &none_tri) != PSM_OK || !none_ids.empty() || !none.empty() || !none_tri.empty()) return 7;
    // a refusal leaves the vectors empty and says why
    psm_grid bad = grid;
    bad.cell[1] = 0.0f;
    none_ids.assign(3, 7u);
    none_words.assign(3, 7u);
    if (th.sparseVoxelize(bad, none_ids, none_words) != PSM_ERR_INVALID || !none_ids.empty() || !none_words.empty()) return 8;
    none_ids.assign(3, 7u);
    none.assign(3, 7.0f);
    if (th.sparseDistanceField(grid, -1.0f, none_ids, none) != PSM_ERR_INVALID || !none_ids.empty() || !none.empty()) return 8;
    none_ids.assign(3, 7u);
    none.assign(3, 7.0f);
    if (th.sparseSignedDistanceField(grid, rmax, 2u, none_ids, none) != PSM_ERR_INVALID || !none_ids.empty() || !none.empty()) return 8;

    FILE * out = std::fopen(argv[2], "wb");
    if (!out) return 3;
    uint64_t N = wids.size();
    std::fwrite(&N, sizeof N, 1, out);
    put(out, wids);
    put(out, words);
    N = dids.size();
    std::fwrite(&N, sizeof N, 1, out);
    put(out, dids);
    put(out, dist);
    put(out, tri);
    N = aids.size();
    std::fwrite(&N, sizeof N, 1, out);
    put(out, aids);
    put(out, alone);
    N = sids.size();
    std::fwrite(&N, sizeof N, 1, out);
    put(out, sids);
    put(out, sdist);
    put(out, stri);
    std::fclose(out);
    return 0;
}
