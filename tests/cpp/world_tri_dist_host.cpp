// The candidate test of a world's clearance queries as world_tri_dist.hip's leaf() makes it -- the stored triangle posed forward by
// fwd_point / fwd_vec (prismarine-core_amd/csrc/psm_world_box_dev.h), then tri_dist (psm_tri_dist_dev.h) against the world
// triangle -- compiled for the host and run on the CPU as a process of its own under the address and undefined-behaviour
// sanitizers (tests/test_world_tri_dist_cpu.py), with -ffp-contract=off as the library: one float32 rounding per operation. It
// reads records from a file -- 30 floats each: the pose m[12], the stored v0, e1, e2 and the query's a, b, c -- and writes five
// floats per record: d2, u, v, s, t. The test holds the file against tests/world_tri_dist_query_model.py bit for bit.
#include <cstdio>
#include <vector>

#define PSM_TRI_FN __host__ __device__ __forceinline__
#define PSM_POINT_FN __host__ __device__ __forceinline__
#define PSM_WORLD_BOX_FN __host__ __device__ __forceinline__
#include "psm_world_box_dev.h"
#include "psm_tri_dist_dev.h"

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: world_tri_dist_host records.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<float> out;
    float p[30];
    size_t pairs = 0, meet = 0;
    while (fread(p, sizeof(float), 30, in) == 30) {
        const float* m = p;
        const psm::v3 v0 = psm::fwd_point(m, psm::mk3(p[12], p[13], p[14]));
        const psm::v3 e1 = psm::fwd_vec(m, psm::mk3(p[15], p[16], p[17])), e2 = psm::fwd_vec(m, psm::mk3(p[18], p[19], p[20]));
        const psm::TriDist w = psm::tri_dist(v0, e1, e2, psm::mk3(p[21], p[22], p[23]), psm::mk3(p[24], p[25], p[26]), psm::mk3(p[27], p[28], p[29]));
        const float rec[5] = {w.d2, w.u, w.v, w.s, w.t};
        out.insert(out.end(), rec, rec + 5);
        pairs++;
        meet += w.d2 == 0.f ? 1 : 0;
    }
    fclose(in);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const bool done = fwrite(out.data(), sizeof(float), out.size(), o) == out.size();
    fclose(o);
    printf("%zu records, %zu at distance 0\n", pairs, meet);
    return done ? 0 : 2;
}
