// The clearance queries' candidate test (prismarine-core_amd/csrc/psm_tri_dist_dev.h), compiled for the host and run on the CPU
// as a process of its own under the address and undefined-behaviour sanitizers (tests/test_tri_dist_query_cpu.py), with
// -ffp-contract=off as the library: one float32 rounding per operation. It reads pairs from a file -- 18 floats each: v0, e1,
// e2 of the stored triangle and a, b, c of the query -- and writes five floats per pair: d2, u, v, s, t of tri_dist. The test
// holds the file against tests/tri_dist_query_model.py bit for bit.
#include <cstdio>
#include <vector>

#define PSM_TRI_FN __host__ __device__ __forceinline__
#define PSM_POINT_FN __host__ __device__ __forceinline__
#include "psm_tri_dist_dev.h"

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: tri_dist_host pairs.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<float> out;
    float p[18];
    size_t pairs = 0, meet = 0;
    while (fread(p, sizeof(float), 18, in) == 18) {
        const psm::TriDist w = psm::tri_dist(psm::mk3(p[0], p[1], p[2]), psm::mk3(p[3], p[4], p[5]), psm::mk3(p[6], p[7], p[8]),
                                             psm::mk3(p[9], p[10], p[11]), psm::mk3(p[12], p[13], p[14]), psm::mk3(p[15], p[16], p[17]));
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
    printf("%zu pairs, %zu at distance 0\n", pairs, meet);
    return done ? 0 : 2;
}
