// The candidate test of a world's triangle queries as world_tri.hip's leaf() makes it -- the stored triangle posed forward by
// fwd_point / fwd_vec (prismarine-core_amd/csrc/psm_world_box_dev.h), then tri_tri (psm_tri_dev.h) against the world triangle --
// compiled for the host and run on the CPU as a process of its own under the address and undefined-behaviour sanitizers
// (tests/test_world_tri_cpu.py), with -ffp-contract=off as the library: one float32 rounding per operation. It reads records from
// a file -- 30 floats each: the pose m[12], the stored v0, e1, e2 and the query's a, b, c -- and writes a byte per record, the
// answer, and the posed (v0', e1', e2') as 9 floats per record. The test holds both against tests/world_tri_query_model.py
// record for record.
#include <cstdio>
#include <vector>

#define PSM_TRI_FN __host__ __device__ __forceinline__
#define PSM_WORLD_BOX_FN __host__ __device__ __forceinline__
#include "psm_world_box_dev.h"
#include "psm_tri_dev.h"

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: world_tri_pose_host records.bin flags.bin posed.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<unsigned char> out;
    std::vector<float> posed;
    float p[30];
    size_t meet = 0;
    while (fread(p, sizeof(float), 30, in) == 30) {
        const float* m = p;
        const psm::v3 v0 = psm::fwd_point(m, psm::mk3(p[12], p[13], p[14]));
        const psm::v3 e1 = psm::fwd_vec(m, psm::mk3(p[15], p[16], p[17])), e2 = psm::fwd_vec(m, psm::mk3(p[18], p[19], p[20]));
        const bool ok = psm::tri_tri(v0, e1, e2, psm::mk3(p[21], p[22], p[23]), psm::mk3(p[24], p[25], p[26]), psm::mk3(p[27], p[28], p[29]));
        out.push_back(ok ? 1 : 0);
        meet += ok ? 1 : 0;
        const float v[9] = {v0.x, v0.y, v0.z, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z};
        posed.insert(posed.end(), v, v + 9);
    }
    fclose(in);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    bool done = fwrite(out.data(), 1, out.size(), o) == out.size();
    fclose(o);
    o = fopen(argv[3], "wb");
    if (!o) return 2;
    done = done && fwrite(posed.data(), sizeof(float), posed.size(), o) == posed.size();
    fclose(o);
    printf("%zu records, %zu meet\n", out.size(), meet);
    return done ? 0 : 2;
}
