// What a world's mesh query computes for one (pose, leaf of `other`, instance, candidate), as world_mesh.hip's begin() and leaf()
// make it -- the query triangle of a stored leaf at a pose (mesh_query_tri, prismarine-core_amd/csrc/psm_mesh_dev.h), the
// candidate posed forward by fwd_point / fwd_vec (psm_world_box_dev.h), then tri_tri (psm_tri_dev.h) -- compiled for the host and
// run on the CPU as a process of its own under the address and undefined-behaviour sanitizers (tests/test_world_mesh_cpu.py),
// with -ffp-contract=off as the library: one float32 rounding per operation. It reads records from a file -- 42 floats each: the
// mesh pose m[12], the other hierarchy's stored v0, e1, e2, the instance's pose w[12] and the candidate's stored v0, e1, e2 -- and
// writes a byte per record, the answer, and 18 floats per record: the query triangle (a, b, c) and the posed candidate
// (v0', e1', e2'). The test holds all three against the models record for record.
#include <cstdio>
#include <vector>

#define PSM_TRI_FN __host__ __device__ __forceinline__
#define PSM_WORLD_BOX_FN __host__ __device__ __forceinline__
#define PSM_MESH_FN __host__ __device__ __forceinline__
#include "psm_mesh_dev.h"

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: world_mesh_host records.bin flags.bin posed.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<unsigned char> out;
    std::vector<float> posed;
    float p[42];
    size_t meet = 0;
    while (fread(p, sizeof(float), 42, in) == 42) {
        const float* w = p + 21;
        psm::v3 a, b, c;
        psm::mesh_query_tri(p, psm::mk3(p[12], p[13], p[14]), psm::mk3(p[15], p[16], p[17]), psm::mk3(p[18], p[19], p[20]), a, b, c);
        const psm::v3 v0 = psm::fwd_point(w, psm::mk3(p[33], p[34], p[35]));
        const psm::v3 e1 = psm::fwd_vec(w, psm::mk3(p[36], p[37], p[38])), e2 = psm::fwd_vec(w, psm::mk3(p[39], p[40], p[41]));
        const bool ok = psm::tri_tri(v0, e1, e2, a, b, c);
        out.push_back(ok ? 1 : 0);
        meet += ok ? 1 : 0;
        const float v[18] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, v0.x, v0.y, v0.z, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z};
        posed.insert(posed.end(), v, v + 18);
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
