// What a mesh query puts in front of the triangle queries' candidate test, as mesh.hip's begin() and leaf() make it -- the query
// triangle of a stored leaf at a pose (mesh_query_tri, prismarine-core_amd/csrc/psm_mesh_dev.h, over fwd_point / fwd_vec of
// psm_world_box_dev.h), then tri_tri (psm_tri_dev.h) of a stored candidate against it -- compiled for the host and run on the CPU
// as a process of its own under the address and undefined-behaviour sanitizers (tests/test_mesh_query_cpu.py), with
// -ffp-contract=off as the library: one float32 rounding per operation. It reads records from a file -- 30 floats each: the pose
// m[12], the other hierarchy's stored v0, e1, e2 and the candidate's stored v0, e1, e2 -- and writes a byte per record, the
// answer, and the query triangle (a, b, c) as 9 floats per record. The test holds both against tests/mesh_query_model.py record
// for record. Before that it holds mesh_split (query i -> pose i / L, leaf i % L, by a multiplication) to the division.
#include <cstdint>
#include <cstdio>
#include <vector>

#define PSM_TRI_FN __host__ __device__ __forceinline__
#define PSM_WORLD_BOX_FN __host__ __device__ __forceinline__
#define PSM_MESH_FN __host__ __device__ __forceinline__
#include "psm_mesh_dev.h"

static bool split_is_division() {
    const uint32_t leaves[] = {1u, 2u, 3u, 5u, 7u, 63u, 64u, 65u, 130u, 1000u, 2304u, 65535u, 65536u, 65537u, 262143u, 1000003u,
                               (1u << 26) - 1u, 1u << 26, (1u << 26) + 1u, (1u << 27) - 1u};
    uint64_t x = 88172645463325252ull;   // xorshift64
    for (uint32_t L : leaves) {
        const uint64_t magic = psm::mesh_magic(L);
        for (int k = 0; k < 20000; k++) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            // below MESH_QUERIES_MAX: small ones, the multiples of L and their neighbours, the top of the range
            uint64_t i = x % psm::MESH_QUERIES_MAX;
            if (k % 4 == 1) i = (i / L) * L;
            if (k % 4 == 2) i = (i / L) * L + (L - 1u);
            if (i >= psm::MESH_QUERIES_MAX) i -= L;
            if (k % 4 == 3) i = psm::MESH_QUERIES_MAX - 1u - (x >> 40);
            if (k < 300) i = (uint64_t)k;
            uint64_t q;
            uint32_t j;
            psm::mesh_split(i, L, magic, q, j);
            if (q != i / L || j != i % L) {
                fprintf(stderr, "mesh_split(%llu, %u): %llu, %u\n", (unsigned long long)i, L, (unsigned long long)q, j);
                return false;
            }
        }
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: mesh_pose_host records.bin flags.bin posed.bin\n");
        return 2;
    }
    if (!split_is_division()) return 3;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<unsigned char> out;
    std::vector<float> posed;
    float p[30];
    size_t meet = 0;
    while (fread(p, sizeof(float), 30, in) == 30) {
        psm::v3 a, b, c;
        psm::mesh_query_tri(p, psm::mk3(p[12], p[13], p[14]), psm::mk3(p[15], p[16], p[17]), psm::mk3(p[18], p[19], p[20]), a, b, c);
        const bool ok = psm::tri_tri(psm::mk3(p[21], p[22], p[23]), psm::mk3(p[24], p[25], p[26]), psm::mk3(p[27], p[28], p[29]), a, b, c);
        out.push_back(ok ? 1 : 0);
        meet += ok ? 1 : 0;
        const float v[9] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
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
