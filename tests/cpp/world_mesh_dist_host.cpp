// One pair of a world's mesh clearance queries as world_mesh_dist.hip makes it -- the other mesh's stored triangle posed by
// mesh_query_tri (prismarine-core_amd/csrc/psm_mesh_dev.h), the instance's stored triangle posed forward by fwd_point / fwd_vec
// (psm_world_box_dev.h), tri_dist (psm_tri_dist_dev.h) between the two, and the key of the pair's dist (psm_mesh_dist_key.h) --
// compiled for the host and run on the CPU as a process of its own under the address and undefined-behaviour sanitizers
// (tests/test_world_mesh_dist_cpu.py), with -ffp-contract=off as the library: one float32 rounding per operation. It reads
// records from a file -- 42 floats each: the other mesh's pose[12] and stored v0, e1, e2, the instance's pose[12] and stored v0,
// e1, e2 -- and writes eight 32-bit words per record: d2, u, v, s, t, the key's low and high half (its triangle is the record's
// number), 0. The test holds the file against tests/world_mesh_dist_query_model.py's parts bit for bit.
#include <cmath>
#include <cstdio>
#include <vector>

#define PSM_TRI_FN __host__ __device__ __forceinline__
#define PSM_POINT_FN __host__ __device__ __forceinline__
#define PSM_WORLD_BOX_FN __host__ __device__ __forceinline__
#define PSM_MESH_FN __host__ __device__ __forceinline__
#define PSM_KEY_FN inline
#include "psm_mesh_dev.h"
#include "psm_tri_dist_dev.h"
#include "psm_mesh_dist_key.h"

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: world_mesh_dist_host records.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<uint32_t> out;
    float p[42];
    uint32_t pairs = 0;
    size_t meet = 0;
    while (fread(p, sizeof(float), 42, in) == 42) {
        psm::v3 a, b, c;
        psm::mesh_query_tri(p, psm::mk3(p[12], p[13], p[14]), psm::mk3(p[15], p[16], p[17]), psm::mk3(p[18], p[19], p[20]), a, b, c);
        const float* m = p + 21;
        const psm::v3 v0 = psm::fwd_point(m, psm::mk3(p[33], p[34], p[35]));
        const psm::v3 e1 = psm::fwd_vec(m, psm::mk3(p[36], p[37], p[38])), e2 = psm::fwd_vec(m, psm::mk3(p[39], p[40], p[41]));
        const psm::TriDist w = psm::tri_dist(v0, e1, e2, a, b, c);
        const uint64_t key = psm::mesh_key(sqrtf(w.d2), pairs);
        const float rec[5] = {w.d2, w.u, w.v, w.s, w.t};
        uint32_t words[8] = {0, 0, 0, 0, 0, (uint32_t)key, (uint32_t)(key >> 32), 0};
        memcpy(words, rec, sizeof rec);
        out.insert(out.end(), words, words + 8);
        pairs++;
        meet += w.d2 == 0.f ? 1 : 0;
    }
    fclose(in);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const bool done = fwrite(out.data(), sizeof(uint32_t), out.size(), o) == out.size();
    fclose(o);
    printf("%u records, %zu at distance 0\n", pairs, meet);
    return done ? 0 : 2;
}
