// The word the lanes of a pose share in the mesh clearance query (prismarine-core_amd/csrc/psm_mesh_dist_key.h), compiled for the
// host and run on the CPU as a process of its own under the address and undefined-behaviour sanitizers
// (tests/test_mesh_dist_cpu.py). It reads records from a file -- a float32 dist and a uint32 t each -- and writes the 64-bit key
// of each; the test holds the keys against tests/mesh_dist_query_model.py and their order against (dist, t). Before that it
// holds the order itself on the values that matter: 0, the denormals, equal dists, +inf, and that no key is all-ones.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#define PSM_KEY_FN inline
#include "psm_mesh_dist_key.h"

static bool order_holds() {
    const float inf = std::numeric_limits<float>::infinity();
    const float dists[] = {0.f, std::numeric_limits<float>::denorm_min(), 2 * std::numeric_limits<float>::denorm_min(),
                           std::nextafter(std::numeric_limits<float>::min(), 0.f), std::numeric_limits<float>::min(), 1e-20f, 0.5f,
                           std::nextafter(1.f, 0.f), 1.f, std::nextafter(1.f, 2.f), 3e38f, std::numeric_limits<float>::max(), inf};
    const uint32_t ids[] = {0u, 1u, 63u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    uint64_t last = 0;
    bool first = true;
    for (float d : dists)
        for (uint32_t t : ids) {
            const uint64_t key = psm::mesh_key(d, t);
            if (key == psm::MESH_KEY_NONE || psm::mesh_key_dist(key) != d || psm::mesh_key_tri(key) != t) return false;
            if (!first && !(last < key)) return false;   // ascending (dist, t) is ascending key
            last = key;
            first = false;
        }
    return last < psm::MESH_KEY_NONE && std::isnan(psm::mesh_key_dist(psm::MESH_KEY_NONE));
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: mesh_dist_key_host records.bin keys.bin\n");
        return 2;
    }
    if (!order_holds()) return 3;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<uint64_t> out;
    struct { float dist; uint32_t t; } rec;
    while (fread(&rec, sizeof rec, 1, in) == 1) out.push_back(psm::mesh_key(rec.dist, rec.t));
    fclose(in);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const bool done = fwrite(out.data(), sizeof(uint64_t), out.size(), o) == out.size();
    fclose(o);
    printf("%zu keys\n", out.size());
    return done ? 0 : 2;
}
