// The id list of the box triangles query (prismarine-core_amd/csrc/psm_box_list.h), compiled for the host and run on the CPU
// under the address and undefined-behaviour sanitizers (tests/test_box_query_cpu.py): for k = 1 .. 16, random sequences of
// distinct ids (small ones, and ones with the top bit set: the order is unsigned) go through offer(); after every offer the list
// must equal the first k of a std::sort of the ids seen. The list has exactly k slots on the heap: a write past it is caught.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "psm_box_list.h"

template <int STRIDE>
static int run(uint32_t k, const std::vector<uint32_t>& seq) {
    // exactly (k - 1) * STRIDE + 1 elements: the last slot's element is the last of the allocation
    const size_t len = (size_t)(k - 1u) * STRIDE + 1;
    uint32_t* ids = new uint32_t[len];
    psm::BoxIdList<STRIDE> L(ids, k);
    L.cnt = 7u;   // (clear() must reset whatever an earlier query left)
    L.clear();
    std::vector<uint32_t> seen;
    int bad = 0;
    for (const uint32_t id : seq) {
        L.offer(id);
        seen.push_back(id);
        std::vector<uint32_t> want = seen;
        std::sort(want.begin(), want.end());
        const size_t n = std::min<size_t>(want.size(), k);
        if (L.cnt != n || L.full() != (n == k)) bad++;
        for (size_t s = 0; s < n && !bad; s++)
            if (ids[s * STRIDE] != want[s]) bad++;
        if (bad) break;
    }
    delete[] ids;
    return bad;
}

int main() {
    std::mt19937 rng(20240611u);
    int bad = 0, runs = 0;
    for (uint32_t k = 1; k <= 16; k++)
        for (int rep = 0; rep < 60; rep++) {
            const size_t n = 1 + rng() % 40;
            std::set<uint32_t> used;   // an id never comes twice: a leaf is visited once per walk
            std::vector<uint32_t> seq;
            for (int tries = 0; seq.size() < n && tries < 1000; tries++) {
                const uint32_t id = rng() % 4 == 0 ? 0x80000000u + rng() % 8 : rng() % (rep % 2 ? 24 : 1000);
                if (used.insert(id).second) seq.push_back(id);
            }
            if (rep % 5 == 0) std::sort(seq.begin(), seq.end());                                     // ascending: every id appends
            if (rep % 5 == 1) std::sort(seq.begin(), seq.end(), [](uint32_t a, uint32_t b) { return a > b; });   // descending: every id shifts all
            bad += run<1>(k, seq);
            bad += run<64>(k, seq);
            runs += 2;
        }
    printf("box_list_host: %d runs, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
