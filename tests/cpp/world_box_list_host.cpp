// The key list of a world's box triangles query (prismarine-core_amd/csrc/psm_world_box_list.h), compiled for the host and run
// on the CPU under the address and undefined-behaviour sanitizers (tests/test_world_box_cpu.py): for k = 1 .. 16, random
// sequences of distinct (instance, triangle) pairs -- small ones, and ones with the top bit set in either half: the order is
// unsigned -- go through offer(); after every offer the list must equal the first k of a std::sort of the keys seen. The list has
// exactly k slots on the heap: a write past it is caught.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "psm_world_box_list.h"

struct Pair {
    uint32_t inst, tri;
};

template <int STRIDE>
static int run(uint32_t k, const std::vector<Pair>& seq) {
    // exactly (k - 1) * STRIDE + 1 elements: the last slot's element is the last of the allocation
    const size_t len = (size_t)(k - 1u) * STRIDE + 1;
    uint64_t* keys = new uint64_t[len];
    psm::WorldBoxList<STRIDE> L(keys, k);
    L.cnt = 7u;   // (clear() must reset whatever an earlier query left)
    L.clear();
    std::vector<uint64_t> seen;
    int bad = 0;
    for (const Pair p : seq) {
        L.offer(p.inst, p.tri);
        seen.push_back(((uint64_t)p.inst << 32) | p.tri);
        std::vector<uint64_t> want = seen;
        std::sort(want.begin(), want.end());
        const size_t n = std::min<size_t>(want.size(), k);
        if (L.cnt != n || L.full() != (n == k)) bad++;
        for (size_t s = 0; s < n && !bad; s++)
            if (keys[s * STRIDE] != want[s]) bad++;
        // the lexicographic order of the pairs is the keys' order
        for (size_t s = 1; s < n && !bad; s++) {
            const uint32_t i0 = (uint32_t)(keys[(s - 1) * STRIDE] >> 32), t0 = (uint32_t)keys[(s - 1) * STRIDE];
            const uint32_t i1 = (uint32_t)(keys[s * STRIDE] >> 32), t1 = (uint32_t)keys[s * STRIDE];
            if (!(i0 < i1 || (i0 == i1 && t0 < t1))) bad++;
        }
        if (bad) break;
    }
    delete[] keys;
    return bad;
}

int main() {
    std::mt19937 rng(20240917u);
    int bad = 0, runs = 0;
    auto half = [&](int rep) -> uint32_t { return (uint32_t)( rng() % 4 == 0 ? 0x80000000u + rng() % 4 : rng() % (rep % 2 ? 6 : 1000)); };
    for (uint32_t k = 1; k <= 16; k++)
        for (int rep = 0; rep < 60; rep++) {
            const size_t n = 1 + rng() % 40;
            std::set<uint64_t> used;   // a pair never comes twice: an instance is entered once, a leaf visited once
            std::vector<Pair> seq;
            for (int tries = 0; seq.size() < n && tries < 1000; tries++) {
                const Pair p = {half(rep), half(rep)};
                if (used.insert(((uint64_t)p.inst << 32) | p.tri).second) seq.push_back(p);
            }
            auto less = [](Pair a, Pair b) { return a.inst < b.inst || (a.inst == b.inst && a.tri < b.tri); };
            if (rep % 5 == 0) std::sort(seq.begin(), seq.end(), less);                                        // ascending: every key appends
            if (rep % 5 == 1) std::sort(seq.begin(), seq.end(), [&](Pair a, Pair b) { return less(b, a); });   // descending: every key shifts all
            bad += run<1>(k, seq);
            bad += run<64>(k, seq);
            runs += 2;
        }
    printf("world_box_list_host: %d runs, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
