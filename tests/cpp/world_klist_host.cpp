// The sorted list of a world's k-best queries (prismarine-core_amd/csrc/psm_world_klist.h), compiled for the host and run on the
// CPU under the address and undefined-behaviour sanitizers (tests/test_world_kbest_cpu.py): for k = 1 .. 16, random sequences of
// candidates (no (inst, tri) twice) with ties in each of the three key words and -0 beside +0 go through offer(); the list must
// equal the first k of a std::sort by (value as a float, inst, tri), and the bound offer() returns must be the last slot's value
// once the list is full. The list has exactly k slots on the heap: a write past it is caught.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "psm_world_klist.h"

struct Key2 {
    uint32_t x, y;
};
struct Cand {
    float x;
    uint32_t inst, tri;
};
static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static bool less(const Cand& a, const Cand& b) { return a.x < b.x || (a.x == b.x && (a.inst < b.inst || (a.inst == b.inst && a.tri < b.tri))); }

template <int STRIDE>
static int run(uint32_t k, const std::vector<Cand>& seq, float window) {
    // exactly (k - 1) * STRIDE + 1 elements: the last slot's element is the last of the allocation
    const size_t len = (size_t)(k - 1u) * STRIDE + 1;
    Key2* keys = new Key2[len];
    uint32_t* ins = new uint32_t[len];
    psm::WorldKList<Key2, STRIDE> L(keys, ins, k);
    L.cnt = 7u;   // (clear() must reset whatever an earlier query left)
    L.clear();
    float lim = window;
    std::vector<Cand> seen;
    int bad = 0;
    for (const Cand& c : seq) {
        lim = L.offer(c.x, c.inst, c.tri, lim);
        seen.push_back(c);
        std::vector<Cand> want = seen;
        std::sort(want.begin(), want.end(), less);
        const size_t n = std::min<size_t>(want.size(), k);
        if (L.cnt != n) bad++;
        for (size_t s = 0; s < n && !bad; s++) {
            const Key2 e = keys[s * STRIDE];
            // the value's bits as offered: -0 stays -0, although it compares equal to +0
            if (e.x != bits(want[s].x) || e.y != want[s].tri || ins[s * STRIDE] != want[s].inst) bad++;
        }
        const float expect = n == k ? want[k - 1].x : window;
        if (bits(lim) != bits(expect) && !(lim == expect)) bad++;
        if (n == k && (L.linst != want[k - 1].inst || L.ltri != want[k - 1].tri)) bad++;
        if (bad) break;
    }
    delete[] keys;
    delete[] ins;
    return bad;
}

int main() {
    std::mt19937 rng(20240607u);
    const float values[] = {-0.0f, 0.0f, 0.5f, 0.5f, 1.0f, 1.25f, 3.0f, 1e-30f, 7.5f};
    int bad = 0, runs = 0;
    for (uint32_t k = 1; k <= 16; k++)
        for (int rep = 0; rep < 60; rep++) {
            const size_t n = 1 + rng() % 30;
            std::set<std::pair<uint32_t, uint32_t>> used;   // an (inst, tri) never comes twice: a leaf is visited once per walk
            std::vector<Cand> seq;
            for (int tries = 0; seq.size() < n && tries < 1000; tries++) {
                Cand c;
                c.x = (rep % 3 == 0) ? values[rng() % 9] : (float)(rng() % 5) * 0.25f;
                c.inst = (rep % 2) ? rng() % 3 : (rng() % 2 ? 0xfffffffeu - rng() % 2 : rng() % 4);   // (unsigned: 0xfffffffe is large)
                c.tri = rng() % 4 == 0 ? 0x80000000u + rng() % 2 : rng() % 12;
                if (used.insert(std::make_pair(c.inst, c.tri)).second) seq.push_back(c);
            }
            bad += run<1>(k, seq, 100.0f);
            bad += run<64>(k, seq, 100.0f);
            runs += 2;
        }
    printf("world_klist_host: %d runs, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
