// psm_world_klist.h -- the sorted list of a world's k-best queries (world.hip): kbest.hip's KList with a third
// key word. Written so that it also compiles for the host (tests/cpp/world_klist_host.cpp runs the insertion against std::sort
// under the address and undefined-behaviour sanitizers): the key pair's type, the stride between a column's slots and the
// function qualifier are the includer's.
//
// Slot s of a query is key[s * STRIDE] = {value bits, tri} and ins[s * STRIDE] = inst. In the kernels both arrays are dynamic
// LDS laid out [slot][lane] like the stack (k x 64 x 12 B per wave, sized by the launch: the k x 64 keys, then the k x 64
// instances) and STRIDE is the wave's 64: a lane touches its own column only -- no cross-lane traffic, no barrier. The order is
// lexicographic on (value as a float, inst unsigned, tri unsigned): -0 == +0 and the ids then decide; no key is a NaN (no
// window holds one). The walk visits a leaf of an instance once, so no key comes twice.
//   * while the list holds fewer than k keys every candidate inside the window enters;
//   * once it holds k, a candidate enters iff its key is below the last slot's, which falls out.
// Entering is an insertion by shifting from the end. linst / ltri (and the caller's `last`) mirror the last slot once the list
// is full: the value every box and every candidate is then judged against.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef PSM_KLIST_FN
#define PSM_KLIST_FN inline
#endif

namespace psm {

template <class Key2, int STRIDE>
struct WorldKList {
    Key2* key;
    uint32_t* ins;
    uint32_t k, cnt, linst, ltri;

    PSM_KLIST_FN WorldKList(Key2* keys, uint32_t* insts, uint32_t slots)
        : key(keys), ins(insts), k(slots), cnt(0u), linst(0xffffffffu), ltri(0xffffffffu) {}
    PSM_KLIST_FN void clear() {
        cnt = 0u;
        linst = 0xffffffffu;
        ltri = 0xffffffffu;
    }
    PSM_KLIST_FN bool full() const { return cnt == k; }
    PSM_KLIST_FN static bool below(float x, uint32_t inst, uint32_t tri, float y, uint32_t yinst, uint32_t ytri) {
        return x < y || (x == y && (inst < yinst || (inst == yinst && tri < ytri)));
    }
    // a candidate that is inside the window: enters unless the list is full and its key is not below the last slot's (`last`,
    // linst, ltri). Returns the bound for the boxes from now on: `last` as it was, or the new last slot's value once the list
    // is full.
    PSM_KLIST_FN float offer(float x, uint32_t inst, uint32_t tri, float last) {
        const bool was_full = full();
        if (was_full && !below(x, inst, tri, last, linst, ltri)) return last;
        uint32_t j = was_full ? k - 1u : cnt;   // the slot that opens: the last one falls out of a full list
        cnt = j + 1u;
        while (j > 0u) {
            const Key2 e = key[(size_t)(j - 1u) * STRIDE];
            const uint32_t ei = ins[(size_t)(j - 1u) * STRIDE];
            if (!below(x, inst, tri, __builtin_bit_cast(float, (uint32_t)e.x), ei, e.y)) break;
            key[(size_t)j * STRIDE] = e;
            ins[(size_t)j * STRIDE] = ei;
            j--;
        }
        key[(size_t)j * STRIDE] = Key2{__builtin_bit_cast(uint32_t, x), tri};
        ins[(size_t)j * STRIDE] = inst;
        if (!full()) return last;
        const Key2 e = key[(size_t)(k - 1u) * STRIDE];
        ltri = e.y;
        linst = ins[(size_t)(k - 1u) * STRIDE];
        return __builtin_bit_cast(float, (uint32_t)e.x);
    }
};

}  // namespace psm
