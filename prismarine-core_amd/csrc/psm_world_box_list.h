// psm_world_box_list.h -- the id list of a world's box query (world_box.hip, psm_world_box_triangles_dev): the k
// lowest pairs (instance, triangle) that count, ascending. psm_box_list.h's list with a 64-bit key, (inst << 32) | tri: the
// order of the keys as unsigned numbers is the lexicographic order of the pairs. Written so that it also compiles for the host
// (tests/cpp/world_box_list_host.cpp runs the insertion against std::sort under the address and undefined-behaviour
// sanitizers): the stride between a column's slots and the function qualifier are the includer's.
//
// Slot s of a query is key[s * STRIDE]. In the kernel the array is dynamic LDS laid out [slot][lane] like the stack (k x 64 x 8 B
// per wave, sized by the launch) and STRIDE is the wave's 64: a lane touches its own column only -- no cross-lane traffic, no
// barrier. The walk enters an instance once and visits a leaf of it once, so no key comes twice.
//   * while the list holds fewer than k keys every candidate that counts enters;
//   * once it holds k, a candidate enters iff its key is below the last slot's, which falls out.
// Entering is an insertion by shifting from the end. Nothing of the list is mirrored in registers.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef PSM_WORLD_BOX_LIST_FN
#define PSM_WORLD_BOX_LIST_FN inline
#endif

namespace psm {

template <int STRIDE>
struct WorldBoxList {
    uint64_t* key;
    uint32_t k, cnt;

    PSM_WORLD_BOX_LIST_FN WorldBoxList(uint64_t* keys, uint32_t slots) : key(keys), k(slots), cnt(0u) {}
    PSM_WORLD_BOX_LIST_FN static uint64_t pack(uint32_t inst, uint32_t tri) { return ((uint64_t)inst << 32) | (uint64_t)tri; }
    PSM_WORLD_BOX_LIST_FN void clear() { cnt = 0u; }
    PSM_WORLD_BOX_LIST_FN bool full() const { return cnt == k; }
    PSM_WORLD_BOX_LIST_FN void offer(uint32_t inst, uint32_t tri) {
        const uint64_t x = pack(inst, tri);
        const bool was_full = full();
        if (was_full && !(x < key[(size_t)(k - 1u) * STRIDE])) return;
        uint32_t j = was_full ? k - 1u : cnt;   // the slot that opens: the last one falls out of a full list
        cnt = j + 1u;
        while (j > 0u) {
            const uint64_t e = key[(size_t)(j - 1u) * STRIDE];
            if (!(x < e)) break;
            key[(size_t)j * STRIDE] = e;
            j--;
        }
        key[(size_t)j * STRIDE] = x;
    }
};

}  // namespace psm
