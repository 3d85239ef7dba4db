// psm_box_list.h -- the id list of a box query (box.hip, psm_bvh_box_triangles_dev): the k lowest triangle ids
// that count, ascending. Written so that it also compiles for the host (tests/cpp/box_list_host.cpp runs the insertion against
// std::sort under the address and undefined-behaviour sanitizers): the stride between a column's slots and the function
// qualifier are the includer's.
//
// Slot s of a query is id[s * STRIDE]. In the kernel the array is dynamic LDS laid out [slot][lane] like the stack (k x 64 x 4 B
// per wave, sized by the launch) and STRIDE is the wave's 64: a lane touches its own column only -- no cross-lane traffic, no
// barrier. The order is the ids' as unsigned numbers. The walk visits a leaf once, so no id comes twice.
//   * while the list holds fewer than k ids every candidate that counts enters;
//   * once it holds k, a candidate enters iff its id is below the last slot's, which falls out.
// Entering is an insertion by shifting from the end. Nothing of the list is mirrored in registers: a full list's last slot is
// read where it is needed.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef PSM_BOX_LIST_FN
#define PSM_BOX_LIST_FN inline
#endif

namespace psm {

template <int STRIDE>
struct BoxIdList {
    uint32_t* id;
    uint32_t k, cnt;

    PSM_BOX_LIST_FN BoxIdList(uint32_t* ids, uint32_t slots) : id(ids), k(slots), cnt(0u) {}
    PSM_BOX_LIST_FN void clear() { cnt = 0u; }
    PSM_BOX_LIST_FN bool full() const { return cnt == k; }
    PSM_BOX_LIST_FN void offer(uint32_t tri) {
        const bool was_full = full();
        if (was_full && !(tri < id[(size_t)(k - 1u) * STRIDE])) return;
        uint32_t j = was_full ? k - 1u : cnt;   // the slot that opens: the last one falls out of a full list
        cnt = j + 1u;
        while (j > 0u) {
            const uint32_t e = id[(size_t)(j - 1u) * STRIDE];
            if (!(tri < e)) break;
            id[(size_t)j * STRIDE] = e;
            j--;
        }
        id[(size_t)j * STRIDE] = tri;
    }
};

}  // namespace psm
