// kbest.hip -- k-best queries against a built hierarchy (new; no reference counterpart; include/psm_hip.h "k-best queries",
// DESIGN.md 4.12): the first k hits of a ray in the order (t, tri), the k nearest triangles of a point in the order (d2, tri).
//
// The walk is query.hip's (query_walk, psm_query_dev.h): one query per lane, one wave64 per workgroup, grid-stride, the stack
// [depth][lane] in LDS with its tail in the context's spill area, nearer child first. The candidates, the window and the box
// tests are the closest-hit / closest-point kernels', unchanged; what a body adds is a sorted list of k keys per lane.
//
// The list. k keys {value bits, tri} of 8 bytes, in dynamic LDS laid out [slot][lane] like the stack (k x 64 x 8 B per wave,
// sized by the launch): a lane reads and writes its own column only -- no bank conflict (a ds_read_b64 serves 16 lanes with
// consecutive 8-byte addresses per cycle), no cross-lane traffic, no barrier. Not registers: 16 keys are 32 VGPRs and an array
// indexed at run time goes to scratch. The order is lexicographic on (value as a float, tri unsigned): -0 == +0 and the id
// then decides; no key is ever a NaN (no window holds one). A leaf is visited once per walk, so no key comes twice.
//   * while the list holds fewer than k keys every candidate inside the window enters, and boxes are pruned against the
//     window's own bound (tmax / the rmax bound of PointBody::begin);
//   * once it holds k, a candidate enters iff its key is below the last slot's (which falls out), and boxes are pruned against
//     the last slot's value with `<=`: a candidate as far as the last and of a lower id must still be reached.
// Entering is an insertion by shifting from the end. u, v are not kept: finish() runs the same tri_query / closest_on_tri on
// the stored triangle again -- the same function on the same inputs gives the same bits (-ffp-contract=off), and the list
// stays at 8 bytes per slot (DESIGN.md 4.12 has the LDS budget).
#include <cstdio>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"

namespace psm {

namespace {

// a lane's column of the wave's list: slot s of this lane is col[s * QUERY_BLOCK]
PSM_D uint2* list_column() {
    extern __shared__ uint2 kbest_list[];
    return kbest_list + threadIdx.x;
}

// The sorted list of one query (see the head of the file). `last` / `ltri` mirror the last slot once the list is full: the
// value every box and every candidate is judged against.
struct KList {
    uint2* col;
    uint32_t k, cnt, ltri;

    PSM_D void clear() {
        cnt = 0u;
        ltri = 0xffffffffu;
    }
    PSM_D bool full() const { return cnt == k; }
    PSM_D static bool below(float x, uint32_t tri, float y, uint32_t ytri) { return x < y || (x == y && tri < ytri); }
    // a candidate that is inside the window: enters unless the list is full and its key is not below the last slot's (`last`).
    // Returns the bound for the boxes from now on: `last` as it was, or the new last slot's value once the list is full.
    PSM_D float offer(float x, uint32_t tri, float last) {
        const bool was_full = full();
        if (was_full && !below(x, tri, last, ltri)) return last;
        uint32_t j = was_full ? k - 1u : cnt;   // the slot that opens: the last one falls out of a full list
        cnt = j + 1u;
        while (j > 0u) {
            const uint2 e = col[(size_t)(j - 1u) * QUERY_BLOCK];
            if (!below(x, tri, __uint_as_float(e.x), e.y)) break;
            col[(size_t)j * QUERY_BLOCK] = e;
            j--;
        }
        col[(size_t)j * QUERY_BLOCK] = make_uint2(__float_as_uint(x), tri);
        if (!full()) return last;
        const uint2 e = col[(size_t)(k - 1u) * QUERY_BLOCK];
        ltri = e.y;
        return __uint_as_float(e.x);
    }
};

// the first k hits of a ray: RayBody<false> (query.hip) with the list in the place of its one best record
struct FirstHitsBody {
    const QueryArgs& a;
    KList L;
    v3 o, d;
    float tmin, tmax, lim;   // lim: the boxes' bound -- tmax until the list is full, then the last slot's t
    Axis X, Y, Z;

    PSM_D bool begin(size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 1.f), r1 = make_float4(1.f, 0.f, 0.f, -1.f);
        if (alive) { r0 = a.rays[2 * i]; r1 = a.rays[2 * i + 1]; }
        o = mk3(r0.x, r0.y, r0.z);
        d = normalize3(mk3(r1.x, r1.y, r1.z));
        tmin = r0.w;
        tmax = r1.w;
        const bool valid = alive && finite3(o) && finite3(d) && tmin <= tmax;
        lim = tmax;
        L.clear();   // per query: the grid-stride loop comes here again
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
        X = ray_axis(M, 0, o, d);
        Y = ray_axis(M, 1, o, d);
        Z = ray_axis(M, 2, o, d);
        return valid;
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& nL, float& nR) const {
        float fL, fR;
        slab(X, Y, Z, half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z), nL, fL);
        slab(X, Y, Z, half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y), nR, fR);
        okL = (nL <= fL) & (nL <= lim) & (fL >= tmin);
        okR = (nR <= fR) & (nR <= lim) & (fR >= tmin);
    }
    PSM_D void leaf(int tri) {
        float t, u, v;
        const bool hit = tri_query(a.tri48, tri, o, d, t, u, v) && t >= tmin && t <= tmax;
        if (hit) lim = L.offer(t, (uint32_t)tri, lim);
    }
    PSM_D bool done() const { return false; }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        float4* __restrict__ row = a.hits + i * L.k;
        for (uint32_t s = 0; s < L.k; s++) {
            float4 h = miss_hit();
            if (s < L.cnt) {
                const uint2 e = L.col[(size_t)s * QUERY_BLOCK];
                float t = 0.f, u = 0.f, v = 0.f;
                (void)tri_query(a.tri48, (int)e.y, o, d, t, u, v);   // the same test again: u, v (and t) bit for bit
                h = make_float4(u, v, __uint_as_float(e.x), __uint_as_float(e.y));
            }
            row[s] = h;
        }
        a.count[i] = L.cnt;
    }
};

// the k nearest triangles of a point: PointBody<false> (query.hip) with the list in the place of its one best record
struct NearestBody {
    const QueryArgs& a;
    const PointBound B;
    KList L;
    v3 p;
    float rmax, best;   // best: the boxes' bound -- the rmax bound until the list is full, then the last slot's d2
    PointImage P;

    PSM_D bool begin(size_t i, bool alive) {
        const float4 q = load_point(a.rays, i, alive);
        p = mk3(q.x, q.y, q.z);
        rmax = q.w;
        const bool valid = alive && finite3(p) && rmax >= 0.f;
        best = (rmax * rmax) * 1.00000095367431640625f + 0x1p-126f;   // fl(rmax^2) (1 + 2^-20) + 2^-126 (PointBody::begin)
        L.clear();
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
        P.set(M, p);
        return valid;
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& kL, float& kR) const {
        P.children(B, n0, n1, best, okL, okR, kL, kR);
    }
    PSM_D float test(int tri, float& u, float& v) const {
        const float4 A = a.tri48[(size_t)3 * tri + 0], Bv = a.tri48[(size_t)3 * tri + 1], C = a.tri48[(size_t)3 * tri + 2];
        return closest_on_tri(mk3(A.x, A.y, A.z), mk3(Bv.x, Bv.y, Bv.z), mk3(C.x, C.y, C.z), p, u, v);
    }
    // (the key is d2, not dist: two different d2 may share a sqrtf; a d2 that counts is <= the rmax bound: psm_query_dev.h)
    PSM_D void leaf(int tri) {
        float u, v;
        const float d2 = test(tri, u, v);
        if (sqrtf(d2) <= rmax) best = L.offer(d2, (uint32_t)tri, best);
    }
    PSM_D bool done() const { return false; }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        float4* __restrict__ row = a.hits + i * L.k;
        for (uint32_t s = 0; s < L.k; s++) {
            float4 h = miss_hit();
            if (s < L.cnt) {
                const uint2 e = L.col[(size_t)s * QUERY_BLOCK];
                float u, v;
                (void)test((int)e.y, u, v);
                h = make_float4(u, v, sqrtf(__uint_as_float(e.x)), __uint_as_float(e.y));
            }
            row[s] = h;
        }
        a.count[i] = L.cnt;
    }
};

}  // namespace

// QueryArgs as the closest-hit / closest-point kernels read it, and: hits [n][k], count [n], samples = k.
// __launch_bounds__(64, 7), not query.hip's 8: the VGPRs fit 64 either way (60 / 62), but at 8 waves per SIMD the compiler may
// use 78 SGPRs only, and the walk with the list's loops inside it needs 87 / 79: it spilled 10 / 2 of them into VGPR lanes.
// At 7 the budget is 94 and nothing spills. From k = 3 on the list's LDS, not the registers, bounds the waves.
__global__ __launch_bounds__(QUERY_BLOCK, 7) void bvh_query_first_hits(QueryArgs a) {
    FirstHitsBody q{a, KList{list_column(), a.samples, 0u, 0u}};
    query_walk(a, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, 7) void bvh_query_nearest(QueryArgs a) {
    float M[16];
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
    NearestBody q{a, point_bound(M), KList{list_column(), a.samples, 0u, 0u}};
    query_walk(a, q);
}

// query.hip's host path (query(): the checks, the stack area, the grid) launches through this: a.samples = k, 1 .. PSM_QUERY_K_MAX
int kbest_launch(psm_ctx* c, bool points, uint32_t grid, const QueryArgs& a) {
    const size_t lds = (size_t)a.samples * QUERY_BLOCK * sizeof(uint2);
    if (points) bvh_query_nearest<<<grid, QUERY_BLOCK, lds, c->stream>>>(a);
    else bvh_query_first_hits<<<grid, QUERY_BLOCK, lds, c->stream>>>(a);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace psm
