// psm_grid_walk.h -- the two brick walks of the grids over a hierarchy, moved here from grid.hip
// and grid_dist.hip as they were so that the dense kernels (grid.hip, grid_dist.hip) and the list-driven ones (grid_sparse.hip)
// instantiate the same text. Which brick a workgroup's turn b is, and where its answer goes, is a compile-time parameter:
// DenseBricks -- the bricks [g.first, g.first + g.bricks) of the grid, the dense kernels' -- or ListBricks -- the bricks a list
// names, slot by slot. The dense kernels compile to the same instructions as with the walks in their own files
// (tests/test_grid_host_cpu.py holds their digests).
#pragma once
#include "psm_query_dev.h"
#include "psm_box_dev.h"   // box_tri, box_row
#include "psm_grid_dev.h"

namespace psm {

namespace {

// the dense kernels' bricks: turn b is brick g.first + b of the grid, and a per-brick answer goes to that index
struct DenseBricks {
    PSM_D uint32_t count(const GridArgs& g) const { return g.bricks; }
    PSM_D uint32_t brick(const GridArgs& g, uint32_t b) const { return g.first + b; }
    PSM_D uint32_t slot(const GridArgs& g, uint32_t b) const { return g.first + b; }
};

// the list-driven kernels' bricks: turn b is brick ids[b] (ids NULL: brick b), its answer goes to slot b. The count is n, or
// with d_n the number on the device (at most n: the launch was sized by n). An id at or above `total`, the grid's brick count,
// becomes `total` itself: brick (0, 0, nbz), whose voxels all lie outside dims (4 nbz >= nz, no overflow: nbz <= 2^18)
struct ListBricks {
    const uint32_t* __restrict__ ids;
    const uint32_t* __restrict__ d_n;
    uint32_t n, total;
    PSM_D uint32_t count(const GridArgs&) const {
        if (!d_n) return n;
        const uint32_t m = *d_n;
        return m < n ? m : n;
    }
    PSM_D uint32_t brick(const GridArgs&, uint32_t b) const {
        const uint32_t id = ids ? ids[b] : b;
        return id < total ? id : total;
    }
    PSM_D uint32_t slot(const GridArgs&, uint32_t b) const { return b; }
};

// GRID_ANY: one byte per brick, whether any voxel of it has its bit -- the surface walk that leaves at the wave's first hit
enum { GRID_SURFACE = 0, GRID_COUNTS = 1, GRID_ANY = 2 };

// the grown image interval of a lane's voxel per normalised axis, and BoxBody::keep (box.hip) compare for compare: a child box
// [mn, mx] is kept iff it meets the interval on all three axes (negations: a NaN keeps the box)
struct Interval {
    float glx, gly, glz, ghx, ghy, ghz;
};
PSM_D bool keep(const Interval& I, float mnx, float mny, float mnz, float mxx, float mxy, float mxz) {
    bool out = mxx < I.glx;
    out |= mnx > I.ghx;
    out |= mxy < I.gly;
    out |= mny > I.ghy;
    out |= mxz < I.glz;
    out |= mnz > I.ghz;
    return !out;
}

// One wave per brick, grid-stride over the bricks. MODE: GRID_SURFACE -- a lane that has its bit stops voting, and the walk
// ends when no lane wants anything --, GRID_COUNTS -- every live lane wants every leaf its interval keeps --, GRID_ANY -- the
// surface's walk, left as soon as one lane has its bit.
// node32: the build's traversal records (bvh_emit); tri48: v0, e1, e2 per triangle; out: a uint64_t word per brick (surface: at
// the brick's slot), the dense uint32_t [nz][ny][nx] (counts), or a byte per slot (any)
template <int MODE, class Bricks, class Out>
PSM_D void grid_walk(const GridArgs& g, const Bricks bricks, const uint4* __restrict__ node32, const float4* __restrict__ tri48,
                     Out* __restrict__ out) {
    __shared__ int stack[QSTACK_MAX];   // the wave's: every lane writes and reads the same entry
    const int lane = (int)threadIdx.x;
    __builtin_assume(lane >= 0 && lane < QUERY_BLOCK);
    const int root = (int)g.sm[SM_ROOT];
    const uint32_t count = g.sm[SM_COUNT];
    const int lone = (count == 1u) ? g.sorted_tri[0] : -1;   // one leaf: no tree, the leaf's triangle is the only candidate
    float M[16];
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = u2f(g.sm[SM_M + k]);
    for (uint32_t b = blockIdx.x; b < bricks.count(g); b += gridDim.x) {
        const Voxel v = voxel_of(g, bricks.brick(g, b), lane);
        v3 lo = mk3(0.f, 0.f, 0.f), hi = mk3(-1.f, -1.f, -1.f);   // a dead lane: lo > hi (BoxBody::begin)
        if (v.inside) {
            // one multiplication, then one addition (the build contracts nothing): neighbours share their face plane bit for bit
            lo = mk3(g.ox + (float)v.ix * g.cx, g.oy + (float)v.iy * g.cy, g.oz + (float)v.iz * g.cz);
            hi = mk3(g.ox + (float)(v.ix + 1u) * g.cx, g.oy + (float)(v.iy + 1u) * g.cy, g.oz + (float)(v.iz + 1u) * g.cz);
        }
        const bool valid = v.inside && finite3(lo) && finite3(hi) && lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z;
        Interval I;   // exactly as BoxBody::begin
        box_row(M, 0, lo, hi, I.glx, I.ghx);
        box_row(M, 1, lo, hi, I.gly, I.ghy);
        box_row(M, 2, lo, hi, I.glz, I.ghz);
        uint32_t cnt = 0u;   // per brick: the grid-stride loop comes here again
        bool wants = valid;
        int t0 = lone, t1 = -1;   // the leaves to test, wave-uniform
        int cur = root, sp = 0;
        bool walking = root >= 0;
        for (;;) {
            // the accepted leaves, one test after the other: the triangle is loaded once for the wave
            while (t0 >= 0) {
                const float4* tp = tri48 + (size_t)3 * (size_t)__builtin_amdgcn_readfirstlane(t0);
                const float4 A = tp[0], B = tp[1], C = tp[2];
                if (wants && box_tri(mk3(A.x, A.y, A.z), mk3(B.x, B.y, B.z), mk3(C.x, C.y, C.z), lo, hi)) cnt++;
                t0 = t1;
                t1 = -1;
            }
            if (MODE != GRID_COUNTS) wants = valid && cnt == 0u;
            if (MODE == GRID_ANY && __ballot(cnt != 0u) != 0ull) break;
            if (!walking || __ballot(wants) == 0ull) break;
            cur = __builtin_amdgcn_readfirstlane(cur);
            const uint4* np = (const uint4*)((const char*)node32 + ((size_t)(uint32_t)cur << 5));
            const uint4 n0 = np[0], n1 = np[1];
            const int lkx = (int)n1.z, lky = (int)n1.w;
            // each lane judges both children against its own interval (the record's fp16 corners as BoxBody::children reads them)
            const bool keepL = keep(I, half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z));
            const bool keepR = keep(I, half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y));
            const bool okL = __ballot(keepL && wants) != 0ull, okR = __ballot(keepR && wants) != 0ull;
            const bool leafL = okL && lkx < 0, leafR = okR && lky < 0;
            t0 = leafL ? ~lkx : (leafR ? ~lky : -1);
            t1 = (leafL && leafR) ? ~lky : -1;
            const bool intL = okL && !leafL, intR = okR && !leafR;
            if (intL && intR) {
                // (sp < QSTACK_MAX always: one entry per internal ancestor of the current node, as a lane's own stack; the host
                // refuses hierarchies whose bound exceeds it. The test keeps every store and every pop inside the array)
                if (sp < QSTACK_MAX) {
                    stack[sp] = lky;
                    sp++;
                }
            }
            cur = intL ? lkx : lky;
            if (!(intL || intR)) {
                if (sp == 0) walking = false;   // (the node's leaves are still tested)
                else {
                    sp--;
                    cur = stack[sp];
                }
            }
        }
        if (MODE == GRID_SURFACE) {
            const unsigned long long word = __ballot(cnt != 0u);
            if (lane == 0) out[bricks.slot(g, b)] = (Out)word;
        } else if (MODE == GRID_ANY) {
            const unsigned long long word = __ballot(cnt != 0u);
            if (lane == 0) out[bricks.slot(g, b)] = (Out)(word != 0ull);
        } else if (valid) {
            out[((size_t)v.iz * g.ny + v.iy) * g.nx + v.ix] = (Out)cnt;
        }
    }
}

// what a distance walk leaves: DIST_DENSE -- the dense dist / tri [nz][ny][nx] of the whole grid (tri may be NULL) --,
// DIST_RECORDS -- a psm_hit per lane of the launch's bricks in lane order (u = v = 0), a miss for a lane outside dims, for the
// sign kernel of query.hip --, DIST_SLOTS -- dist / tri [slot][64] in lane order, +inf / -1 for a lane outside dims (tri may be
// NULL) --, DIST_ANY -- a byte per slot, whether any centre of the brick has a triangle within rmax: the walk left at the
// wave's first record
enum { DIST_DENSE = 0, DIST_RECORDS = 1, DIST_SLOTS = 2, DIST_ANY = 3 };

// One wave per brick, grid-stride over the bricks.
// Visiting order: where both children are internal and kept, the wave goes first to the one that most of the lanes that keep a
// child find nearer (their own kL <= kR): one ballot and two scalar bit counts per node on top of the two ballots that decide
// the entry, where the minimum key over the lanes would take a cross-lane reduction per child. The 64 centres lie within one brick, so the vote is rarely close.
template <int OUT, class Bricks>
PSM_D void dist_walk(const GridArgs& g, const Bricks bricks, float rmax, const uint4* __restrict__ node32, const float4* __restrict__ tri48,
                     float* __restrict__ dist, int32_t* __restrict__ tri, float4* __restrict__ hits, uint8_t* __restrict__ any) {
    __shared__ int stack[QSTACK_MAX];   // the wave's: every lane writes and reads the same entry
    const int lane = (int)threadIdx.x;
    __builtin_assume(lane >= 0 && lane < QUERY_BLOCK);
    const int root = (int)g.sm[SM_ROOT];
    const uint32_t count = g.sm[SM_COUNT];
    const int lone = (count == 1u) ? g.sorted_tri[0] : -1;   // one leaf: no tree, the leaf's triangle is the only candidate
    float M[16];
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = u2f(g.sm[SM_M + k]);
    const PointBound B = point_bound(M);
    for (uint32_t b = blockIdx.x; b < bricks.count(g); b += gridDim.x) {
        const Voxel v = voxel_of(g, bricks.brick(g, b), lane);
        // the centre as grid_centres writes it (grid.hip): one operation per rounding
        const v3 p = mk3(g.ox + ((float)v.ix + 0.5f) * g.cx, g.oy + ((float)v.iy + 0.5f) * g.cy, g.oz + ((float)v.iz + 0.5f) * g.cz);
        const bool live = v.inside && finite3(p);   // (PointBody::begin's valid; rmax was checked on the host)
        PointImage P;
        P.set(M, p);
        // per brick: the grid-stride loop comes here again
        float best = (rmax * rmax) * 1.00000095367431640625f + 0x1p-126f;   // fl(rmax^2) (1 + 2^-20) + 2^-126 (PointBody::begin)
        int btri = -1;
        bool found = false;
        int t0 = lone, t1 = -1;   // the leaves to test, wave-uniform
        int cur = root, sp = 0;
        bool walking = root >= 0;
        for (;;) {
            // the accepted leaves, one test after the other: the triangle is loaded once for the wave
            while (t0 >= 0) {
                const int id = __builtin_amdgcn_readfirstlane(t0);
                const float4* tp = tri48 + (size_t)3 * (size_t)id;
                const float4 A = tp[0], Bv = tp[1], C = tp[2];
                float u, w;
                const float d2 = closest_on_tri(mk3(A.x, A.y, A.z), mk3(Bv.x, Bv.y, Bv.z), mk3(C.x, C.y, C.z), p, u, w);
                // (PointBody::leaf, compare for compare)
                if (live && sqrtf(d2) <= rmax && (d2 < best || (d2 == best && (uint32_t)id < (uint32_t)btri))) {
                    found = true;
                    best = d2;
                    btri = id;
                }
                t0 = t1;
                t1 = -1;
            }
            if (OUT == DIST_ANY && __ballot(found) != 0ull) break;
            if (!walking) break;
            cur = __builtin_amdgcn_readfirstlane(cur);
            const uint4* np = (const uint4*)((const char*)node32 + ((size_t)(uint32_t)cur << 5));
            const uint4 n0 = np[0], n1 = np[1];
            const int lkx = (int)n1.z, lky = (int)n1.w;
            bool keepL, keepR;
            float kL, kR;
            P.children(B, n0, n1, best, keepL, keepR, kL, kR);
            const unsigned long long mL = __ballot(keepL && live), mR = __ballot(keepR && live);
            const bool okL = mL != 0ull, okR = mR != 0ull;
            const bool leafL = okL && lkx < 0, leafR = okR && lky < 0;
            t0 = leafL ? ~lkx : (leafR ? ~lky : -1);
            t1 = (leafL && leafR) ? ~lky : -1;
            const bool intL = okL && !leafL, intR = okR && !leafR;
            // nearer child first, by the majority of the lanes that keep one
            const unsigned long long nearL = __ballot(live && (keepL || keepR) && kL <= kR);
            const bool leftFirst = intL && (!intR || 2 * __popcll(nearL) >= __popcll(mL | mR));
            const int first = leftFirst ? lkx : lky, second = leftFirst ? lky : lkx;
            if (intL && intR) {
                // (sp < QSTACK_MAX always: one entry per internal ancestor of the current node, as a lane's own stack; the host
                // refuses hierarchies whose bound exceeds it. The test keeps every store and every pop inside the array)
                if (sp < QSTACK_MAX) {
                    stack[sp] = second;
                    sp++;
                }
            }
            cur = first;
            if (!(intL || intR)) {
                if (sp == 0) walking = false;   // (the node's leaves are still tested)
                else {
                    sp--;
                    cur = stack[sp];
                }
            }
        }
        const float t = found ? sqrtf(best) : __builtin_inff();
        if (OUT == DIST_ANY) {
            const unsigned long long word = __ballot(found);
            if (lane == 0) any[bricks.slot(g, b)] = (uint8_t)(word != 0ull);
        } else if (OUT == DIST_RECORDS) hits[(size_t)b * QUERY_BLOCK + lane] = make_float4(0.f, 0.f, t, __int_as_float(btri));
        else if (OUT == DIST_SLOTS) {
            const size_t i = (size_t)b * QUERY_BLOCK + lane;
            dist[i] = t;
            if (tri) tri[i] = btri;
        } else if (v.inside) {
            const size_t i = ((size_t)v.iz * g.ny + v.iy) * g.nx + v.ix;
            dist[i] = t;
            if (tri) tri[i] = btri;
        }
    }
}

}  // namespace

}  // namespace psm
