// world_grid_dist.hip -- distance-field grids over an instance world (new; no reference counterpart; include/psm_hip.h "voxel
// grids over a world: distance fields"): the distance from every voxel centre of a regular WORLD grid to the
// nearest posed triangle of any instance within rmax, that triangle's id and its instance; signed, the distance with the sign
// of the world's inside test. Every voxel is answered bit for bit as psm_world_closest_point_dev /
// psm_world_signed_distance_dev answer the voxel's centre.
//
// The walk is world_grid.hip's two-level brick walk with grid_dist.hip's node step: a 4 x 4 x 4 brick of voxels is one wave64
// (voxel_of's lane order), and the wave walks the tree over the instances and the hierarchies of the instances it enters ONCE
// for its 64 centres. The link is wave-uniform (readfirstlane): a top-level node, a table row, a hierarchy's constants and
// record and a leaf's triangle are fetched once per wave, as scalars. Each lane keeps what WorldPointBody<false> (world.hip)
// keeps for one point -- the world centre, its pad, a WorldBest, found, and inside an instance the moved point and its
// PointImage -- and judges every box against its OWN best: world_point_top at the top level (below: WorldPointBody's
// expressions), PointImage::children inside an instance. A child is entered iff some live lane keeps it (__ballot); where both
// are kept, the wave goes first to the one most keeping lanes find nearer (4.30's majority vote). A leaf is accepted with
// WorldPointBody::leaf's comparison. The answer does not depend on which boxes the wave enters beyond a lane's own, nor on the
// order (DESIGN.md 4.31 has the argument). The wave has ONE stack of QSTACK_MAX links in LDS for both levels (top-level links
// carry WORLD_TOP): psm_world_set_instances guarantees depth + deepest + 1 <= QSTACK_MAX, and every push and pop is guarded.
#include <cmath>
#include <cstdio>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"       // PointImage, PointBound, closest_on_tri, inst_point
#include "psm_world_dev.h"       // WorldRow, WorldNode, WorldGridDistArgs, WorldBest, WORLD_TOP, the slacks
#include "psm_world_uni_dev.h"   // uni, uni_ptr, PSM_CONST, words4, floats3

namespace psm {

namespace {

// What a lane keeps of the world at the top level: WorldPointBody's gap2, top and begin's pad (world.hip), restated here
// expression for expression -- lifting them into psm_world_dev.h moved the code of world.hip's three point kernels (the same
// instructions in another order: tools/kernel_diff.py), so world.hip keeps its own. The squared gap from the WORLD point to a
// box grown by the point's own pad; a box at that gap is dropped only beyond WORLD_PSLACK, written as a negation
// so that a NaN keeps it
PSM_D float world_point_gap2(v3 wp, float qpad, float lx, float ly, float lz, float hx, float hy, float hz) {
    const float tx = smaxf(smaxf((lx - qpad) - wp.x, wp.x - (hx + qpad)), 0.f);
    const float ty = smaxf(smaxf((ly - qpad) - wp.y, wp.y - (hy + qpad)), 0.f);
    const float tz = smaxf(smaxf((lz - qpad) - wp.z, wp.z - (hz + qpad)), 0.f);
    return (tx * tx + ty * ty) + tz * tz;
}
PSM_D void world_point_top(v3 wp, float qpad, float best, float4 w0, float4 w1, float4 w2, bool& okL, bool& okR, float& kL, float& kR) {
    kL = world_point_gap2(wp, qpad, w0.x, w0.y, w0.z, w0.w, w1.x, w1.y);
    kR = world_point_gap2(wp, qpad, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w);
    const float lim = best + WORLD_PSLACK * best;
    okL = !(kL > lim);
    okR = !(kR > lim);
}
// the pad of a world point: WORLD_QSLACK times its largest |coordinate|
PSM_D float world_point_pad(v3 wp) { return WORLD_QSLACK * smaxf(smaxf(pabs(wp.x), pabs(wp.y)), pabs(wp.z)); }

// One wave per brick, grid-stride over the launch's bricks. RECORDS = false: the dense dist / tri / inst [nz][ny][nx] of the
// whole grid (tri and inst may each be NULL); RECORDS = true: a psm_hit per lane of the launch's bricks in lane order (u = v =
// 0; a dead lane's is a miss) for the sign kernel of world.hip, and the instance straight into the dense inst, which the sign
// does not touch.
// rows: the world's table; nodes: the tree over the instances
template <bool RECORDS>
PSM_D void world_dist_walk(const WorldGridDistArgs& a, const WorldRow* __restrict__ rows, const WorldNode* __restrict__ nodes,
                           float* __restrict__ dist, int32_t* __restrict__ tri, int32_t* __restrict__ oinst, float4* __restrict__ hits) {
    __shared__ int stack[QSTACK_MAX];   // the wave's: every lane writes and reads the same entry
    const int lane = (int)threadIdx.x;
    __builtin_assume(lane >= 0 && lane < QUERY_BLOCK);
    const WorldGridArgs& g = a.g;
    const float rmax = a.rmax;
    for (uint32_t b = blockIdx.x; b < g.bricks; b += gridDim.x) {
        // (voxel_of's lane order, psm_grid_dev.h, over the brick first + b of the grid)
        const uint32_t gb = a.first + b;
        const uint32_t bx = gb % g.nbx, bt = gb / g.nbx, by = bt % g.nby, bz = bt / g.nby;
        const uint32_t ix = 4u * bx + ((uint32_t)lane & 3u), iy = 4u * by + (((uint32_t)lane >> 2) & 3u), iz = 4u * bz + ((uint32_t)lane >> 4);
        const bool inside = ix < g.nx && iy < g.ny && iz < g.nz;
        // the centre as grid_centres writes it (grid.hip): one operation per rounding
        const v3 wp = mk3(g.ox + ((float)ix + 0.5f) * g.cx, g.oy + ((float)iy + 0.5f) * g.cy, g.oz + ((float)iz + 0.5f) * g.cz);
        const float qpad = world_point_pad(wp);
        const bool valid = inside && finite3(wp);   // (WorldPointBody::begin's; rmax was checked on the host)
        // per brick: the grid-stride loop comes here again
        WorldBest best;
        best.clear((rmax * rmax) * 1.00000095367431640625f + 0x1p-126f);   // fl(rmax^2) (1 + 2^-20) + 2^-126 (PointBody::begin)
        bool found = false;
        // the instance the wave is in: its records, its triangles, its bound; the lane's moved point and image in it
        const PSM_CONST uint32_t* node32 = nullptr;
        const PSM_CONST uint32_t* tri48 = nullptr;
        PointBound B = {};
        PointImage P = {};
        v3 p = mk3(0.f, 0.f, 0.f);
        bool here = false;   // live in this instance: valid, and the moved point is finite (WorldPointBody::enter's -1)
        int inst = -1;
        int cur = g.root < 0 ? g.root : (g.root | WORLD_TOP), sp = 0;
        if (__ballot(valid) != 0ull) {
            for (;;) {
                cur = __builtin_amdgcn_readfirstlane(cur);
                int t0 = -1, t1 = -1;   // the leaves to test, wave-uniform
                bool pop = false;
                if (cur < 0) {
                    // an instance is entered: its row and its hierarchy's constants once for the wave, every lane's point moved
                    // as WorldPointBody::enter moves it
                    inst = ~cur;
                    const uint4* rp = (const uint4*)(rows + inst);
                    const uint4 ra = rp[0], rb = rp[1], rc = rp[2], rd = rp[3], re = rp[4];
                    node32 = uni_ptr(ra.x, ra.y);
                    tri48 = uni_ptr(ra.z, ra.w);
                    const PSM_CONST uint32_t* sm = uni_ptr(rb.x, rb.y);
                    const PSM_CONST uint32_t* sorted_tri = uni_ptr(rb.z, rb.w);
                    float m[12];
                    m[0] = u2f(uni(rc.x)); m[1] = u2f(uni(rc.y)); m[2] = u2f(uni(rc.z)); m[3] = u2f(uni(rc.w));
                    m[4] = u2f(uni(rd.x)); m[5] = u2f(uni(rd.y)); m[6] = u2f(uni(rd.z)); m[7] = u2f(uni(rd.w));
                    m[8] = u2f(uni(re.x)); m[9] = u2f(uni(re.y)); m[10] = u2f(uni(re.z)); m[11] = u2f(uni(re.w));
                    float M[16];
#pragma unroll
                    for (int k = 0; k < 16; k++) M[k] = u2f(sm[SM_M + k]);
                    p = inst_point(m, wp);
                    B = point_bound(M);
                    P.set(M, p);
                    here = valid && finite3(p);
                    pop = true;
                    if (__ballot(here) != 0ull) {
                        const int root = (int)uni(sm[SM_ROOT]);
                        if (uni(sm[SM_COUNT]) == 1u) t0 = (int)uni(sorted_tri[0]);   // one leaf: no tree
                        if (root >= 0) {
                            cur = root;
                            pop = false;
                        }
                    }
                } else if (cur & WORLD_TOP) {
                    const WorldNode* np = (const WorldNode*)((const char*)nodes + ((size_t)(uint32_t)(cur & ~WORLD_TOP) << 6));
                    const float4 w0 = np->w0, w1 = np->w1, w2 = np->w2;
                    const int4 w3 = np->w3;
                    bool keepL, keepR;
                    float kL, kR;
                    world_point_top(wp, qpad, best.best, w0, w1, w2, keepL, keepR, kL, kR);   // (WorldPointBody::top's expressions)
                    const unsigned long long mL = __ballot(keepL && valid), mR = __ballot(keepR && valid);
                    const bool okL = mL != 0ull, okR = mR != 0ull;
                    const int lx = (int)uni((uint32_t)w3.x), ly = (int)uni((uint32_t)w3.y);
                    const int lkL = lx < 0 ? lx : (lx | WORLD_TOP), lkR = ly < 0 ? ly : (ly | WORLD_TOP);
                    // nearer child first, by the majority of the lanes that keep one
                    const unsigned long long nearL = __ballot(valid && (keepL || keepR) && kL <= kR);
                    const bool leftFirst = okL && (!okR || 2 * __popcll(nearL) >= __popcll(mL | mR));
                    const int first = leftFirst ? lkL : lkR, second = leftFirst ? lkR : lkL;
                    if (okL && okR) {
                        // (sp < QSTACK_MAX always: psm_world_set_instances refuses a world whose two depths exceed it. The test
                        // keeps every store and every pop inside the array)
                        if (sp < QSTACK_MAX) {
                            stack[sp] = second;
                            sp++;
                        }
                    }
                    cur = first;
                    pop = !(okL || okR);
                } else {
                    // grid_dist.hip's node step: each lane judges both children against its own best
                    const PSM_CONST uint32_t* np = node32 + ((size_t)(uint32_t)cur << 3);   // (a record is 32 bytes)
                    const uint4 n0 = words4(np), n1 = words4(np + 4);
                    const int lkx = (int)uni(n1.z), lky = (int)uni(n1.w);
                    bool keepL, keepR;
                    float kL, kR;
                    P.children(B, n0, n1, best.best, keepL, keepR, kL, kR);
                    const unsigned long long mL = __ballot(keepL && here), mR = __ballot(keepR && here);
                    const bool okL = mL != 0ull, okR = mR != 0ull;
                    const bool leafL = okL && lkx < 0, leafR = okR && lky < 0;
                    t0 = leafL ? ~lkx : (leafR ? ~lky : -1);
                    t1 = (leafL && leafR) ? ~lky : -1;
                    const bool intL = okL && !leafL, intR = okR && !leafR;
                    const unsigned long long nearL = __ballot(here && (keepL || keepR) && kL <= kR);
                    const bool leftFirst = intL && (!intR || 2 * __popcll(nearL) >= __popcll(mL | mR));
                    const int first = leftFirst ? lkx : lky, second = leftFirst ? lky : lkx;
                    if (intL && intR) {
                        if (sp < QSTACK_MAX) {
                            stack[sp] = second;
                            sp++;
                        }
                    }
                    cur = first;
                    pop = !(intL || intR);
                }
                // the accepted leaves, one test after the other: the triangle is loaded once for the wave
                while (t0 >= 0) {
                    const int id = __builtin_amdgcn_readfirstlane(t0);
                    const PSM_CONST uint32_t* tp = tri48 + (size_t)12 * (size_t)(uint32_t)id;   // (v0, e1, e2: a float4 each)
                    float u, w;
                    const float d2 = closest_on_tri(floats3(tp), floats3(tp + 4), floats3(tp + 8), p, u, w);
                    // (WorldPointBody::leaf, compare for compare)
                    if (here && sqrtf(d2) <= rmax && best.wins(d2, inst, id)) {
                        found = true;
                        best.take(d2, 0.f, 0.f, inst, id);
                    }
                    t0 = t1;
                    t1 = -1;
                }
                if (pop) {
                    if (sp == 0) break;
                    sp--;
                    cur = stack[sp];
                }
            }
        }
        const float t = found ? sqrtf(best.best) : __builtin_inff();
        const size_t i = ((size_t)iz * g.ny + iy) * g.nx + ix;
        if (RECORDS) {
            hits[(size_t)b * QUERY_BLOCK + lane] = make_float4(0.f, 0.f, t, __int_as_float(best.btri));
        } else {
            if (inside) dist[i] = t;
            if (tri) {
                if (inside) tri[i] = best.btri;
            }
        }
        if (oinst) {
            if (inside) oinst[i] = best.binst;
        }
    }
}

}  // namespace

// the bound of the other kernels of a world (128 VGPRs: DESIGN.md 4.31 has what hipcc takes)
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_grid_dist_dense(WorldGridDistArgs a, const WorldRow* __restrict__ rows,
                                                                        const WorldNode* __restrict__ nodes, float* __restrict__ dist,
                                                                        int32_t* __restrict__ tri, int32_t* __restrict__ inst) {
    world_dist_walk<false>(a, rows, nodes, dist, tri, inst, nullptr);
}
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_grid_dist_records(WorldGridDistArgs a, const WorldRow* __restrict__ rows,
                                                                          const WorldNode* __restrict__ nodes, float4* __restrict__ hits,
                                                                          int32_t* __restrict__ inst) {
    world_dist_walk<true>(a, rows, nodes, nullptr, nullptr, inst, hits);
}

// world.hip's host path (world_grid_dist_query(): the checks, the empty world, the stale refusal, the slabs) launches through this
int world_grid_dist_launch(psm_ctx* c, uint32_t grid, const WorldGridDistArgs& a, const WorldRow* rows, const WorldNode* nodes, float* dist,
                           int32_t* tri, int32_t* inst, void* hits) {
    if (hits) world_grid_dist_records<<<grid, QUERY_BLOCK, 0, c->stream>>>(a, rows, nodes, (float4*)hits, inst);
    else world_grid_dist_dense<<<grid, QUERY_BLOCK, 0, c->stream>>>(a, rows, nodes, dist, tri, inst);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace psm
