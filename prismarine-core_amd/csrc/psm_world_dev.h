// psm_world_dev.h -- the device pieces the kernel files of a world share (world.hip, world_box.hip, world_sweep.hip,
// world_tri.hip, world_tri_dist.hip, world_mesh.hip, world_mesh_dist.hip, world_grid.hip, world_grid_dist.hip): the table row, the node of the tree over the instances, the kernel arguments, the padding and the slacks,
// the two-level walk, the loads of a row, the best record of a world (WorldBest) and a ray in a world (WorldRay). Moved here
// from world.hip as they were; every kernel of world.hip compiles to the same instructions as with the pieces in its own file
// (tools/kernel_diff.py; the digests of tests/test_world_query_cpu.py and tests/test_world_kbest_cpu.py).
#pragma once
#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"

namespace psm {

// one instance as the kernels read it: 80 B, 16-byte aligned (five 16-byte loads)
struct WorldRow {
    const uint4* node32;
    const float4* tri48;
    const uint32_t* sm;
    const int32_t* sorted_tri;
    float m[12];   // psm_instance.world_from_object
};
static_assert(sizeof(WorldRow) == 80, "a table row is 80 bytes");

// a node of the tree over the instances, 64 B: both children's float32 boxes and two links (>= 0: a node, < 0: ~instance)
//   w0 = L.lo.xyz L.hi.x | w1 = L.hi.yz R.lo.xy | w2 = R.lo.z R.hi.xyz | w3 = linkL linkR 0 0
struct WorldNode {
    float4 w0, w1, w2;
    int4 w3;
};
static_assert(sizeof(WorldNode) == 64, "a node record is 64 bytes");

struct WorldArgs {
    const float4* rays;      // as QueryArgs
    size_t n;
    int* spill;
    float4* hits;
    uint8_t* occluded;
    uint32_t* count;
    int32_t* geom;           // the winning instance per query, -1 on a miss
    uint32_t samples;
    int root;                // 0: the tree's root node; < 0: ~instance of a world of one
    const WorldRow* rows;
    const WorldNode* nodes;
};

// world_box.hip: the launch of a world's box kernel (mode: 0 overlaps, 1 count, 2 triangles) for world.hip's host path; a.rays
// holds the boxes where a ray's two float4 are, a.samples is the triangles query's k, a.hits its [n][k] int32 triangle rows,
// a.geom its [n][k] instance rows, a.count the counts
int world_box_launch(psm_ctx* c, int mode, uint32_t grid, const WorldArgs& a);

// world_tri.hip: the launch of a world's triangle kernel (mode: 0 overlaps, 1 count, 2 triangles) for world.hip's host path;
// a.rays holds the query triangles (psm_tri_query: three float4 each), the rest as world_box_launch
int world_tri_launch(psm_ctx* c, int mode, uint32_t grid, const WorldArgs& a);

// world_tri_dist.hip: the launch of a world's clearance kernel (within: whether a pair is within rmax; else the nearest pair) for
// world.hip's host path; a.rays holds the query triangles (psm_tri_dist_query: three float4 each, rmax in the first's w), a.hits
// the psm_tri_hit records (two float4 each) and a.geom the instances, or a.occluded the flags. a.rows == NULL (a world without
// instances): the closest query's miss records are written and nothing walks
int world_tri_dist_launch(psm_ctx* c, bool within, uint32_t grid, const WorldArgs& a);

// world_sweep.hip: the launch of a world's sweep kernel (any: whether there is a contact; else the first contact) for
// world.hip's host path; a.rays holds the sweeps (psm_sweep_query) where a ray's two float4 are
int world_sweep_launch(psm_ctx* c, bool any, uint32_t grid, const WorldArgs& a);

// WorldArgs keeps its layout; what a mesh query over a world (world_mesh.hip) adds travels beside it. w: the
// world, spill and outputs (occluded: the flag per pose; count: [p][T]; hits / geom: the int32 [p][T][k] rows), samples = k,
// n = p x L; rays is not read
struct WorldMeshArgs {
    WorldArgs w;
    const float4* tri48;        // the other hierarchy's v0, e1, e2 per triangle
    const int32_t* leaf_tri;    // ... and its leaves in slot order: leaf j is triangle leaf_tri[j], ascending
    const float4* poses;        // [p] x three float4: the rows of [R | T], other's object space into world space
    uint64_t magic;             // mesh_magic(L)
    uint32_t L, T;              // the other's leaf count and loaded triangle count
    uint32_t flags;             // WORLD_MESH_FLAG_*
    int32_t skip;               // the instance that is never entered, -1: none
};
constexpr uint32_t WORLD_MESH_FLAG_SKIP = 1u;   // the flag kernel: a lane whose pose's flag already reads 1 does not walk
// (the most answers, poses x triangles, of one call is psm_mesh_dev.h's MESH_QUERIES_MAX: the kernels index them with 32 bits)

// world_mesh.hip: the launch of a world's mesh kernel (mode: 0 overlaps, 1 count, 2 triangles) for world.hip's host path
// (world_mesh_query()); a.w.samples is the triangles query's k; magic is set there from a.L (mesh_magic, psm_mesh_dev.h)
int world_mesh_launch(psm_ctx* c, int mode, uint32_t grid, WorldMeshArgs a);

// WorldMeshArgs keeps its layout; what a mesh clearance query over a world (world_mesh_dist.hip) adds travels
// beside it. m.w: the world, spill and outputs (closest: hits = psm_tri_hit [p][T], geom [p][T]; within: occluded, the flag per
// pose; pick: hits = psm_mesh_hit [p], geom [p]), n = p x L (pick: p); m.flags: WORLD_MESH_FLAG_SKIP for the within kernel
struct WorldMeshDistArgs {
    WorldMeshArgs m;
    unsigned long long* keys;   // [p]: the poses' shared words (clearance, pick; psm_mesh_dist_key.h)
    float rmax;                 // one per call
};
enum { WMD_CLOSEST = 0, WMD_WITHIN = 1, WMD_CLEAR = 2, WMD_PICK = 3, WMD_FILL = 4 };

// world_mesh_dist.hip: the launch of a world's mesh clearance kernel for world.hip's host path (world_mesh_dist_query()); magic is
// set there from a.m.L. mode WMD_CLEAR: bound is PSM_MESH_BOUND's letter ('0' .. '3'; mesh.hip's mesh_bound() has the meanings). mode
// WMD_FILL: the miss record in a.m.w.n cells of hits (the word after s, t: -1 where the records are psm_mesh_hit, `pick`) and -1 in geom
int world_mesh_dist_launch(psm_ctx* c, int mode, char bound, bool pick, uint32_t grid, WorldMeshDistArgs a);

// A voxel grid over a world (world_grid.hip): the grid's nine numbers, its bricks, the world's root. The table
// and the tree travel beside it as kernel parameters of their own
struct WorldGridArgs {
    float ox, oy, oz, cx, cy, cz;   // psm_grid: origin, cell
    uint32_t nx, ny, nz;            // ... dims
    uint32_t nbx, nby;              // bricks along x and y
    uint32_t bricks;                // all of them: one launch
    int root;                       // as WorldArgs
};
enum { WGRID_SURFACE = 0, WGRID_COUNTS = 1, WGRID_INSTANCES = 2 };

// world_grid.hip: the launch of a world's grid kernel for world.hip's host path (world_grid_query()). out: a uint64_t word per
// brick (WGRID_SURFACE), the dense uint32_t [nz][ny][nx] counts (WGRID_COUNTS) or int32_t labels (WGRID_INSTANCES)
int world_grid_launch(psm_ctx* c, int mode, uint32_t grid, const WorldGridArgs& g, const WorldRow* rows, const WorldNode* nodes, void* out);

// A distance-field grid over a world (world_grid_dist.hip): WorldGridArgs, whose `bricks` is then the launch's own,
// the first brick of the launch (signed works a slab at a time) and the call's one rmax
struct WorldGridDistArgs {
    WorldGridArgs g;
    uint32_t first;                 // the bricks [first, first + g.bricks) of the grid are this launch's
    float rmax;
};

// world_grid_dist.hip: the launch of a world's distance-field kernel for world.hip's host path (world_grid_dist_query()).
// hits == NULL: the dense float32 dist and int32 tri / inst [nz][ny][nx] of the whole grid (tri and inst may each be NULL);
// else a psm_hit per lane of the launch's bricks in lane order into hits (u = v = 0, a miss for a dead lane) for the world's sign
// kernel, and the instance straight into the dense inst (may be NULL); dist and tri are then not read
int world_grid_dist_launch(psm_ctx* c, uint32_t grid, const WorldGridDistArgs& a, const WorldRow* rows, const WorldNode* nodes, float* dist,
                           int32_t* tri, int32_t* inst, void* hits);

namespace {

constexpr int WORLD_TOP = 0x40000000;  // tag of a top-level node link (hierarchy node links stay below 2^28)

// The padding and the slacks (DESIGN.md 4.11 has the derivation). The box test works on the world query and the forward image
// of the object box, T + R box; the candidate test on the query moved by inst_point / inst_rotate, R^T (x - T). They differ by
//   * the move's rounding: one subtraction, three products, two sums per coordinate: <= 4 eps sqrt 3 (|x| + |T|) ~ 4.2e-7 (...)
//   * R^T R = 1 + E, |E_ij| <= 1e-5 (pose_fault): R^-T - R = -R E (1 + E)^-1, a displacement of <= 3e-5 sqrt 3 = 5.2e-5 times
//     the largest object coordinate, and |R^T d| = 1 +- 1.5e-5: world distances are object distances to 1.5e-5 (squares: 3e-5)
//   * tri_query's 1e-5 tolerance on u, v, u + v: a counted crossing lies within 1e-5 of an edge length (<= 2 sqrt 3 times the
//     largest object coordinate) of its triangle: 3.5e-5
// in all <= 8.8e-5 S in position, S the largest of: the object box's largest |coordinate|, |T|, the world box's largest
// |coordinate| -- plus 4.2e-7 of the query's largest |coordinate|. WORLD_PAD = WORLD_QSLACK = 2^-11 = 4.9e-4 (5.5x and > 1000x).
// Distances: WORLD_TSLACK = 2^-12 = 2.4e-4 on t (16x 1.5e-5), WORLD_PSLACK = 2^-11 on d2 (16x 3e-5).
constexpr float WORLD_PAD = 0x1p-11f;      // a leaf box grows by WORLD_PAD * S + WORLD_FLOOR on every side
constexpr float WORLD_FLOOR = 0x1p-100f;   // ... so no box is ever degenerate (the NaN argument at WorldRay::slab)
constexpr float WORLD_QSLACK = 0x1p-11f;   // ... and by WORLD_QSLACK * the query's largest |coordinate| at the test
constexpr float WORLD_TSLACK = 0x1p-12f;   // a ray's prune against best / tmax / tmin: relative
constexpr float WORLD_PSLACK = 0x1p-11f;   // a point's prune against best d2 / rmax^2: relative

// ---- the two-level walk --------------------------------------------------------------------------------------------------------

// The body:
//   bool begin(i, alive)     load query i, clear the running state, set up the WORLD query the top level tests; false: a miss
//   void top(w0, w1, w2, okL, okR, kL, kR)   a top-level node's two boxes: kept or not, and the order key (nearer first)
//   int  enter(inst)         load the instance's row, move the query (re-read from memory, as 4.9), do the per-geometry set-up,
//                            test the lone leaf of a one-leaf hierarchy; returns the hierarchy's root to walk, -1 for none
//                            (fewer than two leaves, or the moved query is invalid in this instance)
//   children, leaf, done, again, finish: as query.hip's scene_walk
// Every loop here is bounded: the node loop by the two trees (each iteration visits a node or an instance once per walk), the
// leaf loop by two, the outer ones by the batch and the sample count.
template <class Body>
PSM_D void world_walk(const WorldArgs& w, Body& q) {
    __shared__ int stack[QSTACK_LDS][QUERY_BLOCK];
    const int lane = (int)threadIdx.x;
    __builtin_assume(lane >= 0 && lane < QUERY_BLOCK);
    const size_t spill_stride = (size_t)gridDim.x * QUERY_BLOCK;
    int* __restrict__ spill = w.spill + (size_t)blockIdx.x * QUERY_BLOCK + lane;
    for (size_t i = (size_t)blockIdx.x * QUERY_BLOCK + (size_t)lane; i - (size_t)lane < w.n; i += spill_stride) {
        const bool alive = i < w.n;
        const bool valid = q.begin(i, alive);
        do {
            int cur = w.root < 0 ? w.root : (w.root | WORLD_TOP), sp = 0;
            bool walking = valid;
            while (walking) {
                bool pop = false;
                if (cur < 0) {
                    const int r = q.enter(~cur);
                    pop = r < 0;
                    cur = r;
                } else if (cur & WORLD_TOP) {
                    const WorldNode* np = (const WorldNode*)((const char*)w.nodes + ((size_t)(uint32_t)(cur & ~WORLD_TOP) << 6));
                    const float4 w0 = np->w0, w1 = np->w1, w2 = np->w2;
                    const int4 w3 = np->w3;
                    bool okL, okR;
                    float kL, kR;
                    q.top(w0, w1, w2, okL, okR, kL, kR);
                    const int lkL = w3.x < 0 ? w3.x : (w3.x | WORLD_TOP), lkR = w3.y < 0 ? w3.y : (w3.y | WORLD_TOP);
                    const bool leftFirst = okL && (!okR || kL <= kR);   // nearer child first
                    const int first = leftFirst ? lkL : lkR, second = leftFirst ? lkR : lkL;
                    if (okL && okR) {
                        // (sp < QSTACK_MAX always: psm_world_set_instances refuses a world whose two depths exceed it)
                        if (sp < QSTACK_LDS) stack[sp][lane] = second;
                        else if (sp < QSTACK_MAX) spill[(size_t)(sp - QSTACK_LDS) * spill_stride] = second;
                        sp++;
                    }
                    cur = first;
                    pop = !(okL || okR);
                } else {
                    const uint4* np = (const uint4*)((const char*)q.node32 + ((uint32_t)cur << 5));
                    const uint4 n0 = np[0], n1 = np[1];
                    const int lkx = (int)n1.z, lky = (int)n1.w;
                    bool okL, okR;
                    float kL, kR;
                    q.children(n0, n1, okL, okR, kL, kR);
                    const bool leafL = okL && lkx < 0, leafR = okR && lky < 0;
                    int t0 = leafL ? ~lkx : (leafR ? ~lky : -1);
                    int t1 = (leafL && leafR) ? ~lky : -1;
                    while (t0 >= 0) {
                        q.leaf(t0);
                        t0 = t1;
                        t1 = -1;
                    }
                    const bool intL = okL && !leafL, intR = okR && !leafR;
                    const bool leftFirst = intL && (!intR || kL <= kR);
                    const int first = leftFirst ? lkx : lky, second = leftFirst ? lky : lkx;
                    if (intL && intR) {
                        if (sp < QSTACK_LDS) stack[sp][lane] = second;
                        else if (sp < QSTACK_MAX) spill[(size_t)(sp - QSTACK_LDS) * spill_stride] = second;
                        sp++;
                    }
                    cur = first;
                    pop = !(intL || intR);
                }
                if (q.done()) break;
                if (pop) {
                    if (sp == 0) break;
                    sp--;
                    cur = sp < QSTACK_LDS ? stack[sp][lane] : spill[(size_t)(sp - QSTACK_LDS) * spill_stride];
                }
            }
        } while (q.again());
        if (alive) q.finish(i);
    }
}

// the row of instance `in`, by five aligned 16-byte loads; the lane keeps the two pointers its walk needs
struct RowLoad {
    const uint32_t* sm;
    const int32_t* sorted_tri;
    float m[12];
};
template <class Q>
PSM_D RowLoad load_row(const WorldArgs& w, int in, Q& q) {
    const uint4* rp = (const uint4*)(w.rows + in);
    const uint4 a = rp[0], b = rp[1], c = rp[2], d = rp[3], e = rp[4];
    q.node32 = (const uint4*)(((uint64_t)a.y << 32) | a.x);
    q.tri48 = (const float4*)(((uint64_t)a.w << 32) | a.z);
    q.inst = in;
    RowLoad r;
    r.sm = (const uint32_t*)(((uint64_t)b.y << 32) | b.x);
    r.sorted_tri = (const int32_t*)(((uint64_t)b.w << 32) | b.z);
    r.m[0] = u2f(c.x); r.m[1] = u2f(c.y); r.m[2] = u2f(c.z); r.m[3] = u2f(c.w);
    r.m[4] = u2f(d.x); r.m[5] = u2f(d.y); r.m[6] = u2f(d.z); r.m[7] = u2f(d.w);
    r.m[8] = u2f(e.x); r.m[9] = u2f(e.y); r.m[10] = u2f(e.z); r.m[11] = u2f(e.w);
    return r;
}

// what finish() needs of the row of instance `in`: the triangles and the pose
PSM_D const float4* load_pose(const WorldArgs& w, uint32_t in, float* m) {
    const uint4* rp = (const uint4*)(w.rows + in);
    const uint4 a = rp[0], c = rp[2], d = rp[3], e = rp[4];
    m[0] = u2f(c.x); m[1] = u2f(c.y); m[2] = u2f(c.z); m[3] = u2f(c.w);
    m[4] = u2f(d.x); m[5] = u2f(d.y); m[6] = u2f(d.z); m[7] = u2f(d.w);
    m[8] = u2f(e.x); m[9] = u2f(e.y); m[10] = u2f(e.z); m[11] = u2f(e.w);
    return (const float4*)(((uint64_t)a.w << 32) | a.z);
}

// The best record of a world (closest hit and closest point; `best` is t or d2). The tree visits the instances in tree order,
// so SceneBest's one-key trick does not carry over: a candidate (x, inst, tri) wins iff x < best, or x == best and (inst, tri)
// is lexicographically lower than the record's (no record: binst = btri = -1, the largest as unsigned). Boxes are kept with <=.
struct WorldBest {
    float best, bu, bv;
    int btri, binst;
    PSM_D void clear(float bound) {
        best = bound;
        bu = 0.f;
        bv = 0.f;
        btri = -1;
        binst = -1;
    }
    PSM_D bool wins(float x, int inst, int tri) const {
        return x < best || (x == best && ((uint32_t)inst < (uint32_t)binst || (inst == binst && (uint32_t)tri < (uint32_t)btri)));
    }
    PSM_D void take(float x, float u, float v, int inst, int tri) {
        best = x;
        bu = u;
        bv = v;
        btri = tri;
        binst = inst;
    }
};

// A ray in a world: the object-space ray of the instance the lane is in (query.hip's SceneRay) and the WORLD ray the top level
// tests: origin, reciprocal of the unit direction (normalize3 of the direction as given: SceneRay::aim's), the query's pad.
struct WorldRay {
    const uint4* node32;
    const float4* tri48;
    int inst;
    v3 o, d;
    float tmin, tmax;
    Axis X, Y, Z;
    v3 wo, wiv;
    float qpad;
    bool nocull;   // the world direction is no unit vector (zero, non-finite, overflowed): every box is kept

    PSM_D void world_ray(v3 orig, v3 dir) {
        wo = orig;
        const v3 dn = normalize3(dir);
        nocull = !(finite3(dn) && dot3(dn, dn) > 0.5f);
        wiv = mk3(1.0f / dn.x, 1.0f / dn.y, 1.0f / dn.z);   // (+-inf for an axis-aligned ray)
        qpad = WORLD_QSLACK * smaxf(smaxf(pabs(orig.x), pabs(orig.y)), pabs(orig.z));
    }
    // The slab test of a world box, grown by qpad. minNum / maxNum: on an axis the ray is parallel to, wiv is
    // +-inf and a plane distance is -inf, +inf or (the origin exactly in the plane: 0 x inf) NaN, which sminf / smaxf ignore.
    // "Passes a leaf's box => passes every ancestor's": an inner box is the exact min / max union of leaf boxes, float
    // subtraction and multiplication by one factor are monotone, so on an axis with a finite wiv an ancestor's interval
    // contains the leaf's. On a parallel axis a leaf passes only with its origin strictly between the grown planes (-inf, +inf:
    // no constraint) -- a leaf box has lo < hi on every axis (WORLD_FLOOR), so one NaN always comes with an infinity of the
    // failing sign, and two NaN never -- and strictly between a leaf's planes is strictly between every ancestor's.
    PSM_D void slab(float lx, float ly, float lz, float hx, float hy, float hz, float& tNear, float& tFar) const {
        const float ax = ((lx - qpad) - wo.x) * wiv.x, bx = ((hx + qpad) - wo.x) * wiv.x;
        const float ay = ((ly - qpad) - wo.y) * wiv.y, by = ((hy + qpad) - wo.y) * wiv.y;
        const float az = ((lz - qpad) - wo.z) * wiv.z, bz = ((hz + qpad) - wo.z) * wiv.z;
        tNear = smaxf(smaxf(sminf(ax, bx), sminf(ay, by)), sminf(az, bz));
        tFar = sminf(sminf(smaxf(ax, bx), smaxf(ay, by)), smaxf(az, bz));
    }
    // both boxes of a top-level node against [tmin, lim], slackened; written as negations so that a NaN bound keeps the box
    PSM_D void top_boxes(float4 w0, float4 w1, float4 w2, float lim, bool& okL, bool& okR, float& nL, float& nR) const {
        float fL, fR;
        slab(w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, nL, fL);
        slab(w1.z, w1.w, w2.x, w2.y, w2.z, w2.w, nR, fR);
        const float hi = lim + WORLD_TSLACK * pabs(lim), lo = tmin - WORLD_TSLACK * pabs(tmin);
        okL = nocull | (!(nL > fL) & !(nL > hi) & !(fL < lo));
        okR = nocull | (!(nR > fR) & !(nR > hi) & !(fR < lo));
    }
    // enter(): the world ray (orig, dir as given) moved into instance `in` as query.hip's inst_ray moves it, then the axes
    PSM_D int enter_ray(const WorldArgs& w, int in, v3 orig, v3 dir, const int32_t*& sorted_tri, uint32_t& count) {
        const RowLoad r = load_row(w, in, *this);
        o = inst_point(r.m, orig);
        d = normalize3(inst_rotate(r.m, dir));
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(r.sm[SM_M + k]);
        X = ray_axis(M, 0, o, d);
        Y = ray_axis(M, 1, o, d);
        Z = ray_axis(M, 2, o, d);
        sorted_tri = r.sorted_tri;
        count = r.sm[SM_COUNT];
        const int root = (int)r.sm[SM_ROOT];
        return (finite3(o) && finite3(d)) ? (root >= 0 ? root : -2) : -1;   // -2: valid here, no tree (0 or 1 leaves)
    }
    // begin() of the bodies whose query is a ray: the window and the world ray (a dead lane: an empty window)
    PSM_D void begin_ray(const WorldArgs& w, size_t i, bool al) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = make_float4(1.f, 0.f, 0.f, -1.f);
        if (al) { r0 = w.rays[2 * i]; r1 = w.rays[2 * i + 1]; }
        tmin = r0.w;
        tmax = r1.w;
        world_ray(mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z));
    }
    PSM_D void boxes(uint4 n0, uint4 n1, float lim, bool& okL, bool& okR, float& nL, float& nR) const {
        float fL, fR;
        psm::slab(X, Y, Z, half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z), nL, fL);
        psm::slab(X, Y, Z, half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y), nR, fR);
        okL = (nL <= fL) & (nL <= lim) & (fL >= tmin);
        okR = (nR <= fR) & (nR <= lim) & (fR >= tmin);
    }
};

}  // namespace

}  // namespace psm
