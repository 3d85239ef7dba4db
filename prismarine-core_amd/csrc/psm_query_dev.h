// psm_query_dev.h -- the device pieces every query kernel file shares (query.hip, kbest.hip, world.hip): the constants of the
// walk, the kernel arguments, the triangle and box tests of rays and points, the move into an instance's object space, the
// directions of the inside test, and the single-hierarchy walk itself. Moved here from query.hip as they were; every kernel of
// the three files compiles to the same instructions as with the pieces in its own file (tools/kernel_diff.py; query.hip's 21
// are hashed by tests/test_world_query_cpu.py).
#pragma once
#include "psm_common.h"
#include "psm_internal.h"

namespace psm {

constexpr int SM_M = 0;        // bvh.hip: the fit transform (16 floats, row-major)
constexpr int SM_COUNT = 24;   // bvh.hip: leaf count
constexpr int SM_ROOT = 25;    // bvh.hip: root link (-1: fewer than two leaves)

constexpr int QUERY_BLOCK = 64;          // one wave per workgroup (rt_traverse: TRAV_BLOCK)
constexpr int QSTACK_LDS = 16;           // stack entries per lane in LDS: 4 KB per wave, as rt_traverse's
// The builder's height bound (bvh_emit): above a run of equal Morton codes every internal node's range shares a strictly longer
// key prefix than its parent's (the split is the highest differing bit), and a 63-bit code has prefixes of 1..63 bits: at most
// 63 such levels. A run of equal codes is split at the median (findSplit), ceil(log2 N) more levels for N <= 2^27 leaves. A ray's
// stack holds at most one entry per internal ancestor of its current node: 63 + 27 = 90 entries.
constexpr int QSTACK_MAX = 96;
#ifndef PSM_QUERY_GRID_CAP
#define PSM_QUERY_GRID_CAP 8192
#endif
// workgroups of a launch at most: 32 waves per CU, all the chip holds at 8 waves per SIMD (4096: 0.54 / 1.41 ms against 0.49 / 0.99 ms for
// 2 M primary / bounce rays, profiles/query_r06.txt); the spill area has a lane for each (80 x 8192 x 64 x 4 B = 168 MB per context)
constexpr uint32_t QUERY_GRID_CAP = PSM_QUERY_GRID_CAP;

struct QueryArgs {
    const float4* rays;      // psm_query_ray: origin.xyz tmin | direct.xyz tmax (ray kernels) / psm_point_query: p.xyz rmax (point kernels)
    size_t n;
    const uint4* node32;     // the build's traversal records (bvh_emit)
    const float4* tri48;     // v0, e1, e2 per triangle (bvh_prepare_tris / bvh_load_mesh)
    const uint32_t* sm;      // transform, leaf count, root
    const int32_t* sorted_tri;  // [0]: the lone leaf's triangle when the leaf count is 1 (bvh_segtree<true> writes it)
    int* spill;              // [QSTACK_MAX - QSTACK_LDS][gridDim.x * 64]
    float4* hits;            // closest hit / closest point: psm_hit per query (signed distance: read, and t rewritten)
    uint8_t* occluded;       // any hit / within / inside: 0 / 1 per query
    uint32_t* count;         // hit count: crossings per ray
    uint32_t samples;        // inside / signed distance: rays per point (1, 3 or 5)
};

// kbest.hip: the launch of a k-best kernel (points: nearest, else first hits) for query.hip's host path; a.samples is k
int kbest_launch(psm_ctx* c, bool points, uint32_t grid, const QueryArgs& a);
// box.hip: the launch of a box kernel (mode: 0 overlaps, 1 count, 2 triangles) for query.hip's host path; a.rays holds the boxes
// where a ray's two float4 are, a.samples is the triangles query's k
int box_launch(psm_ctx* c, int mode, uint32_t grid, const QueryArgs& a);
// sweep.hip: the launch of a sweep kernel (any: whether there is a contact, else the first) for query.hip's host path; a.rays holds
// the sweeps where a ray's two float4 are
int sweep_launch(psm_ctx* c, bool any, uint32_t grid, const QueryArgs& a);
// tri.hip: the launch of a triangle-query kernel (mode: 0 overlaps, 1 count, 2 triangles) for query.hip's host path; a.rays holds
// the query triangles, three float4 each, a.samples is the triangles query's k
int tri_launch(psm_ctx* c, int mode, uint32_t grid, const QueryArgs& a);
// tri_dist.hip: the launch of a clearance kernel (within: whether a triangle is within rmax, else the nearest) for query.hip's
// host path; a.rays holds the query triangles (psm_tri_dist_query), three float4 each; a.hits two float4 per query
int tri_dist_launch(psm_ctx* c, bool within, uint32_t grid, const QueryArgs& a);

// tri_test (trace.hip) operation for operation, with invDev = 1 / det instead of 1 / (max(|det|, 1e-6) * sign(det)) and without
// its `t >= -PZERO` rule (the caller's window decides). det == 0 is a miss; u, v, u + v keep the 1e-5 tolerances. Where
// |det| >= 1e-6 the values are tri_test's bit for bit. Returns false on a miss; t may be NaN (no window holds it).
PSM_D bool tri_query(const float4* __restrict__ tri48, int tri, v3 orig, v3 dir, float& T, float& U, float& V) {
    const float4 a = tri48[(size_t)3 * tri + 0], b = tri48[(size_t)3 * tri + 1], c = tri48[(size_t)3 * tri + 2];
    const v3 v0 = mk3(a.x, a.y, a.z), e1 = mk3(b.x, b.y, b.z), e2 = mk3(c.x, c.y, c.z);
    const v3 pvec = cross3(dir, e2);
    const float det = dot3(e1, pvec);
    if (pabs(det) <= 0.0f) return false;
    const float invDev = 1.f / det;
    const v3 tvec = orig - v0;
    const float u = dot3(tvec, pvec) * invDev;
    if (u < -0.00001f || u > 1.00001f) return false;
    const v3 qvec = cross3(tvec, e1);
    const float v = dot3(dir, qvec) * invDev;
    if (v < -0.00001f || (u + v) > 1.00001f) return false;
    T = dot3(e2, qvec) * invDev;
    U = u;
    V = v;
    return true;
}

namespace {

PSM_D bool finite3(v3 a) { return __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z); }

// Row k of the build's affine map applied to a point x: P = (M (x, 1)).k in the order mat_vec evaluates it (the w row is never
// read), and the per-axis margin h = 2^-16 (2 + S), S = |m0 x| + |m1 y| + |m2 z| + |m3| (a bound on |P| and on the rounding of its
// sum). Shared by the rays' slabs and the points' gaps.
struct Row {
    float P, h;
};
PSM_D Row affine_row(const float* M, int k, v3 x) {
    const float m0 = M[4 * k + 0], m1 = M[4 * k + 1], m2 = M[4 * k + 2], m3 = M[4 * k + 3];
    Row r;
    r.P = ((m0 * x.x + m1 * x.y) + m2 * x.z) + m3;
    const float S = ((pabs(m0 * x.x) + pabs(m1 * x.y)) + pabs(m2 * x.z)) + pabs(m3);
    r.h = (2.0f + S) * 0x1p-16f;
    return r;
}

// One axis of the ray in the build's normalised space, set up so that a box plane b gives its (inflated) distance in ONE fmaf:
//   P = (M (o, 1)).k, D = (M (d, 0)).k      -- the affine map aabbmaker applied to the vertices (mat_vec with w = 1; the w row is
//                                             never read), applied to the line o + t d: the slab distances are WORLD t
//   lo plane: fmaf(b, inv, nlo) = (b - (P + h)) / D,  hi plane: fmaf(b, inv, nhi) = (b - (P - h')) / D,  h' = h + 2^-12
// i.e. the box grown by h below and h' above (for either sign of D; the constant: further down). h covers the rounding of P, D and the slab arithmetic: each is a
// few ulps of |b| + S (S = |m0 ox| + |m1 oy| + |m2 oz| + |m3| bounds |P| and the rounding of its sum), and the error of D moves the
// plane distance by t |dD| <= 3 eps t sum_j |M_kj d_j|, which for the fit transform (M's 3 x 3 part is diagonal unless the build's
// optimisation matrix rotates) is 3 eps |b - P| <= 3 eps (1 + S). All of it is < 8 eps (2 + S); h = 2^-16 (2 + S) ~ 128 eps (2 + S)
// -- with a 16x margin left for an optimisation matrix whose 3 x 3 part has a condition number up to ~16 (tests/test_ray_prune_cpu.py
// holds the margin to a brute force under rotating, shearing and anisotropic matrices). A box is then dropped only when its exact
// slab interval misses [tmin, limit].
// Which hits lie in their leaf's box: the WELL-POSED ones -- a hit whose point o + t d, mapped by M, is at most 2.5e-4 (PZERO / 2)
// outside its triangle's exact normalised bounding box on every axis (tests/ray_prune_model.py). Where |det| is
// well above its rounding an accepted hit point is within ~1e-5 edge lengths of its triangle (the u, v tolerances) and is
// well-posed; that holds for well-posed hits ONLY: for a ray almost in the triangle's plane det is noise, t with it, and the point
// can be anywhere. Such a hit may be reported or not (it is never invented); only well-posed hits are promised.
// The leaf box is the triangle's padded by PZERO = 5e-4 before the fp16 rounding. In [0.5, 1) that rounding takes at most
// 2^-12 = 2.44e-4 of the padding: >= 2.5e-4 of headroom. But a leaf at the top of the scene has its padded corner in
// [1, 1 + PZERO), where fp16's half-ulp is 2^-11 = 4.88e-4 and the corner can round down to 1.0: as little as 1.2e-5 of the
// padding is left. Only a box's UPPER planes can lie there (a lower corner is a vertex less PZERO: below 1, and fp16 is finer
// toward 0), so the hi plane's margin carries the constant 2^-12 on top of h (1.2e-5 + 2^-12 > 2.5e-4) and the lo plane's is h
// alone: the box grown so holds every well-posed hit of its triangle wherever the box lies. (Without the constant a window
// tmin = tmax = t lost such a hit on the deep fixture under a build matrix: DESIGN.md 4.5.) The points' gaps keep h alone: they
// measure distances to the triangles themselves, which the boxes hold exactly.
// A direction component under 1e-20 in magnitude is taken as +-1e-20 (no infinite reciprocal): the line moves by t * 1e-20,
// below h for every t < 1e15.
struct Axis {
    float inv, nlo, nhi;
};
PSM_D Axis ray_axis(const float* M, int k, v3 o, v3 d) {
    const float m0 = M[4 * k + 0], m1 = M[4 * k + 1], m2 = M[4 * k + 2];
    const Row r = affine_row(M, k, o);
    float D = (m0 * d.x + m1 * d.y) + m2 * d.z;
    if (!(pabs(D) >= 1e-20f)) D = __builtin_copysignf(1e-20f, D);
    Axis a;
    a.inv = 1.0f / D;
    a.nlo = -(r.P + r.h) * a.inv;
    a.nhi = ((r.h + 0x1p-12f) - r.P) * a.inv;
    return a;
}

// slab test of one child box (slab_child, trace.hip, without the reference's PZERO rules): near / far of the inflated box
PSM_D void slab(const Axis& X, const Axis& Y, const Axis& Z, float mnx, float mny, float mnz, float mxx, float mxy, float mxz,
                float& tNear, float& tFar) {
    const float ax = fmaf(mnx, X.inv, X.nlo), bx = fmaf(mxx, X.inv, X.nhi);
    const float ay = fmaf(mny, Y.inv, Y.nlo), by = fmaf(mxy, Y.inv, Y.nhi);
    const float az = fmaf(mnz, Z.inv, Z.nlo), bz = fmaf(mxz, Z.inv, Z.nhi);
    tNear = smaxf(smaxf(sminf(ax, bx), sminf(ay, by)), sminf(az, bz));
    tFar = sminf(sminf(smaxf(ax, bx), smaxf(ay, by)), smaxf(az, bz));
}

// Straight-line pieces the three families' bodies share: only those that leave every kernel's instructions as they were
// (tools/kernel_diff.py). The transform load, the rays' load and two-slab children and the inside vote move kernels when shared
// and stay written out at each site.

// point i of a batch; a dead lane gets a point with a negative rmax (InstInsideBody keeps its own copy: DESIGN.md 4.10)
PSM_D float4 load_point(const float4* points, size_t i, bool alive) {
    float4 q = make_float4(0.f, 0.f, 0.f, -1.f);
    if (alive) q = points[i];
    return q;
}

// the psm_hit of a query that found nothing
PSM_D float4 miss_hit() { return make_float4(0.f, 0.f, __builtin_inff(), __int_as_float(-1)); }

// The walk every query kernel runs: one query per lane, grid-stride over the batch; per query the lone leaf of a one-leaf
// hierarchy, then the tree from the root. A node's two child boxes are judged by the body (kept or not, and an order key: nearer
// first), the accepted leaves are tested one after the other (one copy of the leaf code in the loop), and a kept internal child
// that is not visited next goes on the stack: QSTACK_LDS entries per lane in LDS ([depth][lane]), the rest in the context's spill
// area (spill_for). The body:
//   bool begin(i, alive)  load query i (alive: i < n) and set up; false: the query misses without a walk
//   void children(n0, n1, okL, okR, kL, kR), void leaf(tri), bool done() (the lane retires), void finish(i)
//   bool again()          after a walk: true sets up another walk of the same query (the inside queries' next ray)
// The stack holds links only: a popped subtree is visited and its children judged against the best as it is then
// (keeping each entry's bound to drop it at the pop measured 8 % slower on the point queries).
template <class Body>
PSM_D void query_walk(const QueryArgs& a, Body& q) {
    __shared__ int stack[QSTACK_LDS][QUERY_BLOCK];
    const int lane = (int)threadIdx.x;
    __builtin_assume(lane >= 0 && lane < QUERY_BLOCK);
    const size_t spill_stride = (size_t)gridDim.x * QUERY_BLOCK;
    int* __restrict__ spill = a.spill + (size_t)blockIdx.x * QUERY_BLOCK + lane;
    const uint4* __restrict__ node32 = a.node32;
    const int root = (int)a.sm[SM_ROOT];
    const uint32_t count = a.sm[SM_COUNT];
    const int lone = (count == 1u) ? a.sorted_tri[0] : -1;   // one leaf: no tree, the leaf's triangle is the only candidate
    for (size_t i = (size_t)blockIdx.x * QUERY_BLOCK + (size_t)lane; i - (size_t)lane < a.n; i += spill_stride) {
        const bool alive = i < a.n;
        const bool valid = q.begin(i, alive);
        do {
            if (valid && lone >= 0) q.leaf(lone);
            int cur = root, sp = 0;
            bool walking = valid && root >= 0;
            while (walking) {
                const uint4* np = (const uint4*)((const char*)node32 + ((uint32_t)cur << 5));
                const uint4 n0 = np[0], n1 = np[1];
                const int lkx = (int)n1.z, lky = (int)n1.w;
                bool okL, okR;
                float kL, kR;
                q.children(n0, n1, okL, okR, kL, kR);
                const bool leafL = okL && lkx < 0, leafR = okR && lky < 0;
                // the accepted leaves, one test after the other (one copy of the triangle code in the loop)
                int t0 = leafL ? ~lkx : (leafR ? ~lky : -1);
                int t1 = (leafL && leafR) ? ~lky : -1;
                while (t0 >= 0) {
                    q.leaf(t0);
                    t0 = t1;
                    t1 = -1;
                }
                if (q.done()) break;
                const bool intL = okL && !leafL, intR = okR && !leafR;
                const bool leftFirst = intL && (!intR || kL <= kR);   // nearer child first
                const int first = leftFirst ? lkx : lky, second = leftFirst ? lky : lkx;
                if (intL && intR) {
                    // (sp < QSTACK_MAX always: see QSTACK_MAX; the host refuses hierarchies whose bound exceeds it)
                    if (sp < QSTACK_LDS) stack[sp][lane] = second;
                    else if (sp < QSTACK_MAX) spill[(size_t)(sp - QSTACK_LDS) * spill_stride] = second;
                    sp++;
                }
                cur = first;
                if (!(intL || intR)) {
                    if (sp == 0) break;
                    sp--;
                    cur = sp < QSTACK_LDS ? stack[sp][lane] : spill[(size_t)(sp - QSTACK_LDS) * spill_stride];
                }
            }
        } while (q.again());
        if (alive) q.finish(i);
    }
}

// ---- point queries: closest point and within radius (psm_point_query; include/psm_hip.h) ---------------------

// clamp01 and closest_on_tri also compile for the host: a stand-alone program defines PSM_POINT_FN as a host function's
// decoration before it includes this file (tests/cpp/tri_dist_host.cpp, through psm_tri_dist_dev.h)
#ifndef PSM_POINT_FN
#define PSM_POINT_FN PSM_D
#endif

PSM_POINT_FN float clamp01(float x) {   // (x > 0 ? x : 0) then (x < 1 ? x : 1): NaN and -0 give +0 (tests/point_query_model.py _clamp01)
    x = x > 0.f ? x : 0.f;
    return x < 1.f ? x : 1.f;
}

// The closest point of triangle (v0, e1 = v1 - v0, e2 = v2 - v0) to p: Ericson's region test (Real-Time Collision Detection 5.1.5)
// with the dot products of the edges hoisted (d3 = d1 - aa, ... are Ericson's d3..d6 for bp = ap - e1, cp = ap - e2, and vc / vb
// his vc / vb multiplied out). Returns d2 = |p - c|^2 for c = (v0 + u e1) + v e2, the point in every region.
// Guards (a degenerate triangle gives a finite answer for finite input):
//   * an edge region is taken only when its denominator is positive; a zero-length edge never matches and its vertices' and the
//     other edges' regions decide (for a triangle with two equal vertices every region of the zero edge holds with equality)
//   * the face: det = aa bb - ab^2 (= |e1 x e2|^2, Ericson's va + vb + vc) must exceed 2^-16 aa bb (sin^2 of the angle at v0). The
//     rounding of det is ~14 eps aa bb, so a thinner triangle's face barycentrics are noise; it is taken as its longest edge, the
//     clamped projection onto it (a collinear triangle's longest edge spans it; a thin one lies within its width, <= s L with
//     s <= 2^-8 the sine at v0, of it). A face just above the threshold keeps ~8 eps / s^2 L of barycentric noise: near
//     s = 2^-8 a distance can be off by ~2^-7 L either way.
//     The face's u, v are clamped into the triangle (u in [0, 1], v in [0, 1 - u]): c never leaves the triangle by more than
//     rounding, which the pruning bound relies on.
PSM_POINT_FN float closest_on_tri(v3 v0, v3 e1, v3 e2, v3 p, float& U, float& V) {
    const v3 ap = p - v0;
    const float aa = dot3(e1, e1), ab = dot3(e1, e2), bb = dot3(e2, e2);
    const float d1 = dot3(e1, ap), d2 = dot3(e2, ap);
    const float d3 = d1 - aa, d4 = d2 - ab, d5 = d1 - ab, d6 = d2 - bb;
    const float vc = aa * d2 - ab * d1;
    const float vb = bb * d1 - ab * d2;
    const float va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    const float det = aa * bb - ab * ab;
    const v3 e21 = e2 - e1;
    const float cc = dot3(e21, e21);
    // The region, first match wins: taken from the last to the first, each match overriding, so one small integer and the
    // operands of the one division it needs stay live (branch-free; a wave meets every region anyway). reg: 0 vertex v0, 1 vertex
    // v1, 2 edge v0 v1, 3 vertex v2, 4 edge v0 v2, 5 edge v1 v2, 6 face, 7 / 8 / 9 a sliver's longest edge e1 / e2 / e2 - e1.
    const bool sa = aa >= bb && aa >= cc, sb = bb >= cc;
    int reg = sa ? 7 : (sb ? 8 : 9);
    float n1 = sa ? d1 : (sb ? d2 : e43), q1d = sa ? aa : (sb ? bb : cc);
    if (det > (aa * bb) * 0x1p-16f) { reg = 6; n1 = vb; q1d = det; }
    if (va <= 0.f && e43 >= 0.f && e56 >= 0.f && e43 + e56 > 0.f) { reg = 5; n1 = e43; q1d = e43 + e56; }
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f && d2 - d6 > 0.f) { reg = 4; n1 = d2; q1d = d2 - d6; }
    if (d6 >= 0.f && d5 <= d6) { reg = 3; n1 = 0.f; q1d = 1.f; }
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f && d1 - d3 > 0.f) { reg = 2; n1 = d1; q1d = d1 - d3; }
    if (d3 >= 0.f && d4 <= d3) { reg = 1; n1 = 0.f; q1d = 1.f; }
    if (d1 <= 0.f && d2 <= 0.f) { reg = 0; n1 = 0.f; q1d = 1.f; }
    const float q1 = n1 / q1d;
    const float q2 = (reg == 6 ? vc : 0.f) / (reg == 6 ? det : 1.f);
    const float c1 = clamp01(q1);
    float u = 0.f, v = 0.f;
    if (reg == 1) u = 1.f;
    if (reg == 2) u = q1;
    if (reg == 3) v = 1.f;
    if (reg == 4) v = q1;
    if (reg == 5) { u = 1.f - q1; v = q1; }
    if (reg == 6) {
        u = c1;
        const float f = q2 > 0.f ? q2 : 0.f, lim = 1.f - c1;
        v = f < lim ? f : lim;
    }
    if (reg == 7) u = c1;
    if (reg == 8) v = c1;
    if (reg == 9) { u = 1.f - c1; v = c1; }
    const v3 c = mk3((v0.x + u * e1.x) + v * e2.x, (v0.y + u * e1.y) + v * e2.y, (v0.z + u * e1.z) + v * e2.z);
    const v3 dp = p - c;
    U = u;
    V = v;
    return dot3(dp, dp);
}

// The pruning bound of a point (per launch; every workgroup evaluates it once before its loop, from the build's transform).
// A box of the tree holds, for every point x of every triangle under it, the exact normalised image y = M3 x + m: the leaf box is
// the triangle's padded by PZERO before the fp16 rounding, far above the rounding of aabbmaker's float M v. For the query point
// p let P = M3 p + m (computed: within ~3 eps S of exact per axis, S as affine_row) and g_k >= 0 the gap on axis k from P to the
// box grown by h = 2^-16 (2 + S): h >> the rounding of P and of the two subtractions, so g_k <= G_k, the exact gap of the exact
// image of p to the ungrown box, and |(M3 (x - p)).k| >= G_k >= g_k for every x in it. World distance from normalised gaps:
//   * rows r_k of M3 with norms lambda_k = |r_k| and cosines c_ij = r_i . r_j / (lambda_i lambda_j); with M3 = D R, D = diag
//     (lambda), |x - p| = |R^-1 D^-1 M3 (x - p)| >= |D^-1 M3 (x - p)| / sigma_max(R), and sigma_max(R)^2 = the largest eigenvalue
//     of R R^T (unit diagonal, off-diagonal c_ij) <= 1 + 2 c_max (Gershgorin). So LB^2 = sum_k (g_k / lambda_k)^2 / (1 + 2 c_max)
//     holds for every invertible M3, and is exact for orthogonal rows (the fit transform: diagonal; a rotate-and-scale
//     optimisation matrix: D R).
//   * |(M3 (x - p)).k| <= lambda_k |x - p| (Cauchy-Schwarz), so LB = max_k g_k / lambda_k holds too, whatever the rows.
// Tolerance: the orthogonal form is used iff c_max <= 2^-11, where its factor 1 / (1 + 2 c_max) costs at most 2^-10 of the bound
// (a float rotation's rows have c ~ 1e-7); a shear leaves c_max far above it and takes the max form, which the sum form scaled
// by 1 / (1 + 2 c_max) would not always beat. c_max is taken 2^-20 above its computed value (the rounding of the cosines).
// Rounding: lambda, 1 / lambda, the squares and the sum are < 20 eps in all, and the distance a triangle is judged by,
// d2 = dot3(p - c, p - c), is >= (1 - 6 eps) |p - c|^2 for its c in the box: every LB^2 is scaled by 1 - 2^-18 (64 eps). A box is
// dropped only when LB^2 > the bound: every point of it is farther than the best so far (or than rmax, below), so a triangle
// with a smaller d2, or an equal d2 and a lower id, is never dropped.
// rmax: a candidate counts iff sqrtf(d2) <= rmax; sqrtf is correctly rounded, so such a d2 is <= rmax^2 (1 + 2^-22), and the
// bound starts at fl(rmax^2) (1 + 2^-20) + 2^-126 (above it for every rmax; +inf for rmax = +inf). Non-finite or overflowing
// arithmetic only makes h infinite or a gap NaN, which fmaxf takes as 0: the box is kept.
// The clearance queries (tri_dist.hip) use the same bound with the query triangle's bounding box in place of
// the point. [gl_k, gh_k] is box_row's interval of the box's image on axis k, grown by its h = 2^-16 (2 + S); the gap of a child
// box is g_k = max(mn_k - gh_k, gl_k - mx_k, 0). A pair's d2 is tri_dist_d2's dot3(Q - P, Q - P) with P = u e1 + v e2 and
// Q = (A + s g1) + t g2 for weights in [0, 1] (u + v and s + t at most 1 up to one rounding). Let x = v0 + P and y = v0 + Q for
// the COMPUTED P and Q. P differs from the point of the stored triangle with those weights by the two products' and the sum's
// roundings, < 3 u (|e1| + |e2|) per component: far inside the leaf box's PZERO padding, so M3 x + m lies in the box. Q differs
// from the point of the real query triangle with those weights by the roundings of A = a - v0, of g1, g2 and of its three sums,
// < 8 u (max(|a_j|, |b_j|, |c_j|) + |v0_j|) on component j (u = 2^-24, one rounding); on normalised axis k that moves the image
// by < 8 u (S + T), S as box_row has it and T = sum_j |m_kj v0_j|. For a diagonal M3 (the plain fit) T <= 1 + |m_k3| <= 1 + S,
// because v0's image lies in the unit cube: the move is < 16 u (2 + S), a sixteenth of h = 256 u (2 + S); the 16x is left for a
// full M3, where T exceeds the image by up to the matrix's condition number (16: the rays' allowance, above). So the image of y
// lies in [gl_k, gh_k], |(M3 (x - y)).k| >= g_k, both forms of the bound hold for |x - y|, and the computed
// d2 >= (1 - 6 u) |Q - P|^2 = (1 - 6 u) |x - y|^2 (one subtraction, three squares and two sums: each (1 + u)), inside the
// 1 - 2^-18 scale. A pair that tri_tri holds has d2 = 0: its unit axes did not separate, so the query's box meets the stored
// triangle's on every axis, every g_k is 0 and LB^2 = 0 (tri.hip's argument). tests/test_tri_dist_query_cpu.py
// holds LB^2 <= d2 for every pair under plain, rotating, rotate-and-scale and shearing matrices.
struct PointBound {
    float il0, il1, il2;   // (1 / lambda_k), 0 for a zero row
    float wf;              // (1 - 2^-18), divided by (1 + 2 c_max) for the orthogonal form
    bool orth;
};
PSM_D PointBound point_bound(const float* M) {
    PointBound b;
    float il[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float lam = sqrtf(dot3(mk3(M[4 * k], M[4 * k + 1], M[4 * k + 2]), mk3(M[4 * k], M[4 * k + 1], M[4 * k + 2])));
        il[k] = lam > 0.f ? 1.0f / lam : 0.f;
    }
    const v3 r0 = mk3(M[0], M[1], M[2]), r1 = mk3(M[4], M[5], M[6]), r2 = mk3(M[8], M[9], M[10]);
    const float c01 = pabs(dot3(r0, r1)) * il[0] * il[1], c02 = pabs(dot3(r0, r2)) * il[0] * il[2];
    const float c12 = pabs(dot3(r1, r2)) * il[1] * il[2];
    const float cmax = smaxf(smaxf(c01, c02), c12) + 0x1p-20f;
    b.il0 = il[0];
    b.il1 = il[1];
    b.il2 = il[2];
    b.orth = cmax <= 0x1p-11f && il[0] > 0.f && il[1] > 0.f && il[2] > 0.f;
    b.wf = b.orth ? (1.0f - 0x1p-18f) / (1.0f + 2.0f * cmax) : (1.0f - 0x1p-18f);
    return b;
}

// a point in a hierarchy's normalised space: its image under the fit transform and the margin, the largest of the three axes' h
struct PointImage {
    float Px, Py, Pz, h;

    PSM_D void set(const float* M, v3 p) {
        const Row X = affine_row(M, 0, p), Y = affine_row(M, 1, p), Z = affine_row(M, 2, p);
        Px = X.P;
        Py = Y.P;
        Pz = Z.P;
        h = smaxf(smaxf(X.h, Y.h), Z.h);
    }
    // LB^2 of one child box (mn / mx: its fp16 corners)
    PSM_D float lb2(const PointBound& B, float mnx, float mny, float mnz, float mxx, float mxy, float mxz) const {
        const float tx = smaxf(smaxf(mnx - Px, Px - mxx) - h, 0.f) * B.il0;
        const float ty = smaxf(smaxf(mny - Py, Py - mxy) - h, 0.f) * B.il1;
        const float tz = smaxf(smaxf(mnz - Pz, Pz - mxz) - h, 0.f) * B.il2;
        const float m = smaxf(smaxf(tx, ty), tz);
        return (B.orth ? ((tx * tx + ty * ty) + tz * tz) : m * m) * B.wf;
    }
    // a node's two child boxes: kept iff LB^2 <= best (<=: a triangle as near as the best and of a lower id still counts); the
    // order key is LB^2
    PSM_D void children(const PointBound& B, uint4 n0, uint4 n1, float best, bool& okL, bool& okR, float& kL, float& kR) const {
        kL = lb2(B, half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z));
        kR = lb2(B, half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y));
        okL = kL <= best;
        okR = kR <= best;
    }
};

// ---- what the inside queries and the posed queries (instances, worlds) share ------------------------------------------------

// The rays of the inside test (psm_hip.h PSM_INSIDE_DIRECTIONS: written there once): ray k of a point p is {p, 0, row k, +inf}.
__device__ const float INSIDE_DIR[PSM_INSIDE_MAX_SAMPLES][3] = PSM_INSIDE_DIRECTIONS;

// The canonical move into an instance's object space (psm_hip.h; tests/instance_query_model.py states it in numpy): a direction
// goes through R^T, x'_j = (R[0][j] d.x + R[1][j] d.y) + R[2][j] d.z, a point through the same after d = x - T per component.
// One float32 operation order (the build contracts nothing: -ffp-contract=off).
PSM_D v3 inst_rotate(const float* m, v3 d) {
    return mk3((m[0] * d.x + m[4] * d.y) + m[8] * d.z, (m[1] * d.x + m[5] * d.y) + m[9] * d.z, (m[2] * d.x + m[6] * d.y) + m[10] * d.z);
}
PSM_D v3 inst_point(const float* m, v3 x) { return inst_rotate(m, mk3(x.x - m[3], x.y - m[7], x.z - m[11])); }

}  // namespace

}  // namespace psm
