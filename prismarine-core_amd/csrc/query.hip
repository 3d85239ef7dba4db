// query.hip -- batched queries against a built hierarchy (new; no reference counterpart): closest hit and any hit of rays,
// closest point and within-radius of points (the point queries are described at point_body below), and the hit
// count of rays with the inside / outside and signed-distance queries of points built on it (CountRay below).
//
// psm_rt_traverse follows directTraverse.comp bit for bit: a 16-entry stack that drops subtrees (STACK_CAP), a PZERO-tolerant
// "closest", intersectTriangle's clamp of |det| at 1e-6. These kernels answer "what does this ray hit?" exactly instead
// (include/psm_hip.h, psm_query_ray):
//   * the candidates are the hierarchy's leaves (PSM_BVH_LEAF_TRI), tested by tri_test's arithmetic without the clamp;
//   * a hit counts iff tmin <= t <= tmax; closest = the smallest t, on bit-equal t the lowest triangle id -- a result that does
//     not depend on the traversal order;
//   * the stack never drops an entry: 16 levels in LDS, the rest in a per-lane global area sized to the builder's height bound.
// Structure as rt_traverse (trace.hip): one ray per lane, one wave64 per workgroup, the stack in LDS laid out [depth][lane],
// child boxes by fmaf on the fp16 record coordinates (v_fma_mix_f32), nearer child first. The kernels are grid-stride. The walk
// (query_walk: grid-stride loop, stack, leaf scheduling) is shared by the ray and the point kernels; a body says what a query is.
// The same seven queries over a list of hierarchies (scene_walk) and over posed instances (4.9) follow. The host
// side is one path for all 21 entry points: check_list / check_data / batch_args / launch over a per-family kernel table (4.10).
#include <cmath>
#include <cstdio>
#include <mutex>
#include <type_traits>
#include <unordered_map>

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
//   lo plane: fmaf(b, inv, nlo) = (b - (P + h)) / D,  hi plane: fmaf(b, inv, nhi) = (b - (P - h)) / D
// i.e. the box grown by h on both sides (for either sign of D). h covers the rounding of P, D and the slab arithmetic: each is a
// few ulps of |b| + S (S = |m0 ox| + |m1 oy| + |m2 oz| + |m3| bounds |P| and the rounding of its sum), and the error of D moves the
// plane distance by t |dD| <= 3 eps t sum_j |M_kj d_j|, which for the fit transform (M's 3 x 3 part is diagonal unless the build's
// optimisation matrix rotates) is 3 eps |b - P| <= 3 eps (1 + S). All of it is < 8 eps (2 + S); h = 2^-16 (2 + S) ~ 128 eps (2 + S)
// -- with a 16x margin left for an optimisation matrix whose 3 x 3 part has a condition number up to ~16. A box is then dropped
// only when its exact slab interval misses [tmin, limit]. The hit itself lies in its leaf's exact box: an accepted hit point is
// within ~1e-5 edge lengths of its triangle (the u, v tolerances), and the leaf box is the triangle's padded by PZERO = 5e-4
// before the fp16 rounding (<= 2.44e-4 in [0, 1]), >= 2.5e-4 normalised units of headroom.
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
    a.nhi = (r.h - r.P) * a.inv;
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

// the ray queries: closest hit (ANY = false) and any hit (ANY = true); psm_query_ray, DESIGN.md 4.5
template <bool ANY>
struct RayBody {
    const QueryArgs& a;
    v3 o, d;
    float tmin, tmax, best, bu, bv;
    int btri;
    bool found;
    Axis X, Y, Z;

    PSM_D bool begin(size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 1.f), r1 = make_float4(1.f, 0.f, 0.f, -1.f);
        if (alive) { r0 = a.rays[2 * i]; r1 = a.rays[2 * i + 1]; }
        o = mk3(r0.x, r0.y, r0.z);
        d = normalize3(mk3(r1.x, r1.y, r1.z));   // t is the distance along the unit direction (as the oracle's brute force)
        tmin = r0.w;
        tmax = r1.w;
        // NaN anywhere, a zero direction (normalize3 gives NaN) or an empty window: a miss
        const bool valid = alive && finite3(o) && finite3(d) && tmin <= tmax;
        best = tmax;
        bu = 0.f;
        bv = 0.f;
        btri = -1;
        found = false;
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
        // closest: pruned against the best hit so far (a hit at exactly `best` with a lower id still counts: <=)
        const float lim = ANY ? tmax : best;
        okL = (nL <= fL) & (nL <= lim) & (fL >= tmin);
        okR = (nR <= fR) & (nR <= lim) & (fR >= tmin);
    }
    // a candidate triangle: inside the window, and (closest) before the best so far or as far and of a lower id
    // ((uint32_t) btri: -1 is the largest, so the first hit inside the window always counts)
    PSM_D void leaf(int tri) {
        float t, u, v;
        if (tri_query(a.tri48, tri, o, d, t, u, v) && t >= tmin && (t < best || (t == best && (uint32_t)tri < (uint32_t)btri))) {
            found = true;
            if (!ANY) { best = t; bu = u; bv = v; btri = tri; }
        }
    }
    PSM_D bool done() const { return ANY && found; }   // any hit: the lane retires at its first hit
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (ANY) a.occluded[i] = found ? 1 : 0;
        else a.hits[i] = found ? make_float4(bu, bv, best, __int_as_float(btri)) : miss_hit();
    }
};

// ---- point queries: closest point and within radius (psm_point_query; include/psm_hip.h) ---------------------

PSM_D float clamp01(float x) {   // (x > 0 ? x : 0) then (x < 1 ? x : 1): NaN and -0 give +0 (tests/point_query_model.py _clamp01)
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
PSM_D float closest_on_tri(v3 v0, v3 e1, v3 e2, v3 p, float& U, float& V) {
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

// the point queries: closest point (WITHIN = false) and within radius (WITHIN = true)
template <bool WITHIN>
struct PointBody {
    const QueryArgs& a;
    const PointBound B;
    v3 p;
    float rmax, best, bu, bv;   // best: the pruning bound -- the best d2 so far, the rmax bound until one is found
    int btri;
    bool found;
    PointImage P;

    PSM_D bool begin(size_t i, bool alive) {
        const float4 q = load_point(a.rays, i, alive);
        p = mk3(q.x, q.y, q.z);
        rmax = q.w;
        const bool valid = alive && finite3(p) && rmax >= 0.f;   // NaN or negative rmax: a miss; +inf: no limit
        best = (rmax * rmax) * 1.00000095367431640625f + 0x1p-126f;   // fl(rmax^2) (1 + 2^-20) + 2^-126
        bu = 0.f;
        bv = 0.f;
        btri = -1;
        found = false;
        float M[16];
        #pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
        P.set(M, p);
        return valid;
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& kL, float& kR) const {
        P.children(B, n0, n1, best, okL, okR, kL, kR);
    }
    // a candidate: within rmax, and (closest) nearer than the best so far or as near and of a lower id
    // ((uint32_t) btri: -1 is the largest; before the first, best is the rmax bound, >= every d2 that counts)
    PSM_D void leaf(int tri) {
        const float4 A = a.tri48[(size_t)3 * tri + 0], Bv = a.tri48[(size_t)3 * tri + 1], C = a.tri48[(size_t)3 * tri + 2];
        float u, v;
        const float d2 = closest_on_tri(mk3(A.x, A.y, A.z), mk3(Bv.x, Bv.y, Bv.z), mk3(C.x, C.y, C.z), p, u, v);
        if (sqrtf(d2) <= rmax && (d2 < best || (d2 == best && (uint32_t)tri < (uint32_t)btri))) {
            found = true;
            if (!WITHIN) { best = d2; bu = u; bv = v; btri = tri; }
        }
    }
    PSM_D bool done() const { return WITHIN && found; }   // within: the lane retires at its first counting candidate
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (WITHIN) a.occluded[i] = found ? 1 : 0;
        else a.hits[i] = found ? make_float4(bu, bv, sqrtf(best), __int_as_float(btri)) : miss_hit();
    }
};

template <bool ANY>
PSM_D void query_body(const QueryArgs& a) {
    RayBody<ANY> q{a};
    query_walk(a, q);
}

template <bool WITHIN>
PSM_D void point_body(const QueryArgs& a) {
    float M[16];
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
    PointBody<WITHIN> q{a, point_bound(M)};
    query_walk(a, q);
}

// ---- hit count, inside / outside, signed distance (include/psm_hip.h) ------------------------------------------

// The ray every one of these walks: all candidates with tri_query's acceptance and tmin <= t <= tmax are counted -- the any-hit
// predicate, asked "how many?". Against the any-hit body: a child box is kept against [tmin, tmax] only (there is no best t to
// prune by) and the lane never retires early. The count is a sum of integers: it does not depend on the traversal order, so the
// children's order key (the near distance, as the other ray bodies) is only a matter of memory locality.
struct CountRay {
    const QueryArgs& a;
    v3 o, d;
    float tmin, tmax;
    uint32_t count;
    Axis X, Y, Z;

    // aim the ray (dir: as given, normalised here as every query ray's) and clear the count; false: the ray is invalid (RayBody)
    PSM_D bool aim(v3 orig, v3 dir, float lo, float hi) {
        o = orig;
        d = normalize3(dir);
        tmin = lo;
        tmax = hi;
        count = 0u;
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
        X = ray_axis(M, 0, o, d);
        Y = ray_axis(M, 1, o, d);
        Z = ray_axis(M, 2, o, d);
        return finite3(o) && finite3(d) && tmin <= tmax;
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& nL, float& nR) const {
        float fL, fR;
        slab(X, Y, Z, half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z), nL, fL);
        slab(X, Y, Z, half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y), nR, fR);
        okL = (nL <= fL) & (nL <= tmax) & (fL >= tmin);
        okR = (nR <= fR) & (nR <= tmax) & (fR >= tmin);
    }
    PSM_D void leaf(int tri) {
        float t, u, v;
        if (tri_query(a.tri48, tri, o, d, t, u, v) && t >= tmin && t <= tmax) count++;
    }
    PSM_D bool done() const { return false; }   // every crossing counts: the walk ends when the stack is empty
};

// hit count of a ray (psm_bvh_count_hits_dev)
struct CountBody : CountRay {
    PSM_D bool begin(size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 1.f), r1 = make_float4(1.f, 0.f, 0.f, -1.f);
        if (alive) { r0 = a.rays[2 * i]; r1 = a.rays[2 * i + 1]; }
        return aim(mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), r0.w, r1.w) && alive;
    }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const { a.count[i] = count; }
};

// The rays of the inside test (psm_hip.h PSM_INSIDE_DIRECTIONS: written there once): ray k of a point p is {p, 0, row k, +inf}.
__device__ const float INSIDE_DIR[PSM_INSIDE_MAX_SAMPLES][3] = PSM_INSIDE_DIRECTIONS;

// inside / outside of a point (SIGN = false: psm_bvh_inside_dev) and the sign of a closest-point result (SIGN = true: the second
// kernel of psm_bvh_signed_distance_dev, after bvh_query_point has written hits[i]). One point per lane; its `samples` rays are
// walked one after the other (again()), so at any moment every lane of the wave follows the same direction from nearby origins.
// A ray votes "inside" iff its count is odd; the point is inside iff more than half of the rays vote so.
// SIGN: a point whose closest-point result is a miss (no triangle within rmax, an invalid query) walks nothing and keeps its
// record; the others get the sign bit of t set when inside (a distance of 0 becomes -0).
template <bool SIGN>
struct InsideBody : CountRay {
    v3 p;
    uint32_t k, votes;
    float dist;
    bool valid;

    PSM_D bool shoot() {
        const int r = __builtin_amdgcn_readfirstlane((int)k);   // (the same k in every lane that walks: the row by scalar loads)
        return aim(p, mk3(INSIDE_DIR[r][0], INSIDE_DIR[r][1], INSIDE_DIR[r][2]), 0.f, __builtin_inff());
    }
    PSM_D bool begin(size_t i, bool alive) {
        const float4 q = load_point(a.rays, i, alive);
        p = mk3(q.x, q.y, q.z);
        k = 0u;
        votes = 0u;
        dist = 0.f;
        valid = alive;
        if (SIGN) {
            float4 h = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
            if (alive) h = a.hits[i];
            dist = h.z;
            valid = __float_as_int(h.w) >= 0;
        }
        valid = shoot() && valid;   // (a non-finite p: outside)
        return valid;
    }
    PSM_D bool again() {
        votes += count & 1u;
        k++;
        if (!valid || k >= a.samples) return false;
        shoot();
        return true;
    }
    PSM_D void finish(size_t i) const {
        const bool in = 2u * votes > a.samples;
        if (!SIGN) a.occluded[i] = in ? 1 : 0;
        else if (in) ((float*)(a.hits + i))[2] = __uint_as_float(__float_as_uint(dist) | 0x80000000u);
    }
};

PSM_D void count_body(const QueryArgs& a) {
    CountBody q{{a}};
    query_walk(a, q);
}

template <bool SIGN>
PSM_D void inside_body(const QueryArgs& a) {
    InsideBody<SIGN> q{{a}};
    query_walk(a, q);
}

}  // namespace

// the kernels, under names of their own (profiles and the codegen tests find them by these)
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_closest(QueryArgs a) { query_body<false>(a); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_any(QueryArgs a) { query_body<true>(a); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_point(QueryArgs a) { point_body<false>(a); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_within(QueryArgs a) { point_body<true>(a); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_count(QueryArgs a) { count_body(a); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_inside(QueryArgs a) { inside_body<false>(a); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_sign(QueryArgs a) { inside_body<true>(a); }

// ---- scene queries: the seven queries over several hierarchies at once (include/psm_hip.h "scene queries") ------

// One geometry of a scene as a kernel reads it: QueryArgs' four hierarchy pointers. The table of a launch travels in the
// kernel-argument segment (PSM_SCENE_MAX_GEOMETRIES x 32 B = 1 KB): no device allocation, nothing that could go stale.
struct SceneGeom {
    const uint4* node32;
    const float4* tri48;
    const uint32_t* sm;
    const int32_t* sorted_tri;
};
struct SceneArgs {
    const float4* rays;      // as QueryArgs
    size_t n;
    int* spill;
    float4* hits;
    uint8_t* occluded;
    uint32_t* count;
    int32_t* geom;           // closest hit / closest point / signed distance: the winning geometry per query, -1 on a miss
    uint32_t samples;
    uint32_t geoms;          // G: 1 .. PSM_SCENE_MAX_GEOMETRIES
    SceneGeom g[PSM_SCENE_MAX_GEOMETRIES];
};

namespace {

// query_walk over a scene, as a walk of its own (the seven single-hierarchy kernels keep theirs, and with it their code): per
// query the geometries one after the other, geometry 0 first, each walked as query_walk walks its hierarchy. The geometry index
// is the same in every lane of the wave, so the four pointers, the root and the leaf count of a geometry are scalar loads from
// the kernel-argument table. The body carries its running state (best, count, parity, found) from one geometry to the next:
//   bool begin(i, alive)     load query i and clear the running state; false: the query misses without a walk
//   void enter(gm, g)        the per-geometry set-up (the ray's axes / the point's bound from that geometry's fit transform)
//   children, leaf, done, again, finish: as query_walk's; a lane that is done() skips the remaining geometries
//   again(): every geometry is walked again (the inside queries' next ray: its parity is summed over the whole scene)
// Args: SceneArgs, or the instanced queries' InstArgs (below): the same walk over a table whose entries also carry a pose. A
// body whose enter() returns bool says whether the query is valid in that entry (the instanced queries: validity is judged
// per instance, on the moved query); one that returns void is valid everywhere (the scene bodies, whose code this leaves as it was).
template <class Args, class Body>
PSM_D void scene_walk(const Args& s, Body& q) {
    __shared__ int stack[QSTACK_LDS][QUERY_BLOCK];
    const int lane = (int)threadIdx.x;
    __builtin_assume(lane >= 0 && lane < QUERY_BLOCK);
    const size_t spill_stride = (size_t)gridDim.x * QUERY_BLOCK;
    int* __restrict__ spill = s.spill + (size_t)blockIdx.x * QUERY_BLOCK + lane;
    for (size_t i = (size_t)blockIdx.x * QUERY_BLOCK + (size_t)lane; i - (size_t)lane < s.n; i += spill_stride) {
        const bool alive = i < s.n;
        const bool valid = q.begin(i, alive);
        do {
            for (uint32_t g = 0; g < s.geoms; g++) {
                const auto gm = s.g[g];
                const uint4* __restrict__ node32 = gm.node32;
                const int root = (int)gm.sm[SM_ROOT];
                const uint32_t count = gm.sm[SM_COUNT];
                const int lone = (count == 1u) ? gm.sorted_tri[0] : -1;
                bool here = true;
                if constexpr (std::is_void_v<decltype(q.enter(gm, (int)g))>) q.enter(gm, (int)g);
                else here = q.enter(gm, (int)g);
                const bool go = valid && here && !q.done();
                if (go && lone >= 0) q.leaf(lone);
                int cur = root, sp = 0;
                bool walking = go && root >= 0;
                while (walking) {
                    const uint4* np = (const uint4*)((const char*)node32 + ((uint32_t)cur << 5));
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
                    if (q.done()) break;
                    const bool intL = okL && !leafL, intR = okR && !leafR;
                    const bool leftFirst = intL && (!intR || kL <= kR);
                    const int first = leftFirst ? lkx : lky, second = leftFirst ? lky : lkx;
                    if (intL && intR) {
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
            }
        } while (q.again());
        if (alive) q.finish(i);
    }
}

// The tie rule across geometries (closest hit and closest point; `best` is t or d2). The winner is the smallest value, on a
// bit-equal value the lexicographically lowest (geom, tri). The geometries are walked in ascending order, so at a candidate
// (g, tri) with value x every earlier record is of a geometry <= g:
//   x <  best                                   wins, whatever the ids
//   x == best, the record is of geometry g      wins iff tri < btri: `<` on the id, as inside one hierarchy
//   x == best, the record is of a geometry < g  loses: (geom, tri) of the record is lower whatever tri is
//   x == best, no record yet                    wins (best is the window's / the radius' own bound): any id is below "none"
// One unsigned key `tie` holds all of it as "tri < tie": 0xffffffff while there is no record, 0 from enter() on when the record
// is of an earlier geometry (no id is below 0), the record's tri once it is of this geometry. The same hierarchy twice
// therefore answers with the lower index. Boxes are kept with `<=` against best in every case: inside geometry g a candidate at
// exactly best with a lower id must still be reached, and best may have become this geometry's at any leaf. For a best that is
// still an earlier geometry's, `<` would be enough (an equal value loses); keeping `<=` there visits, and rejects at the leaf,
// only candidates at exactly the earlier best -- never a wrong answer, and no second compare in the node loop.
struct SceneBest {
    float best, bu, bv;
    int btri, bgeom, cur;
    uint32_t tie;
    PSM_D void clear(float bound) {
        best = bound;
        bu = 0.f;
        bv = 0.f;
        btri = -1;
        bgeom = -1;
        tie = 0xffffffffu;
    }
    PSM_D void enter_geom(int g) {
        cur = g;
        if (bgeom >= 0) tie = 0u;
    }
    PSM_D bool wins(float x, int tri) const { return x < best || (x == best && (uint32_t)tri < tie); }
    PSM_D void take(float x, float u, float v, int tri) {
        best = x;
        bu = u;
        bv = v;
        btri = tri;
        bgeom = cur;
        tie = (uint32_t)tri;
    }
};

// a ray in a scene: RayBody's / CountRay's ray, with the axes redone per geometry (each has a fit transform of its own)
struct SceneRay {
    SceneGeom gm;
    v3 o, d;
    float tmin, tmax;
    Axis X, Y, Z;

    PSM_D bool aim(v3 orig, v3 dir, float lo, float hi) {
        o = orig;
        d = normalize3(dir);
        tmin = lo;
        tmax = hi;
        return finite3(o) && finite3(d) && tmin <= tmax;
    }
    template <class Args>
    PSM_D bool load(const Args& s, size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 1.f), r1 = make_float4(1.f, 0.f, 0.f, -1.f);
        if (alive) { r0 = s.rays[2 * i]; r1 = s.rays[2 * i + 1]; }
        return aim(mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), r0.w, r1.w) && alive;
    }
    PSM_D void axes(const SceneGeom& g) {
        gm = g;
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(g.sm[SM_M + k]);
        X = ray_axis(M, 0, o, d);
        Y = ray_axis(M, 1, o, d);
        Z = ray_axis(M, 2, o, d);
    }
    PSM_D void boxes(uint4 n0, uint4 n1, float lim, bool& okL, bool& okR, float& nL, float& nR) const {
        float fL, fR;
        slab(X, Y, Z, half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z), nL, fL);
        slab(X, Y, Z, half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y), nR, fR);
        okL = (nL <= fL) & (nL <= lim) & (fL >= tmin);
        okR = (nR <= fR) & (nR <= lim) & (fR >= tmin);
    }
};

// closest hit (ANY = false) and any hit (ANY = true) of a scene: RayBody with the best carried across the geometries
// (Args: SceneArgs; the instanced bodies below derive from these over InstArgs and replace begin() and enter())
template <bool ANY, class Args = SceneArgs>
struct SceneRayBody : SceneRay {
    const Args& s;
    SceneBest b;
    bool found;

    PSM_D SceneRayBody(const Args& a) : s(a) {}
    PSM_D bool begin(size_t i, bool alive) {
        const bool valid = load(s, i, alive);
        b.clear(tmax);
        found = false;
        return valid;
    }
    PSM_D void enter(const SceneGeom& g, int gi) {
        axes(g);
        b.enter_geom(gi);
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& nL, float& nR) const {
        boxes(n0, n1, ANY ? tmax : b.best, okL, okR, nL, nR);   // (<=: see SceneBest)
    }
    PSM_D void leaf(int tri) {
        float t, u, v;
        if (tri_query(gm.tri48, tri, o, d, t, u, v) && t >= tmin && b.wins(t, tri)) {
            found = true;
            if (!ANY) b.take(t, u, v, tri);
        }
    }
    PSM_D bool done() const { return ANY && found; }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (ANY) {
            s.occluded[i] = found ? 1 : 0;
        } else {
            s.hits[i] = found ? make_float4(b.bu, b.bv, b.best, __int_as_float(b.btri)) : miss_hit();
            s.geom[i] = b.bgeom;
        }
    }
};

// closest point (WITHIN = false) and within radius (WITHIN = true) of a scene: PointBody with the best d2 carried across the
// geometries; the point's normalised image and the bound's factors are redone per geometry (point_bound: per fit transform)
template <bool WITHIN, class Args = SceneArgs>
struct ScenePointBody {
    const Args& s;
    SceneGeom gm;
    PointBound B;
    v3 p;
    float rmax;
    SceneBest b;
    bool found;
    PointImage P;

    PSM_D ScenePointBody(const Args& a) : s(a) {}
    PSM_D bool begin(size_t i, bool alive) {
        const float4 q = load_point(s.rays, i, alive);
        p = mk3(q.x, q.y, q.z);
        rmax = q.w;
        b.clear((rmax * rmax) * 1.00000095367431640625f + 0x1p-126f);   // (PointBody::begin)
        found = false;
        return alive && finite3(p) && rmax >= 0.f;
    }
    PSM_D void enter(const SceneGeom& g, int gi) {
        gm = g;
        float M[16];
        #pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(g.sm[SM_M + k]);
        B = point_bound(M);
        P.set(M, p);
        b.enter_geom(gi);
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& kL, float& kR) const {
        // (<=: see SceneBest; LB^2 is a world distance, comparable across the geometries' transforms)
        P.children(B, n0, n1, b.best, okL, okR, kL, kR);
    }
    PSM_D void leaf(int tri) {
        const float4 A = gm.tri48[(size_t)3 * tri + 0], Bv = gm.tri48[(size_t)3 * tri + 1], Cv = gm.tri48[(size_t)3 * tri + 2];
        float u, v;
        const float d2 = closest_on_tri(mk3(A.x, A.y, A.z), mk3(Bv.x, Bv.y, Bv.z), mk3(Cv.x, Cv.y, Cv.z), p, u, v);
        if (sqrtf(d2) <= rmax && b.wins(d2, tri)) {
            found = true;
            if (!WITHIN) b.take(d2, u, v, tri);
        }
    }
    PSM_D bool done() const { return WITHIN && found; }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (WITHIN) {
            s.occluded[i] = found ? 1 : 0;
        } else {
            s.hits[i] = found ? make_float4(b.bu, b.bv, sqrtf(b.best), __int_as_float(b.btri)) : miss_hit();
            s.geom[i] = b.bgeom;
        }
    }
};

// the counting ray of a scene (CountRay): the count runs on across the geometries
struct SceneCountRay : SceneRay {
    uint32_t count;
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& nL, float& nR) const { boxes(n0, n1, tmax, okL, okR, nL, nR); }
    PSM_D void leaf(int tri) {
        float t, u, v;
        if (tri_query(gm.tri48, tri, o, d, t, u, v) && t >= tmin && t <= tmax) count++;
    }
    PSM_D bool done() const { return false; }
};

template <class Args = SceneArgs>
struct SceneCountBody : SceneCountRay {
    const Args& s;
    PSM_D SceneCountBody(const Args& a) : s(a) {}
    PSM_D bool begin(size_t i, bool alive) {
        count = 0u;
        return load(s, i, alive);
    }
    PSM_D void enter(const SceneGeom& g, int) { axes(g); }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const { s.count[i] = count; }
};

// inside / outside of a point against a scene (SIGN = false) and the sign of a scene closest-point result (SIGN = true):
// InsideBody, with ray k's crossings summed over all geometries before it votes (again() comes after the last geometry)
template <bool SIGN, class Args = SceneArgs>
struct SceneInsideBody : SceneCountRay {
    const Args& s;
    v3 p;
    uint32_t k, votes;
    float dist;
    bool valid;

    PSM_D SceneInsideBody(const Args& a) : s(a) {}
    PSM_D bool shoot() {
        const int r = __builtin_amdgcn_readfirstlane((int)k);
        count = 0u;
        return aim(p, mk3(INSIDE_DIR[r][0], INSIDE_DIR[r][1], INSIDE_DIR[r][2]), 0.f, __builtin_inff());
    }
    PSM_D bool begin(size_t i, bool alive) {
        const float4 q = load_point(s.rays, i, alive);
        p = mk3(q.x, q.y, q.z);
        k = 0u;
        votes = 0u;
        dist = 0.f;
        valid = alive;
        if (SIGN) {
            float4 h = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
            if (alive) h = s.hits[i];
            dist = h.z;
            valid = __float_as_int(h.w) >= 0;
        }
        valid = shoot() && valid;
        return valid;
    }
    PSM_D void enter(const SceneGeom& g, int) { axes(g); }
    PSM_D bool again() {
        votes += count & 1u;
        k++;
        if (!valid || k >= s.samples) return false;
        shoot();
        return true;
    }
    PSM_D void finish(size_t i) const {
        const bool in = 2u * votes > s.samples;
        if (!SIGN) s.occluded[i] = in ? 1 : 0;
        else if (in) ((float*)(s.hits + i))[2] = __uint_as_float(__float_as_uint(dist) | 0x80000000u);
    }
};

template <class Body, class Args>
PSM_D void scene_body(const Args& s) {
    Body q(s);
    scene_walk(s, q);
}

}  // namespace

__global__ __launch_bounds__(QUERY_BLOCK, 8) void scene_query_closest(SceneArgs s) { scene_body<SceneRayBody<false>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void scene_query_any(SceneArgs s) { scene_body<SceneRayBody<true>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void scene_query_point(SceneArgs s) { scene_body<ScenePointBody<false>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void scene_query_within(SceneArgs s) { scene_body<ScenePointBody<true>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void scene_query_count(SceneArgs s) { scene_body<SceneCountBody<>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void scene_query_inside(SceneArgs s) { scene_body<SceneInsideBody<false>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void scene_query_sign(SceneArgs s) { scene_body<SceneInsideBody<true>>(s); }

// ---- instanced scene queries: a rigid transform per entry (include/psm_hip.h "instanced scene queries") ---------

// One instance as a kernel reads it: a geometry of a scene and its pose, the 12 floats of psm_instance.world_from_object
// (row-major 3 x 4 [R | T]). The table travels in the kernel-argument segment as SceneArgs' does (32 x 80 B = 2560 B): a pose
// changed on the host is the next launch's, and nothing on the device can go stale. The instance index is the same in every
// lane of a wave, so the matrix is read by scalar loads and never leaves the scalar registers.
struct InstGeom : SceneGeom {
    float m[12];
};
struct InstArgs {
    const float4* rays;      // as SceneArgs
    size_t n;
    int* spill;
    float4* hits;
    uint8_t* occluded;
    uint32_t* count;
    int32_t* geom;           // the winning INSTANCE per query, -1 on a miss
    uint32_t samples;
    uint32_t geoms;          // instances: 1 .. PSM_SCENE_MAX_GEOMETRIES
    InstGeom g[PSM_SCENE_MAX_GEOMETRIES];
};
static_assert(sizeof(InstGeom) == 80 && sizeof(InstArgs) <= 4096, "the instance table must fit the kernel-argument segment");

namespace {

// The canonical move into an instance's object space (psm_hip.h; tests/instance_query_model.py states it in numpy): a direction
// goes through R^T, x'_j = (R[0][j] d.x + R[1][j] d.y) + R[2][j] d.z, a point through the same after d = x - T per component.
// One float32 operation order (the build contracts nothing: -ffp-contract=off).
PSM_D v3 inst_rotate(const float* m, v3 d) {
    return mk3((m[0] * d.x + m[4] * d.y) + m[8] * d.z, (m[1] * d.x + m[5] * d.y) + m[9] * d.z, (m[2] * d.x + m[6] * d.y) + m[10] * d.z);
}
PSM_D v3 inst_point(const float* m, v3 x) { return inst_rotate(m, mk3(x.x - m[3], x.y - m[7], x.z - m[11])); }

// The instanced bodies are the scene bodies over InstArgs with begin() and enter() replaced. begin() keeps what passes through
// unchanged (the window, rmax) and the query's index; enter() reads the query again from memory (16 or 32 B, resident in L2),
// moves it into the instance's object space, then does the scene body's per-geometry set-up. The world query is therefore never
// live across the walk, which would cost the registers the scene kernels do not have to spare. enter() returns whether the moved
// query is valid in this instance (NaN and infinity propagate through the move; a finite query can overflow in it).

// enter() of the ray bodies: the ray aimed as SceneRay::aim aims it (the direction rotated as given, then normalised)
PSM_D bool inst_ray(SceneRay& r, const float4* __restrict__ rays, const InstGeom& g, size_t i, bool alive) {
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = make_float4(1.f, 0.f, 0.f, 0.f);
    if (alive) { r0 = rays[2 * i]; r1 = rays[2 * i + 1]; }
    r.o = inst_point(g.m, mk3(r0.x, r0.y, r0.z));
    r.d = normalize3(inst_rotate(g.m, mk3(r1.x, r1.y, r1.z)));
    r.axes(g);
    return finite3(r.o) && finite3(r.d);
}
// begin() of the ray bodies: the window alone
PSM_D bool inst_window(SceneRay& r, const float4* __restrict__ rays, size_t i, bool alive) {
    r.tmin = 0.f;
    r.tmax = -1.f;
    if (alive) { r.tmin = rays[2 * i].w; r.tmax = rays[2 * i + 1].w; }
    return alive && r.tmin <= r.tmax;
}

// closest hit / any hit over instances. t is the distance along the moved unit direction: an object-space value, comparable
// across instances because the move is rigid (to 1e-5 relative: psm_hip.h)
template <bool ANY>
struct InstRayBody : SceneRayBody<ANY, InstArgs> {
    size_t idx;
    bool alive;
    PSM_D InstRayBody(const InstArgs& a) : SceneRayBody<ANY, InstArgs>(a) {}
    PSM_D bool begin(size_t i, bool al) {
        idx = i;
        alive = al;
        const bool valid = inst_window(*this, this->s.rays, i, al);
        this->b.clear(this->tmax);
        this->found = false;
        return valid;
    }
    PSM_D bool enter(const InstGeom& g, int gi) {
        const bool here = inst_ray(*this, this->s.rays, g, idx, alive);   // the move, then the axes; then the tie key
        this->b.enter_geom(gi);
        return here;
    }
};

struct InstCountBody : SceneCountBody<InstArgs> {
    size_t idx;
    bool alive;
    PSM_D InstCountBody(const InstArgs& a) : SceneCountBody<InstArgs>(a) {}
    PSM_D bool begin(size_t i, bool al) {
        idx = i;
        alive = al;
        count = 0u;
        return inst_window(*this, s.rays, i, al);
    }
    PSM_D bool enter(const InstGeom& g, int) { return inst_ray(*this, s.rays, g, idx, alive); }
};

// closest point / within over instances: p is the point in the instance's object space; rmax passes through, d2 is an
// object-space value (see InstRayBody)
template <bool WITHIN>
struct InstPointBody : ScenePointBody<WITHIN, InstArgs> {
    size_t idx;
    bool alive;
    PSM_D InstPointBody(const InstArgs& a) : ScenePointBody<WITHIN, InstArgs>(a) {}
    PSM_D bool begin(size_t i, bool al) {
        idx = i;
        alive = al;
        const float4 q = load_point(this->s.rays, i, al);
        this->rmax = q.w;
        this->b.clear((q.w * q.w) * 1.00000095367431640625f + 0x1p-126f);   // (PointBody::begin)
        this->found = false;
        return al && finite3(mk3(q.x, q.y, q.z)) && q.w >= 0.f;   // (a non-finite world point is non-finite in every instance)
    }
    PSM_D bool enter(const InstGeom& g, int gi) {
        const float4 q = load_point(this->s.rays, idx, alive);
        this->p = inst_point(g.m, mk3(q.x, q.y, q.z));
        ScenePointBody<WITHIN, InstArgs>::enter(g, gi);
        return finite3(this->p);
    }
};

// inside / the sign of a closest-point result over instances: ray k is the WORLD ray {p, 0, PSM_INSIDE_DIRECTIONS[k], +inf},
// moved per instance; its crossings are summed over all instances before it votes
template <bool SIGN>
struct InstInsideBody : SceneInsideBody<SIGN, InstArgs> {
    size_t idx;
    bool alive;
    PSM_D InstInsideBody(const InstArgs& a) : SceneInsideBody<SIGN, InstArgs>(a) {}
    PSM_D bool begin(size_t i, bool al) {
        idx = i;
        alive = al;
        float4 q = make_float4(0.f, 0.f, 0.f, -1.f);
        if (al) q = this->s.rays[i];
        this->k = 0u;
        this->votes = 0u;
        this->count = 0u;
        this->dist = 0.f;
        this->tmin = 0.f;
        this->tmax = __builtin_inff();
        this->valid = al;
        if (SIGN) {
            float4 h = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
            if (al) h = this->s.hits[i];
            this->dist = h.z;
            this->valid = __float_as_int(h.w) >= 0;
        }
        this->valid = finite3(mk3(q.x, q.y, q.z)) && this->valid;   // (a non-finite p: outside)
        return this->valid;
    }
    PSM_D bool enter(const InstGeom& g, int) {
        float4 q = make_float4(0.f, 0.f, 0.f, -1.f);
        if (alive) q = this->s.rays[idx];
        const int r = __builtin_amdgcn_readfirstlane((int)this->k);
        this->o = inst_point(g.m, mk3(q.x, q.y, q.z));
        this->d = normalize3(inst_rotate(g.m, mk3(INSIDE_DIR[r][0], INSIDE_DIR[r][1], INSIDE_DIR[r][2])));
        this->axes(g);
        return finite3(this->o) && finite3(this->d);
    }
    PSM_D bool again() {
        this->votes += this->count & 1u;
        this->k++;
        if (!this->valid || this->k >= this->s.samples) return false;
        this->count = 0u;
        return true;
    }
};

}  // namespace

__global__ __launch_bounds__(QUERY_BLOCK, 8) void inst_query_closest(InstArgs s) { scene_body<InstRayBody<false>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void inst_query_any(InstArgs s) { scene_body<InstRayBody<true>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void inst_query_point(InstArgs s) { scene_body<InstPointBody<false>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void inst_query_within(InstArgs s) { scene_body<InstPointBody<true>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void inst_query_count(InstArgs s) { scene_body<InstCountBody>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void inst_query_inside(InstArgs s) { scene_body<InstInsideBody<false>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void inst_query_sign(InstArgs s) { scene_body<InstInsideBody<true>>(s); }

namespace {

// the stack entries beyond the LDS part, per context, shared by every query kind (all run on the context's stream, never at
// once): one column per lane of a launch (allocated on the context's first query)
constexpr size_t SPILL_BYTES = (size_t)(QSTACK_MAX - QSTACK_LDS) * QUERY_GRID_CAP * QUERY_BLOCK * sizeof(int);
std::mutex spill_mu;
std::unordered_map<const psm_ctx*, void*> spill_area;

int spill_for(psm_ctx* c, void** out) {
    std::lock_guard<std::mutex> lk(spill_mu);
    void*& p = spill_area[c];
    if (!p) PSM_HIP(c, hipMalloc(&p, SPILL_BYTES));
    *out = p;
    return PSM_OK;
}

// ceil(log2(n)) for n >= 1
int ceil_log2(size_t n) {
    int k = 0;
    while (((size_t)1 << k) < n) k++;
    return k;
}

enum QueryKind { Q_CLOSEST, Q_ANY, Q_POINT, Q_WITHIN, Q_COUNT, Q_INSIDE, Q_SIGNED };
// per kind: the single-hierarchy entry point, what the input and the output are called in its messages (out: NULL when its
// alignment is not checked: a byte per query), the output's alignment, the family in the state / capacity texts
struct QueryDesc {
    const char* name;
    const char* in;
    const char* out;
    unsigned out_align;
    bool points;
};
const QueryDesc QUERY_DESC[] = {{"psm_bvh_intersect_dev", "rays", "hits", 16, false},
                                {"psm_bvh_occluded_dev", "rays", nullptr, 1, false},
                                {"psm_bvh_closest_point_dev", "points", "hits", 16, true},
                                {"psm_bvh_within_dev", "points", nullptr, 1, true},
                                {"psm_bvh_count_hits_dev", "rays", "counts", 4, false},
                                {"psm_bvh_inside_dev", "points", nullptr, 1, true},
                                {"psm_bvh_signed_distance_dev", "points", "hits", 16, true}};
const char* const SCENE_NAME[] = {"psm_scene_intersect_dev", "psm_scene_occluded_dev", "psm_scene_closest_point_dev",
                                  "psm_scene_within_dev", "psm_scene_count_hits_dev", "psm_scene_inside_dev",
                                  "psm_scene_signed_distance_dev"};
const char* const INST_NAME[] = {"psm_instances_intersect_dev", "psm_instances_occluded_dev", "psm_instances_closest_point_dev",
                                 "psm_instances_within_dev", "psm_instances_count_hits_dev", "psm_instances_inside_dev",
                                 "psm_instances_signed_distance_dev"};

// a family's seven kernels by QueryKind (Q_SIGNED: the sign kernel)
template <class Args>
struct Kernels {
    void (*k[7])(Args);
};
const Kernels<QueryArgs> BVH_KERNELS = {{bvh_query_closest, bvh_query_any, bvh_query_point, bvh_query_within, bvh_query_count,
                                         bvh_query_inside, bvh_query_sign}};
const Kernels<SceneArgs> SCENE_KERNELS = {{scene_query_closest, scene_query_any, scene_query_point, scene_query_within,
                                           scene_query_count, scene_query_inside, scene_query_sign}};
const Kernels<InstArgs> INST_KERNELS = {{inst_query_closest, inst_query_any, inst_query_point, inst_query_within, inst_query_count,
                                         inst_query_inside, inst_query_sign}};

// The launch of every query. Q_SIGNED is two launches: the family's unchanged closest-point kernel, then the sign of what it
// found (the same stream: in order)
template <class Args>
int launch(psm_ctx* c, const Kernels<Args>& kernels, QueryKind kind, uint32_t grid, const Args& a) {
    if (kind == Q_SIGNED) {
        kernels.k[Q_POINT]<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
        PSM_HIP(c, hipGetLastError());
    }
    kernels.k[kind]<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

// The data checks every query shares, under the entry point's name: in / out must be non-NULL, in 16-byte aligned, out as its
// kind asks (a psm_hit 16 bytes, a count 4); samples (the inside kinds only): 1, 3 or 5. index: what the per-query index array
// (d_geom: the kinds with a psm_hit output only) is called in the messages, NULL for a query that has none. A batch that passes
// makes the context's device the current one.
int check_data(psm_ctx* c, const char* name, const char* index, QueryKind kind, const void* d_in, const void* d_out, const int32_t* d_geom,
               uint32_t samples) {
    const QueryDesc& k = QUERY_DESC[kind];
    char msg[128];
    const bool with_geom = index && k.out_align == 16;
    if (!d_in || !d_out || (with_geom && !d_geom)) {
        snprintf(msg, sizeof msg, "%s: NULL pointer", name);
        return set_err(c, PSM_ERR_INVALID, msg);
    }
    const bool in_bad = ((uintptr_t)d_in & 15u) != 0, out_bad = ((uintptr_t)d_out & (uintptr_t)(k.out_align - 1)) != 0;
    if (in_bad || out_bad) {
        if (k.out_align == 16) snprintf(msg, sizeof msg, "%s: %s or %s not 16-byte aligned", name, k.in, k.out);
        else if (in_bad) snprintf(msg, sizeof msg, "%s: %s not 16-byte aligned", name, k.in);
        else snprintf(msg, sizeof msg, "%s: %s not %u-byte aligned", name, k.out, k.out_align);
        return set_err(c, PSM_ERR_INVALID, msg);
    }
    if (with_geom && ((uintptr_t)d_geom & 3u) != 0) {
        snprintf(msg, sizeof msg, "%s: %s not 4-byte aligned", name, index);
        return set_err(c, PSM_ERR_INVALID, msg);
    }
    if ((kind == Q_INSIDE || kind == Q_SIGNED) && samples != 1 && samples != 3 && samples != 5) {
        snprintf(msg, sizeof msg, "%s: samples must be 1, 3 or 5", name);
        return set_err(c, PSM_ERR_INVALID, msg);
    }
    (void)hipSetDevice(c->device);
    return PSM_OK;
}

// The context's stack area (a context's first query allocates: a later one can be captured into a graph), the grid, and the
// scalars QueryArgs, SceneArgs and InstArgs share
template <class Args>
int batch_args(psm_ctx* c, const void* d_in, size_t n, void* d_out, uint32_t samples, Args& a, uint32_t& grid) {
    void* spill = nullptr;
    const int rc = spill_for(c, &spill);
    if (rc != PSM_OK) return rc;
    const size_t waves = (n + QUERY_BLOCK - 1) / QUERY_BLOCK;
    grid = (uint32_t)(waves < QUERY_GRID_CAP ? waves : QUERY_GRID_CAP);
    a.rays = (const float4*)d_in; a.n = n;
    a.spill = (int*)spill;
    a.hits = (float4*)d_out; a.occluded = (uint8_t*)d_out; a.count = (uint32_t*)d_out;   // (a kernel reads its own)
    a.samples = samples;
    return PSM_OK;
}

bool too_deep(const psm_bvh* b) { return 63 + ceil_log2(b->cap) > QSTACK_MAX; }

// A query of one hierarchy: n == 0 is answered before anything else is looked at; then the data, the state, the depth.
int query(psm_bvh* b, QueryKind kind, const void* d_in, size_t n, void* d_out, uint32_t samples = 0) {
    if (!b) return PSM_ERR_INVALID;
    if (n == 0) return PSM_OK;
    psm_ctx* c = b->ctx;
    const bool points = QUERY_DESC[kind].points;
    int rc = check_data(c, QUERY_DESC[kind].name, nullptr, kind, d_in, d_out, nullptr, samples);
    if (rc != PSM_OK) return rc;
    if (!b->built) return set_err(c, PSM_ERR_STATE, points ? "point query before build" : "ray query before build");
    if (too_deep(b))
        return set_err(c, PSM_ERR_CAPACITY, points ? "point query: hierarchy deeper than the query stack"
                                                   : "ray query: hierarchy deeper than the query stack");
    QueryArgs qa = {};
    uint32_t grid = 0;
    rc = batch_args(c, d_in, n, d_out, samples, qa, grid);
    if (rc != PSM_OK) return rc;
    qa.node32 = b->d_node32; qa.tri48 = b->d_tri48; qa.sm = b->d_small; qa.sorted_tri = b->d_sorted_tri;
    return launch(c, BVH_KERNELS, kind, grid, qa);
}

// Why a pose is refused, or NULL (psm_hip.h): in double, on the host. A rigid motion or a reflection has R^T R = 1; the bound
// leaves room for a matrix that was composed in float32 and refuses every scale or shear a user could mean.
const char* pose_fault(const float* m) {
    for (int k = 0; k < 12; k++)
        if (!std::isfinite(m[k])) return "has a non-finite transform";
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            double dot = 0.0;
            for (int i = 0; i < 3; i++) dot += (double)m[4 * i + a] * (double)m[4 * i + b];
            if (std::fabs(dot - (a == b ? 1.0 : 0.0)) > 1e-5) return "has a transform that is not rigid (R^T R differs from 1 by more than 1e-5)";
        }
    return nullptr;
}

// An entry of a list as the list queries read it: a scene's psm_bvh*, or a psm_instance (a hierarchy and its pose). noun: what
// the messages call it; fault: why the entry itself is refused, or NULL; fill: its row of the kernel-argument table.
struct SceneEntry {
    using Args = SceneArgs;
    static constexpr const char* noun = "geometry";
    static psm_bvh* bvh(psm_bvh* e) { return e; }
    static const char* fault(psm_bvh*) { return nullptr; }
    static void fill(SceneGeom& t, psm_bvh* b) { t = SceneGeom{b->d_node32, b->d_tri48, b->d_small, b->d_sorted_tri}; }
};
struct InstEntry {
    using Args = InstArgs;
    static constexpr const char* noun = "instance";
    static psm_bvh* bvh(const psm_instance& e) { return e.bvh; }
    static const char* fault(const psm_instance& e) { return pose_fault(e.world_from_object); }
    static void fill(InstGeom& t, const psm_instance& e) {
        SceneEntry::fill(t, e.bvh);
        for (int k = 0; k < 12; k++) t.m[k] = e.world_from_object[k];
    }
};

// The list of a scene or an instanced query, checked first and whole, also for n == 0, all of it on the host before any device
// is touched: its length; then every entry's handle (NULL, another context than the first non-NULL entry's), every entry's own
// fault (the poses), every entry's state (not built, too deep for the stack) -- the message naming the first failing index. The
// message goes to the context of the first non-NULL entry, *ctx (a list of NULLs only has no context to tell: the return code alone).
template <class E, class Entry>
int check_list(const Entry* list, uint32_t count, const char* name, psm_ctx** ctx) {
    if (!list || count == 0 || count > PSM_SCENE_MAX_GEOMETRIES) return PSM_ERR_INVALID;
    psm_ctx* c = nullptr;
    for (uint32_t g = 0; g < count && !c; g++)
        if (E::bvh(list[g])) c = E::bvh(list[g])->ctx;
    if (!c) return PSM_ERR_INVALID;
    *ctx = c;
    char msg[160];
    for (uint32_t g = 0; g < count; g++) {
        if (!E::bvh(list[g])) {
            snprintf(msg, sizeof msg, "%s: %s %u is NULL", name, E::noun, g);
            return set_err(c, PSM_ERR_INVALID, msg);
        }
        if (E::bvh(list[g])->ctx != c) {
            snprintf(msg, sizeof msg, "%s: %s %u belongs to another context", name, E::noun, g);
            return set_err(c, PSM_ERR_INVALID, msg);
        }
    }
    for (uint32_t g = 0; g < count; g++)
        if (const char* why = E::fault(list[g])) {
            snprintf(msg, sizeof msg, "%s: %s %u %s", name, E::noun, g, why);
            return set_err(c, PSM_ERR_INVALID, msg);
        }
    for (uint32_t g = 0; g < count; g++) {
        if (!E::bvh(list[g])->built) {
            snprintf(msg, sizeof msg, "%s: %s %u is not built", name, E::noun, g);
            return set_err(c, PSM_ERR_STATE, msg);
        }
        if (too_deep(E::bvh(list[g]))) {
            snprintf(msg, sizeof msg, "%s: %s %u is deeper than the query stack", name, E::noun, g);
            return set_err(c, PSM_ERR_CAPACITY, msg);
        }
    }
    return PSM_OK;
}

// A query of a list (E: SceneEntry or InstEntry): the list, n == 0, the data, the table, the launch. index: what d_geom is
// called in the messages ("geom" / "inst").
template <class E, class Entry>
int list_query(const Entry* list, uint32_t count, const char* name, const char* index, const Kernels<typename E::Args>& kernels,
               QueryKind kind, const void* d_in, size_t n, void* d_out, int32_t* d_geom, uint32_t samples) {
    psm_ctx* c = nullptr;
    int rc = check_list<E>(list, count, name, &c);
    if (rc != PSM_OK || n == 0) return rc;
    rc = check_data(c, name, index, kind, d_in, d_out, d_geom, samples);
    if (rc != PSM_OK) return rc;
    typename E::Args a = {};
    uint32_t grid = 0;
    rc = batch_args(c, d_in, n, d_out, samples, a, grid);
    if (rc != PSM_OK) return rc;
    a.geom = d_geom;
    a.geoms = count;
    for (uint32_t g = 0; g < count; g++) E::fill(a.g[g], list[g]);
    return launch(c, kernels, kind, grid, a);
}

int scene_query(psm_bvh* const* geoms, uint32_t count, QueryKind kind, const void* d_in, size_t n, void* d_out, int32_t* d_geom,
                uint32_t samples = 0) {
    return list_query<SceneEntry>(geoms, count, SCENE_NAME[kind], "geom", SCENE_KERNELS, kind, d_in, n, d_out, d_geom, samples);
}

int inst_query(const psm_instance* insts, uint32_t count, QueryKind kind, const void* d_in, size_t n, void* d_out, int32_t* d_inst,
               uint32_t samples = 0) {
    return list_query<InstEntry>(insts, count, INST_NAME[kind], "inst", INST_KERNELS, kind, d_in, n, d_out, d_inst, samples);
}

}  // namespace

// psm_ctx_destroy (api.hip): the context's spill area goes with it (the stream has been synchronised)
void query_release(psm_ctx* c) {
    std::lock_guard<std::mutex> lk(spill_mu);
    auto it = spill_area.find(c);
    if (it == spill_area.end()) return;
    if (it->second) (void)hipFree(it->second);
    spill_area.erase(it);
}

// world.hip: the context's stack area serves the world queries too (their launches use the same grid cap)
int query_spill(psm_ctx* c, void** out) { return spill_for(c, out); }

}  // namespace psm

int psm_bvh_intersect_dev(psm_bvh* bvh, const psm_query_ray* d_rays, size_t n, psm_hit* d_hits) {
    return psm::query(bvh, psm::Q_CLOSEST, d_rays, n, d_hits);
}

int psm_bvh_occluded_dev(psm_bvh* bvh, const psm_query_ray* d_rays, size_t n, uint8_t* d_hit) {
    return psm::query(bvh, psm::Q_ANY, d_rays, n, d_hit);
}

int psm_bvh_closest_point_dev(psm_bvh* bvh, const psm_point_query* d_points, size_t n, psm_hit* d_hits) {
    return psm::query(bvh, psm::Q_POINT, d_points, n, d_hits);
}

int psm_bvh_within_dev(psm_bvh* bvh, const psm_point_query* d_points, size_t n, uint8_t* d_hit) {
    return psm::query(bvh, psm::Q_WITHIN, d_points, n, d_hit);
}

int psm_bvh_count_hits_dev(psm_bvh* bvh, const psm_query_ray* d_rays, size_t n, uint32_t* d_count) {
    return psm::query(bvh, psm::Q_COUNT, d_rays, n, d_count);
}

int psm_bvh_inside_dev(psm_bvh* bvh, const psm_point_query* d_points, size_t n, uint32_t samples, uint8_t* d_inside) {
    return psm::query(bvh, psm::Q_INSIDE, d_points, n, d_inside, samples);
}

int psm_bvh_signed_distance_dev(psm_bvh* bvh, const psm_point_query* d_points, size_t n, uint32_t samples, psm_hit* d_hits) {
    return psm::query(bvh, psm::Q_SIGNED, d_points, n, d_hits, samples);
}

int psm_scene_intersect_dev(psm_bvh* const* geoms, uint32_t count, const psm_query_ray* d_rays, size_t n, psm_hit* d_hits, int32_t* d_geom) {
    return psm::scene_query(geoms, count, psm::Q_CLOSEST, d_rays, n, d_hits, d_geom);
}

int psm_scene_occluded_dev(psm_bvh* const* geoms, uint32_t count, const psm_query_ray* d_rays, size_t n, uint8_t* d_hit) {
    return psm::scene_query(geoms, count, psm::Q_ANY, d_rays, n, d_hit, nullptr);
}

int psm_scene_closest_point_dev(psm_bvh* const* geoms, uint32_t count, const psm_point_query* d_points, size_t n, psm_hit* d_hits,
                                int32_t* d_geom) {
    return psm::scene_query(geoms, count, psm::Q_POINT, d_points, n, d_hits, d_geom);
}

int psm_scene_within_dev(psm_bvh* const* geoms, uint32_t count, const psm_point_query* d_points, size_t n, uint8_t* d_hit) {
    return psm::scene_query(geoms, count, psm::Q_WITHIN, d_points, n, d_hit, nullptr);
}

int psm_scene_count_hits_dev(psm_bvh* const* geoms, uint32_t count, const psm_query_ray* d_rays, size_t n, uint32_t* d_count) {
    return psm::scene_query(geoms, count, psm::Q_COUNT, d_rays, n, d_count, nullptr);
}

int psm_scene_inside_dev(psm_bvh* const* geoms, uint32_t count, const psm_point_query* d_points, size_t n, uint32_t samples,
                         uint8_t* d_inside) {
    return psm::scene_query(geoms, count, psm::Q_INSIDE, d_points, n, d_inside, nullptr, samples);
}

int psm_scene_signed_distance_dev(psm_bvh* const* geoms, uint32_t count, const psm_point_query* d_points, size_t n, uint32_t samples,
                                  psm_hit* d_hits, int32_t* d_geom) {
    return psm::scene_query(geoms, count, psm::Q_SIGNED, d_points, n, d_hits, d_geom, samples);
}

int psm_instances_intersect_dev(const psm_instance* insts, uint32_t count, const psm_query_ray* d_rays, size_t n, psm_hit* d_hits,
                                int32_t* d_inst) {
    return psm::inst_query(insts, count, psm::Q_CLOSEST, d_rays, n, d_hits, d_inst);
}

int psm_instances_occluded_dev(const psm_instance* insts, uint32_t count, const psm_query_ray* d_rays, size_t n, uint8_t* d_hit) {
    return psm::inst_query(insts, count, psm::Q_ANY, d_rays, n, d_hit, nullptr);
}

int psm_instances_closest_point_dev(const psm_instance* insts, uint32_t count, const psm_point_query* d_points, size_t n, psm_hit* d_hits,
                                    int32_t* d_inst) {
    return psm::inst_query(insts, count, psm::Q_POINT, d_points, n, d_hits, d_inst);
}

int psm_instances_within_dev(const psm_instance* insts, uint32_t count, const psm_point_query* d_points, size_t n, uint8_t* d_hit) {
    return psm::inst_query(insts, count, psm::Q_WITHIN, d_points, n, d_hit, nullptr);
}

int psm_instances_count_hits_dev(const psm_instance* insts, uint32_t count, const psm_query_ray* d_rays, size_t n, uint32_t* d_count) {
    return psm::inst_query(insts, count, psm::Q_COUNT, d_rays, n, d_count, nullptr);
}

int psm_instances_inside_dev(const psm_instance* insts, uint32_t count, const psm_point_query* d_points, size_t n, uint32_t samples,
                             uint8_t* d_inside) {
    return psm::inst_query(insts, count, psm::Q_INSIDE, d_points, n, d_inside, nullptr, samples);
}

int psm_instances_signed_distance_dev(const psm_instance* insts, uint32_t count, const psm_point_query* d_points, size_t n,
                                      uint32_t samples, psm_hit* d_hits, int32_t* d_inst) {
    return psm::inst_query(insts, count, psm::Q_SIGNED, d_points, n, d_hits, d_inst, samples);
}
