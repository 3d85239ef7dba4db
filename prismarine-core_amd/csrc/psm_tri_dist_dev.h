// psm_tri_dist_dev.h -- the candidate test of the clearance queries (tri_dist.hip; include/psm_hip.h "clearance queries",
// DESIGN.md 4.23): tri_dist, the distance between a stored triangle (v0, e1, e2) and a query triangle (a, b, c) in float32 with
// the weights of the two nearest points, and seg_seg, the clamped closest points of two segments. One operation order, one
// rounding per operation (-ffp-contract=off), division and sqrtf correctly rounded. It also compiles for the host: a stand-alone
// program defines PSM_TRI_FN and PSM_POINT_FN as a host function's decoration before it includes this file
// (tests/cpp/tri_dist_host.cpp), and the CPU test holds what it computes against tests/tri_dist_query_model.py bit for bit.
#pragma once
#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"   // closest_on_tri, clamp01
#include "psm_tri_dev.h"     // tri_tri

namespace psm {

namespace {

// The clamped closest points of the segments p1 + x d1 and p2 + y d2, x, y in [0, 1] (Ericson, Real-Time Collision Detection
// 5.1.9), branch-free: x from the two lines' normal equations, y the best for that x, then x the best for that y. Ericson takes
// the last step only when y was clamped; taken always it changes nothing in real numbers (an optimum is a fixed point of it)
// and for a parallel pair, which starts from x = 0, it is what finds the overlap.
// Guards, in closest_on_tri's spirit (finite weights in [0, 1] for every finite input):
//   * a zero-length segment is its point: its weight is 0 and no division by its squared length is made
//   * the pair is taken as parallel unless den = a e - b^2 (= |d1 x d2|^2) exceeds 2^-16 a e (sin^2 of the angle between them),
//     where closest_on_tri's det has its threshold: the rounding of den is a few eps a e, so below it x would be noise. A
//     zero-length segment, an overflow (inf - inf) and a NaN all fail the comparison and land here
//   * every clamp is clamp01: a NaN quotient (0 / 0 cannot occur; inf / inf after an overflow can) becomes 0
PSM_TRI_FN void seg_seg(v3 p1, v3 d1, v3 p2, v3 d2, float& X, float& Y) {
    const v3 r = p1 - p2;
    const float a = dot3(d1, d1), e = dot3(d2, d2), b = dot3(d1, d2);
    const float c = dot3(d1, r), f = dot3(d2, r);
    const float den = a * e - b * b;
    const bool skew = den > (a * e) * 0x1p-16f;
    const float x0 = clamp01((skew ? b * f - c * e : 0.f) / (skew ? den : 1.f));
    const bool ye = e > 0.f, xa = a > 0.f;
    const float y = clamp01((ye ? b * x0 + f : 0.f) / (ye ? e : 1.f));
    const float x = clamp01((xa ? b * y - c : 0.f) / (xa ? a : 1.f));
    X = x;
    Y = y;
}

// what tri_dist keeps of a pair: the squared distance and the weights of the two nearest points, (u, v) of e1, e2 on the stored
// triangle and (s, t) of g1 = b - a, g2 = c - a on the query triangle
struct TriDist {
    float d2, u, v, s, t;
};

// d2 of four weights, the same way for every feature: Q = (A + s g1) + t g2, P = u e1 + v e2, d2 = dot3(Q - P, Q - P)
PSM_TRI_FN float tri_dist_d2(v3 e1, v3 e2, v3 A, v3 g1, v3 g2, float u, float v, float s, float t) {
    const v3 Q = mk3((A.x + s * g1.x) + t * g2.x, (A.y + s * g1.y) + t * g2.y, (A.z + s * g1.z) + t * g2.z);
    const v3 P = mk3(u * e1.x + v * e2.x, u * e1.y + v * e2.y, u * e1.z + v * e2.z);
    const v3 w = Q - P;
    return dot3(w, w);
}

// a later feature replaces the winner only with a smaller d2: a bit-equal d2 keeps the first, a NaN replaces nothing
PSM_TRI_FN void tri_dist_offer(TriDist& w, v3 e1, v3 e2, v3 A, v3 g1, v3 g2, float u, float v, float s, float t) {
    const float d2 = tri_dist_d2(e1, e2, A, g1, g2, u, v, s, t);
    if (d2 < w.d2) { w.d2 = d2; w.u = u; w.v = v; w.s = s; w.t = t; }
}

// The candidate test (include/psm_hip.h "clearance queries" states it; tests/tri_dist_query_model.py restates it in numpy):
// everything relative to the stored v0, as tri_tri has it, so the overlap test and the distances see the same rounded
// coordinates. Fifteen features in a fixed order -- the query's vertices against the stored triangle, the stored vertices
// against the query triangle (closest_on_tri both ways), the nine edge pairs in tri_tri's order (seg_seg) --, each judged by
// tri_dist_d2 of its weights; the smallest d2 wins, the first on a bit-equal one. Where tri_tri holds the pair's d2 is 0: two
// triangles that meet have clearance 0, and an edge that pierces a face leaves all fifteen positive. The weights are then
// STILL the fifteen features' winner: where the two boundaries come closest, not a point of the intersection.
PSM_TRI_FN TriDist tri_dist(v3 v0, v3 e1, v3 e2, v3 a, v3 b, v3 c) {
    const v3 A = a - v0, B = b - v0, C = c - v0;
    const v3 g1 = B - A, g2 = C - A, g3 = C - B;
    const v3 e3 = e2 - e1;
    const v3 O = mk3(0.f, 0.f, 0.f);
    TriDist w;
    float x, y;
    // F0 - F2: a, b, c against the stored triangle
    closest_on_tri(v0, e1, e2, a, x, y);
    w.u = x; w.v = y; w.s = 0.f; w.t = 0.f;
    w.d2 = tri_dist_d2(e1, e2, A, g1, g2, x, y, 0.f, 0.f);
    closest_on_tri(v0, e1, e2, b, x, y);
    tri_dist_offer(w, e1, e2, A, g1, g2, x, y, 1.f, 0.f);
    closest_on_tri(v0, e1, e2, c, x, y);
    tri_dist_offer(w, e1, e2, A, g1, g2, x, y, 0.f, 1.f);
    // F3 - F5: the stored vertices 0, e1, e2 against the query triangle {A, g1, g2}
    closest_on_tri(A, g1, g2, O, x, y);
    tri_dist_offer(w, e1, e2, A, g1, g2, 0.f, 0.f, x, y);
    closest_on_tri(A, g1, g2, e1, x, y);
    tri_dist_offer(w, e1, e2, A, g1, g2, 1.f, 0.f, x, y);
    closest_on_tri(A, g1, g2, e2, x, y);
    tri_dist_offer(w, e1, e2, A, g1, g2, 0.f, 1.f, x, y);
    // F6 - F14: the edge pairs e_i, g_j, i outer, j inner. e1 and e2 start at 0, e3 at e1; g1 and g2 start at A, g3 at B. A
    // weight x along e1 / e2 / e3 is (u, v) = (x, 0) / (0, x) / (1 - x, x), and y along g1 / g2 / g3 likewise for (s, t)
    seg_seg(O, e1, A, g1, x, y);
    tri_dist_offer(w, e1, e2, A, g1, g2, x, 0.f, y, 0.f);
    seg_seg(O, e1, A, g2, x, y);
    tri_dist_offer(w, e1, e2, A, g1, g2, x, 0.f, 0.f, y);
    seg_seg(O, e1, B, g3, x, y);
    tri_dist_offer(w, e1, e2, A, g1, g2, x, 0.f, 1.f - y, y);
    seg_seg(O, e2, A, g1, x, y);
    tri_dist_offer(w, e1, e2, A, g1, g2, 0.f, x, y, 0.f);
    seg_seg(O, e2, A, g2, x, y);
    tri_dist_offer(w, e1, e2, A, g1, g2, 0.f, x, 0.f, y);
    seg_seg(O, e2, B, g3, x, y);
    tri_dist_offer(w, e1, e2, A, g1, g2, 0.f, x, 1.f - y, y);
    seg_seg(e1, e3, A, g1, x, y);
    tri_dist_offer(w, e1, e2, A, g1, g2, 1.f - x, x, y, 0.f);
    seg_seg(e1, e3, A, g2, x, y);
    tri_dist_offer(w, e1, e2, A, g1, g2, 1.f - x, x, 0.f, y);
    seg_seg(e1, e3, B, g3, x, y);
    tri_dist_offer(w, e1, e2, A, g1, g2, 1.f - x, x, 1.f - y, y);
    if (tri_tri(v0, e1, e2, a, b, c)) w.d2 = 0.f;
    return w;
}

// LB^2 of one child box (mn / mx: its fp16 corners) against the grown image interval [gl, gh] of the query's bounding box per
// normalised axis: PointImage::lb2 with the gap to an interval (a NaN gap is 0: kept). tri_dist.hip's prune and, with a world's
// intervals, world_tri_dist.hip's (psm_query_dev.h has the bound's derivation)
PSM_D float tri_dist_lb2(const PointBound& B, float glx, float gly, float glz, float ghx, float ghy, float ghz, float mnx, float mny,
                         float mnz, float mxx, float mxy, float mxz) {
    const float tx = smaxf(smaxf(mnx - ghx, glx - mxx), 0.f) * B.il0;
    const float ty = smaxf(smaxf(mny - ghy, gly - mxy), 0.f) * B.il1;
    const float tz = smaxf(smaxf(mnz - ghz, glz - mxz), 0.f) * B.il2;
    const float m = smaxf(smaxf(tx, ty), tz);
    return (B.orth ? ((tx * tx + ty * ty) + tz * tz) : m * m) * B.wf;
}

}  // namespace

}  // namespace psm
