// psm_sweep_dev.h -- the pieces of the sphere sweep a kernel file shares (sweep.hip, world_sweep.hip; include/psm_hip.h "sweep
// queries"): the candidate test sweep_tri with its helpers, and sweep_axis, one axis of the swept sphere in the
// build's normalised space. sweep_tri_from -- sweep_tri given the closest point of the start, which is closest_on_tri's
// (psm_query_dev.h, device only) -- also compiles for the host: a stand-alone program defines PSM_SWEEP_FN as a host function's
// decoration before it includes this file (tests/cpp/sweep_tri_host.cpp), and the CPU test holds what it computes bit for bit
// against tests/sweep_query_model.py.
// One float32 operation order, one rounding per operation (-ffp-contract=off), division and sqrtf correctly rounded.
#pragma once
#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"

#ifndef PSM_SWEEP_FN
#define PSM_SWEEP_FN PSM_D
#endif

namespace psm {

namespace {

// a candidate's first contact: t = +inf (u = v = 0) when there is none
struct SweepHit {
    float t, u, v;
};

// a + s b per component
PSM_SWEEP_FN v3 along(v3 a, float s, v3 b) { return mk3(a.x + s * b.x, a.y + s * b.y, a.z + s * b.z); }
// a - s b per component
PSM_SWEEP_FN v3 back(v3 a, float s, v3 b) { return mk3(a.x - s * b.x, a.y - s * b.y, a.z - s * b.z); }

// When the ball of squared radius rr around the point m + t dp (a = dp . dp) first holds the origin, by closest approach: t0
// the time of the closest approach, l the offset there, qq = rr - l . l what is left of the radius; the entry lies
// sqrtf(qq / a) before t0. The textbook quadratic's c = m . m - rr cancels where the closest approach's l . l does not
// (DESIGN.md 4.17). ok: a > 0, t0 > 0 (approaching), qq >= 0 (the line reaches the ball). An entry before the start -- the
// origin is already inside the ball and still approaching -- is a contact at the start: t = 0 (started()). The value is noise
// when !ok.
PSM_SWEEP_FN float started(float t) { return t > 0.f ? t : 0.f; }
PSM_SWEEP_FN float approach(v3 m, v3 dp, float a, float rr, bool& ok) {
    const float t0 = -dot3(m, dp) / a;
    const v3 l = along(m, t0, dp);
    const float qq = rr - dot3(l, l);
    ok = a > 0.f && t0 > 0.f && qq >= 0.f;
    return started(t0 - sqrtf(qq / a));
}

// the smaller of the best so far and a feature's contact (a tie keeps the earlier feature)
PSM_SWEEP_FN void sweep_take(SweepHit& best, bool ok, float t, float u, float v) {
    if (ok && t < best.t) { best.t = t; best.u = u; best.v = v; }
}

// an edge q + s e, s in [0, 1]: the axial part of the motion is taken out first (sm, sn: the axial coordinates of o - q and of
// d per unit of e), the rest is a point against a circle; s = sm + t sn is where on the edge. A zero-length edge never counts.
PSM_SWEEP_FN float sweep_edge(v3 q, v3 e, v3 o, v3 d, float rr, float& s, bool& ok) {
    const float ee = dot3(e, e);
    const v3 m = o - q;
    const float sm = dot3(m, e) / ee, sn = dot3(d, e) / ee;
    const v3 mp = back(m, sm, e), dp = back(d, sn, e);
    const float t = approach(mp, dp, dot3(dp, dp), rr, ok);
    s = sm + t * sn;
    ok = ok && ee > 0.f && s >= 0.f && s <= 1.f;
    return t;
}

// The first contact with the seven features of triangle (v0, e1, e2) of a sphere of radius r that starts at o, moves along d
// and does NOT touch the triangle at t = 0 as closest_on_tri sees it (sweep_tri decides that): the smallest valid t >= 0, a tie
// going to the earlier of face, v0, v1, v2, edge v0 v1, edge v0 v2, edge v1 v2. A feature the sphere is moving towards and
// already reaches at the start gives t = 0: the start test and the features round independently, and without this a sphere
// that rests on a triangle within rounding of its radius -- where every sweep leaves it -- and moves into it would be seen by
// neither. include/psm_hip.h states it; tests/sweep_query_model.py restates it.
PSM_SWEEP_FN SweepHit sweep_features(v3 v0, v3 e1, v3 e2, v3 o, v3 d, float r) {
    SweepHit best = {__builtin_inff(), 0.f, 0.f};
    const float rr = r * r, dd = dot3(d, d);
    const float aa = dot3(e1, e1), ab = dot3(e1, e2), bb = dot3(e2, e2);
    const float det = aa * bb - ab * ab;
    const v3 w0 = o - v0;
    bool ok;
    {   // the face (closest_on_tri's sliver rule: a thinner triangle has none), from the side the centre is on
        const v3 n = cross3(e1, e2);
        const float s0 = dot3(n, w0), sd = dot3(n, d), rn = r * sqrtf(dot3(n, n));
        const float t = started(((s0 > 0.f ? rn : -rn) - s0) / sd);   // (|s0| <= rn: the plane is reached already)
        const v3 w = along(w0, t, d);
        const float p1 = dot3(w, e1), p2 = dot3(w, e2);
        const float u = (bb * p1 - ab * p2) / det, v = (aa * p2 - ab * p1) / det;
        ok = det > (aa * bb) * 0x1p-16f && s0 * sd < 0.f && u >= 0.f && v >= 0.f && u + v <= 1.f;
        sweep_take(best, ok, t, u, v);
    }
    const v3 q1 = v0 + e1, q2 = v0 + e2;
    float t = approach(w0, d, dd, rr, ok);
    sweep_take(best, ok, t, 0.f, 0.f);
    t = approach(o - q1, d, dd, rr, ok);
    sweep_take(best, ok, t, 1.f, 0.f);
    t = approach(o - q2, d, dd, rr, ok);
    sweep_take(best, ok, t, 0.f, 1.f);
    float s;
    t = sweep_edge(v0, e1, o, d, rr, s, ok);
    sweep_take(best, ok, t, s, 0.f);
    t = sweep_edge(v0, e2, o, d, rr, s, ok);
    sweep_take(best, ok, t, 0.f, s);
    t = sweep_edge(q1, e2 - e1, o, d, rr, s, ok);
    sweep_take(best, ok, t, 1.f - s, s);
    return best;
}

// The candidate test from the closest point of the triangle to the start o (d2 its squared distance, cu, cv its weights): a
// sphere that touches the triangle where it starts -- sqrtf(d2) <= r, the predicate of the within query -- has t = 0 and the
// closest point's (u, v); any other the first contact with the features (0 as well when a feature finds the start touching).
// The caller holds t against tmax.
PSM_SWEEP_FN SweepHit sweep_tri_from(float d2, float cu, float cv, v3 v0, v3 e1, v3 e2, v3 o, v3 d, float r) {
    SweepHit h = sweep_features(v0, e1, e2, o, d, r);
    if (sqrtf(d2) <= r) { h.t = 0.f; h.u = cu; h.v = cv; }
    return h;
}

// The candidate test: the first contact of the swept sphere with triangle (v0, e1, e2) as the build stores it; the start is
// closest_on_tri, the point queries' function bit for bit
PSM_D SweepHit sweep_tri(v3 v0, v3 e1, v3 e2, v3 o, v3 d, float r) {
    float cu, cv;
    const float d2 = closest_on_tri(v0, e1, e2, o, cu, cv);
    return sweep_tri_from(d2, cu, cv, v0, e1, e2, o, d, r);
}

// One axis of the swept sphere in the build's normalised space: ray_axis (psm_query_dev.h) with the box grown by
//   H = h + W r + 2^-11 (2 + S + W r)
// instead of h alone. h = 2^-16 (2 + S) is ray_axis's own margin (the rounding of the image and of the slab); W = |m0| + |m1| +
// |m2|, the row sum, is at least the row's norm, so the image of the sphere around a centre lies within W r of the centre's image
// on this axis (the Minkowski sum of a box and the sphere's image lies in the box grown by W r per axis); the last term holds
// the image of the leaf test's residual -- at its reported t the centre is within r + delta of the triangle, delta measured,
// not proven -- and the rounding of H itself (DESIGN.md 4.17 has the chain and its observed-to-granted ratios).
// P, S and h are affine_row's, operation for operation (written out: this function also compiles for the host, where the
// stand-alone program holds it bit for bit against the model's sweep_axis).
PSM_SWEEP_FN Axis sweep_axis(const float* M, int k, v3 o, v3 d, float r) {
    const float m0 = M[4 * k + 0], m1 = M[4 * k + 1], m2 = M[4 * k + 2], m3 = M[4 * k + 3];
    Row row;
    row.P = ((m0 * o.x + m1 * o.y) + m2 * o.z) + m3;
    row.h = (2.0f + (((pabs(m0 * o.x) + pabs(m1 * o.y)) + pabs(m2 * o.z)) + pabs(m3))) * 0x1p-16f;
    const float W = (pabs(m0) + pabs(m1)) + pabs(m2);
    const float H = row.h * 33.0f + (W * r) * 1.00048828125f;   // h + 2^-11 (2 + S) = 33 h; W r (1 + 2^-11)
    float D = (m0 * d.x + m1 * d.y) + m2 * d.z;
    if (!(pabs(D) >= 1e-20f)) D = __builtin_copysignf(1e-20f, D);
    Axis a;
    a.inv = 1.0f / D;
    a.nlo = -(row.P + H) * a.inv;
    a.nhi = (H - row.P) * a.inv;
    return a;
}

}  // namespace

}  // namespace psm
