// psm_box_dev.h -- the device pieces the box kernels share (box.hip, world_box.hip): the candidate test
// box_tri with its helpers, and box_row, a row of an affine map applied to a box. Moved here from box.hip as they were; box.hip's
// three kernels compile to the same instructions as with the pieces in their own file (tools/kernel_diff.py).
#pragma once
#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"

namespace psm {

namespace {

// one term of bmin(a): a >= 0 ? a L : a H (bmax: the same with L and H swapped)
PSM_D float bterm(float a, float l, float h) { return a >= 0.f ? a * l : a * h; }

// does the axis with the triangle's projections {0, p} (relative to v0) and the box's [bmin, bmax] separate them
PSM_D bool separates(float p, float bmin, float bmax) {
    const float pmx = p > 0.f ? p : 0.f, pmn = p < 0.f ? p : 0.f;
    return !(pmx >= bmin && pmn <= bmax);
}

// an edge axis unit_k x f: its two components that are not zero by construction, a1 on the axis of (l1, h1) and a2 on the axis
// of (l2, h2) in component order, and the matching components g1, g2 of the edge whose projection is the triangle's other value
PSM_D bool edge_separates(float a1, float a2, float l1, float h1, float l2, float h2, float g1, float g2) {
    const float bmin = bterm(a1, l1, h1) + bterm(a2, l2, h2);
    const float bmax = bterm(a1, h1, l1) + bterm(a2, h2, l2);
    return separates(a1 * g1 + a2 * g2, bmin, bmax);
}

// the three edge axes of f (unit_x x f, unit_y x f, unit_z x f) with g the edge that gives the projection
PSM_D bool edge_axes_separate(v3 f, v3 g, v3 L, v3 H) {
    bool sep = edge_separates(-f.z, f.y, L.y, H.y, L.z, H.z, g.y, g.z);   // (0, -fz, fy)
    sep |= edge_separates(f.z, -f.x, L.x, H.x, L.z, H.z, g.x, g.z);       // (fz, 0, -fx)
    sep |= edge_separates(-f.y, f.x, L.x, H.x, L.y, H.y, g.x, g.y);       // (-fy, fx, 0)
    return sep;
}

// a unit axis: the triangle's {0, a, b} against [l, h] directly
PSM_D bool unit_separates(float a, float b, float l, float h) {
    float pmx = a > 0.f ? a : 0.f, pmn = a < 0.f ? a : 0.f;
    pmx = b > pmx ? b : pmx;
    pmn = b < pmn ? b : pmn;
    return !(pmx >= l && pmn <= h);
}

// The candidate test (include/psm_hip.h "box queries" states it; tests/box_query_model.py restates it in numpy): triangle
// (v0, e1, e2) against the closed box [lo, hi], one float32 operation order, no division, no square root.
PSM_D bool box_tri(v3 v0, v3 e1, v3 e2, v3 lo, v3 hi) {
    const v3 L = lo - v0, H = hi - v0;
    const v3 f3 = e2 - e1;
    bool sep = unit_separates(e1.x, e2.x, L.x, H.x);
    sep |= unit_separates(e1.y, e2.y, L.y, H.y);
    sep |= unit_separates(e1.z, e2.z, L.z, H.z);
    sep |= edge_axes_separate(e1, e2, L, H);
    sep |= edge_axes_separate(e2, e1, L, H);
    sep |= edge_axes_separate(f3, e1, L, H);
    const v3 n = cross3(e1, e2);
    const float bmin = (bterm(n.x, L.x, H.x) + bterm(n.y, L.y, H.y)) + bterm(n.z, L.z, H.z);
    const float bmax = (bterm(n.x, H.x, L.x) + bterm(n.y, H.y, L.y)) + bterm(n.z, H.z, L.z);
    sep |= separates(0.f, bmin, bmax);
    return !sep;
}

// Row k of the build's affine map applied to the box [lo, hi]: the interval of the image on normalised axis k, the sums in
// affine_row's order, grown by affine_row's margin h = 2^-16 (2 + S) with S the sum of the larger magnitudes and |m3|. For a
// diagonal 3 x 3 part (the plain fit) the interval is the image; for a full one (an optimisation matrix) it is the image's
// bounding interval, which the row sums make right. DESIGN.md 4.15 has why no triangle that counts is cut.
PSM_D void box_row(const float* M, int k, v3 lo, v3 hi, float& glo, float& ghi) {
    const float m0 = M[4 * k + 0], m1 = M[4 * k + 1], m2 = M[4 * k + 2], m3 = M[4 * k + 3];
    const float ax = m0 * lo.x, bx = m0 * hi.x, ay = m1 * lo.y, by = m1 * hi.y, az = m2 * lo.z, bz = m2 * hi.z;
    const float ilo = ((sminf(ax, bx) + sminf(ay, by)) + sminf(az, bz)) + m3;
    const float ihi = ((smaxf(ax, bx) + smaxf(ay, by)) + smaxf(az, bz)) + m3;
    const float S = ((smaxf(pabs(ax), pabs(bx)) + smaxf(pabs(ay), pabs(by))) + smaxf(pabs(az), pabs(bz))) + pabs(m3);
    const float h = (2.0f + S) * 0x1p-16f;
    glo = ilo - h;
    ghi = ihi + h;
}

}  // namespace

}  // namespace psm
