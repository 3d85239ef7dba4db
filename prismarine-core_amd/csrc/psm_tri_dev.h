// psm_tri_dev.h -- the candidate test of the triangle queries (tri.hip; include/psm_hip.h "triangle queries"):
// tri_tri, a closed separating-axis test of a stored triangle (v0, e1, e2) and a query triangle (a, b, c) in float32 with its
// helpers. Multiplications, additions, subtractions and compares only, one operation order, one rounding per operation
// (-ffp-contract=off). It also compiles for the host: a stand-alone program defines PSM_TRI_FN as a host function's decoration
// before it includes this file (tests/cpp/tri_tri_host.cpp), and the CPU test holds what it computes against
// tests/tri_query_model.py pair for pair. The prune of the kernels is the box family's box_row (psm_box_dev.h) on the query's
// bounding box; box_tri's unit_separates is device code, so its selections are restated here (tri_max3 / tri_min3 with a
// leading 0 are its pmx / pmn, operation for operation).
#pragma once
#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"
#include "psm_box_dev.h"   // box_row (device only)

#ifndef PSM_TRI_FN
#define PSM_TRI_FN PSM_D
#endif

namespace psm {

namespace {

// the largest / smallest of three projections, by selections in this order (y against x, then z against the result)
PSM_TRI_FN float tri_max3(float x, float y, float z) {
    float m = y > x ? y : x;
    m = z > m ? z : m;
    return m;
}
PSM_TRI_FN float tri_min3(float x, float y, float z) {
    float m = y < x ? y : x;
    m = z < m ? z : m;
    return m;
}

// do the intervals [tmin, tmax] (the stored triangle's) and [qmin, qmax] (the query's) miss each other: closed, and a NaN bound
// separates
PSM_TRI_FN bool tri_apart(float tmin, float tmax, float qmin, float qmax) { return !(tmax >= qmin && qmax >= tmin); }

// a unit axis k, no product: {0, e1_k, e2_k} against {A_k, B_k, C_k}
PSM_TRI_FN bool tri_unit_separates(float e1, float e2, float a, float b, float c) {
    return tri_apart(tri_min3(0.f, e1, e2), tri_max3(0.f, e1, e2), tri_min3(a, b, c), tri_max3(a, b, c));
}

// a general axis: {0, ax . e1, ax . e2} against {ax . A, ax . B, ax . C} (dot3: (x x + y y) + z z). A zero axis projects
// everything to 0 and separates nothing
PSM_TRI_FN bool tri_axis_separates(v3 ax, v3 e1, v3 e2, v3 A, v3 B, v3 C) {
    const float p1 = dot3(ax, e1), p2 = dot3(ax, e2);
    const float qa = dot3(ax, A), qb = dot3(ax, B), qc = dot3(ax, C);
    return tri_apart(tri_min3(0.f, p1, p2), tri_max3(0.f, p1, p2), tri_min3(qa, qb, qc), tri_max3(qa, qb, qc));
}

// The candidate test (include/psm_hip.h "triangle queries" states it; tests/tri_query_model.py restates it in numpy): the
// stored triangle (v0, e1, e2) against the query triangle (a, b, c), everything relative to v0, 20 axes in a fixed order:
// the 3 unit axes, the two normals, the 9 edge pairs, the 6 in-plane axes that decide coplanar pairs.
PSM_TRI_FN bool tri_tri(v3 v0, v3 e1, v3 e2, v3 a, v3 b, v3 c) {
    const v3 A = a - v0, B = b - v0, C = c - v0;
    bool sep = tri_unit_separates(e1.x, e2.x, A.x, B.x, C.x);
    sep |= tri_unit_separates(e1.y, e2.y, A.y, B.y, C.y);
    sep |= tri_unit_separates(e1.z, e2.z, A.z, B.z, C.z);
    const v3 e3 = e2 - e1;
    const v3 g1 = B - A, g2 = C - A, g3 = C - B;
    const v3 n = cross3(e1, e2), m = cross3(g1, g2);
    sep |= tri_axis_separates(n, e1, e2, A, B, C);
    sep |= tri_axis_separates(m, e1, e2, A, B, C);
    sep |= tri_axis_separates(cross3(e1, g1), e1, e2, A, B, C);
    sep |= tri_axis_separates(cross3(e1, g2), e1, e2, A, B, C);
    sep |= tri_axis_separates(cross3(e1, g3), e1, e2, A, B, C);
    sep |= tri_axis_separates(cross3(e2, g1), e1, e2, A, B, C);
    sep |= tri_axis_separates(cross3(e2, g2), e1, e2, A, B, C);
    sep |= tri_axis_separates(cross3(e2, g3), e1, e2, A, B, C);
    sep |= tri_axis_separates(cross3(e3, g1), e1, e2, A, B, C);
    sep |= tri_axis_separates(cross3(e3, g2), e1, e2, A, B, C);
    sep |= tri_axis_separates(cross3(e3, g3), e1, e2, A, B, C);
    sep |= tri_axis_separates(cross3(n, e1), e1, e2, A, B, C);
    sep |= tri_axis_separates(cross3(n, e2), e1, e2, A, B, C);
    sep |= tri_axis_separates(cross3(n, e3), e1, e2, A, B, C);
    sep |= tri_axis_separates(cross3(m, g1), e1, e2, A, B, C);
    sep |= tri_axis_separates(cross3(m, g2), e1, e2, A, B, C);
    sep |= tri_axis_separates(cross3(m, g3), e1, e2, A, B, C);
    return !sep;
}

}  // namespace

}  // namespace psm
