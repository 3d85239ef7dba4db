"""A numpy float32 restatement of the point queries (psm_bvh_closest_point_dev / psm_bvh_within_dev, include/psm_hip.h;
query.hip, closest_on_tri).

Every operation is one float32 numpy operation in the order query.hip writes it (the library builds with -ffp-contract=off, so
each float32 operation rounds once, as numpy's do; division and sqrt are correctly rounded on both sides). Selections are
np.where on the same comparisons the kernel's branches make, so -0, NaN and clamps come out bit for bit. The brute force here is
the yardstick of tests/test_point_query_cpu.py and tests/test_gpu_point_query.py."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from query_model import dot3

F = np.float32
# a face whose Gram determinant aa bb - ab^2 is at most 2^-16 aa bb (sin^2 of its smallest angle at v0 <= 2^-16) is taken as the
# segment of its longest edge (include/psm_hip.h)
SLIVER = F(2.0 ** -16)


def _split(tris):
    tris = np.asarray(tris, F).reshape(-1, 3, 3)
    return tris[:, 0, :], tris[:, 1, :] - tris[:, 0, :], tris[:, 2, :] - tris[:, 0, :]   # bvh_prepare_tris: v0, e1, e2


def _clamp01(x):
    """(x > 0 ? x : 0) then (x < 1 ? x : 1): NaN and -0 go to +0"""
    x = np.where(x > F(0), x, F(0))
    return np.where(x < F(1), x, F(1))


def closest_on_tris(v0, e1, e2, p):
    """closest_on_tri for every pair: v0 / e1 / e2 [..., 3] and p [..., 3] broadcast. Returns u, v (weights of e1, e2) and d2."""
    with np.errstate(all="ignore"):
        ap = p - v0
        aa, ab, bb = dot3(e1, e1), dot3(e1, e2), dot3(e2, e2)
        d1, d2 = dot3(e1, ap), dot3(e2, ap)
        d3, d4, d5, d6 = d1 - aa, d2 - ab, d1 - ab, d2 - bb
        vc = aa * d2 - ab * d1
        vb = bb * d1 - ab * d2
        va = d3 * d6 - d5 * d4
        den_ab = d1 - d3
        den_ac = d2 - d6
        e43, e56 = d4 - d3, d5 - d6
        den_bc = e43 + e56
        det = aa * bb - ab * ab
        # the face: clamped into the triangle
        fu = vb / det
        fu = _clamp01(fu)
        fv = vc / det
        fv = np.where(fv > F(0), fv, F(0))
        lim = F(1) - fu
        fv = np.where(fv < lim, fv, lim)
        # a sliver: the clamped projection onto its longest edge
        e21 = e2 - e1
        cc = dot3(e21, e21)
        ta = _clamp01(d1 / aa)
        tb = _clamp01(d2 / bb)
        tc = _clamp01(e43 / cc)
        a_long = (aa >= bb) & (aa >= cc)
        b_long = ~a_long & (bb >= cc)
        su = np.where(a_long, ta, np.where(b_long, F(0), F(1) - tc))
        sv = np.where(a_long, F(0), np.where(b_long, tb, tc))
        face = det > aa * bb * SLIVER
        fu, fv = np.where(face, fu, su), np.where(face, fv, sv)
        # Ericson's regions, first match wins; an edge region with a non-positive denominator is not taken
        w_bc = e43 / den_bc
        conds = [(d1 <= F(0)) & (d2 <= F(0)),                                                    # vertex v0
                 (d3 >= F(0)) & (d4 <= d3),                                                      # vertex v1
                 (vc <= F(0)) & (d1 >= F(0)) & (d3 <= F(0)) & (den_ab > F(0)),                   # edge v0 v1
                 (d6 >= F(0)) & (d5 <= d6),                                                      # vertex v2
                 (vb <= F(0)) & (d2 >= F(0)) & (d6 <= F(0)) & (den_ac > F(0)),                   # edge v0 v2
                 (va <= F(0)) & (e43 >= F(0)) & (e56 >= F(0)) & (den_bc > F(0))]                 # edge v1 v2
        us = [F(0), F(1), d1 / den_ab, F(0), F(0), F(1) - w_bc]
        vs = [F(0), F(0), F(0), F(1), d2 / den_ac, w_bc]
        u = np.select(conds, [np.broadcast_to(F(x), fu.shape) if np.ndim(x) == 0 else x for x in us], fu).astype(F)
        v = np.select(conds, [np.broadcast_to(F(x), fv.shape) if np.ndim(x) == 0 else x for x in vs], fv).astype(F)
        c = (v0 + u[..., None] * e1) + v[..., None] * e2
        dp = p - c
        d2_ = dot3(dp, dp)
    return u, v, d2_


def point_valid(p, rmax):
    """the queries' points that can find a triangle: finite, rmax >= 0 (NaN and negative radii miss; -0 is 0)"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(p).all(axis=1) & (rmax >= F(0))


def _chunks(n, per, budget):
    step = max(1, budget // max(per, 1))
    for a in range(0, n, step):
        yield a, min(n, a + step)


def query(tris, cand, points, rmax=np.inf):
    """psm_bvh_closest_point_dev and psm_bvh_within_dev over the candidate triangle ids `cand` (the hierarchy's leaves,
    PSM_BVH_LEAF_TRI): a candidate counts iff sqrt(d2) <= rmax; closest = the smallest d2, on bit-equal d2 the lowest id.
    Returns (hits [R, 4] float32 as the kernel writes psm_hit -- u, v, dist, tri bits; a miss is 0, 0, +inf, -1 --, within [R])."""
    p = np.asarray(points, F).reshape(-1, 3)
    R = p.shape[0]
    rm = np.broadcast_to(np.asarray(rmax, F), (R,)).astype(F)
    cand = np.sort(np.asarray(cand, np.int64).reshape(-1))
    v0, e1, e2 = _split(np.asarray(tris, F).reshape(-1, 3, 3)[cand])
    hits = np.zeros((R, 4), F)
    hits[:, 2] = np.inf
    hits.view(np.int32)[:, 3] = -1
    within = np.zeros(R, bool)
    valid = point_valid(p, rm)
    if cand.size == 0:
        return hits, within

    def chunk(ab):
        a, b = ab
        u, v, d2 = closest_on_tris(v0[None], e1[None], e2[None], p[a:b, None, :])
        with np.errstate(invalid="ignore"):
            dist = np.sqrt(d2)
            ok = valid[a:b, None] & (dist <= rm[a:b, None])
        found = ok.any(axis=1)
        best = np.where(ok, d2, F(np.inf)).min(axis=1)
        k = np.argmax(ok & (d2 == best[:, None]), axis=1)   # the lowest id of the smallest d2 (candidates sorted by id)
        r = np.arange(b - a)
        hits[a:b, 0] = np.where(found, u[r, k], F(0))
        hits[a:b, 1] = np.where(found, v[r, k], F(0))
        hits[a:b, 2] = np.where(found, dist[r, k], F(np.inf))
        hits.view(np.int32)[a:b, 3] = np.where(found, cand[k], -1)
        within[a:b] = found

    with ThreadPoolExecutor(max_workers=8) as pool:   # (numpy releases the GIL: point chunks on a few threads)
        list(pool.map(chunk, _chunks(R, cand.size, 1 << 19)))
    return hits, within


def point_of(tris, tri, u, v):
    """the kernel's point from a result: c = (v0 + u e1) + v e2 of triangle `tri`, in float32"""
    v0, e1, e2 = _split(np.asarray(tris, F).reshape(-1, 3, 3)[np.asarray(tri)])
    u = np.asarray(u, F)[..., None]
    v = np.asarray(v, F)[..., None]
    return (v0 + u * e1) + v * e2


def closest_f64(tris, p):
    """A second reading in float64, by a different method: the minimum of the face distance (where p's projection onto the
    plane falls inside, by a 2 x 2 solve) and the three segment distances (clamped projections). tris [T, 3, 3], p [R, 3];
    returns the distance [R, T]."""
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    p = np.asarray(p, np.float64).reshape(-1, 3)[:, None, :]
    a, b, c = t[None, :, 0], t[None, :, 1], t[None, :, 2]

    def seg(x, y):
        d = y - x
        dd = np.sum(d * d, -1)
        with np.errstate(all="ignore"):
            s = np.where(dd > 0, np.sum((p - x) * d, -1) / dd, 0.0)
        s = np.clip(s, 0.0, 1.0)
        q = x + s[..., None] * d
        return np.sqrt(np.sum((p - q) ** 2, -1))

    best = np.minimum(np.minimum(seg(a, b), seg(a, c)), seg(b, c))
    e1, e2, ap = b - a, c - a, p - a
    g11, g12, g22 = np.sum(e1 * e1, -1), np.sum(e1 * e2, -1), np.sum(e2 * e2, -1)
    r1, r2 = np.sum(e1 * ap, -1), np.sum(e2 * ap, -1)
    det = g11 * g22 - g12 * g12
    with np.errstate(all="ignore"):
        s = (g22 * r1 - g12 * r2) / det
        w = (g11 * r2 - g12 * r1) / det
        inside = (det > 0) & (s >= 0) & (w >= 0) & (s + w <= 1)
        q = a + s[..., None] * e1 + w[..., None] * e2
        face = np.sqrt(np.sum((p - q) ** 2, -1))
    return np.where(inside, np.minimum(best, face), best)
