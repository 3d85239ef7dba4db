"""The sphere sweep (psm_bvh_sweep_sphere_dev / psm_bvh_sweep_occluded_dev, include/psm_hip.h "sweep queries"; sweep.hip,
psm_sweep_dev.h) restated in numpy: the canonical statement of sweep_tri.

sweep_tri is written once over a float type T. With T = float32 every operation is one float32 numpy operation in the order
psm_sweep_dev.h writes it (the library builds with -ffp-contract=off, so each operation rounds once, as numpy's do; division and
sqrt are correctly rounded on both sides), selections are np.where on the comparisons the kernel makes: the kernel's t, u, v
come out bit for bit. With T = float64 it is the second reading. first_contact_by_definition is a third that shares no formula
with it: the smallest t with dist(c(t), triangle) <= r, by a convex line search and a bisection over a float64 point-triangle
distance. The brute force over the leaves is the yardstick of tests/test_sweep_query_cpu.py and tests/test_gpu_sweep_query.py."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import point_query_model as PQ
from query_model import cross3, dot3, normalize3

F = np.float32
D = np.float64


def _clamp01(x, T):
    x = np.where(x > T(0), x, T(0))
    return np.where(x < T(1), x, T(1))


def closest_on_tris(v0, e1, e2, p, T=F):
    """closest_on_tri over the float type T: u, v, d2. float32 is point_query_model's (the point queries' yardstick, bit for bit the
    kernel's); any other type is the same regions, guards and operation order in that type."""
    if T is F:
        return PQ.closest_on_tris(v0, e1, e2, p)
    with np.errstate(all="ignore"):
        ap = p - v0
        aa, ab, bb = dot3(e1, e1), dot3(e1, e2), dot3(e2, e2)
        d1, d2 = dot3(e1, ap), dot3(e2, ap)
        d3, d4, d5, d6 = d1 - aa, d2 - ab, d1 - ab, d2 - bb
        vc, vb, va = aa * d2 - ab * d1, bb * d1 - ab * d2, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        det = aa * bb - ab * ab
        fu = _clamp01(vb / det, T)
        fv = vc / det
        fv = np.where(fv > T(0), fv, T(0))
        fv = np.where(fv < T(1) - fu, fv, T(1) - fu)
        e21 = e2 - e1
        cc = dot3(e21, e21)
        ta, tb, tc = _clamp01(d1 / aa, T), _clamp01(d2 / bb, T), _clamp01(e43 / cc, T)
        a_long = (aa >= bb) & (aa >= cc)
        b_long = ~a_long & (bb >= cc)
        su = np.where(a_long, ta, np.where(b_long, T(0), T(1) - tc))
        sv = np.where(a_long, T(0), np.where(b_long, tb, tc))
        face = det > aa * bb * T(2.0 ** -16)
        fu, fv = np.where(face, fu, su), np.where(face, fv, sv)
        w_bc = e43 / (e43 + e56)
        zero, one = np.zeros_like(fu), np.ones_like(fu)
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0) & (d1 - d3 > 0),
                 (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0) & (d2 - d6 > 0),
                 (va <= 0) & (e43 >= 0) & (e56 >= 0) & (e43 + e56 > 0)]
        u = np.select(conds, [zero, one, d1 / (d1 - d3), zero, zero, T(1) - w_bc], fu)
        v = np.select(conds, [zero, zero, zero, one, d2 / (d2 - d6), w_bc], fv)
        dp = p - ((v0 + u[..., None] * e1) + v[..., None] * e2)
        return u, v, dot3(dp, dp)


def _started(t):
    """t > 0 ? t : 0 -- a feature the sphere moves towards and already reaches at the start is a contact at the start"""
    return np.where(t > 0, t, np.zeros_like(t))


def _approach(m, dp, a, rr):
    """psm_sweep_dev.h approach: the entry time by closest approach, and whether it is one"""
    t0 = -dot3(m, dp) / a
    l = m + t0[..., None] * dp
    qq = rr - dot3(l, l)
    ok = (a > 0) & (t0 > 0) & (qq >= 0)
    return _started(t0 - np.sqrt(qq / a)), ok


def _edge(q, e, o, d, rr):
    ee = dot3(e, e)
    m = o - q
    sm, sn = dot3(m, e) / ee, dot3(d, e) / ee
    mp, dp = m - sm[..., None] * e, d - sn[..., None] * e
    t, ok = _approach(mp, dp, dot3(dp, dp), rr)
    s = sm + t * sn
    return t, s, ok & (ee > 0) & (s >= 0) & (s <= 1)


FEATURES = ("face", "v0", "v1", "v2", "edge v0 v1", "edge v0 v2", "edge v1 v2")   # the order ties are broken in


def sweep_tri(v0, e1, e2, o, d, r, tmax=np.inf, T=F, feature=False):
    """The first contact of the sphere (o + t d, r) with triangle (v0, e1, e2), arrays [..., 3] and [...] that broadcast: t, u, v
    (t = +inf, u = v = 0: no contact within tmax). d is the unit direction (normalize3 is the caller's, as in the kernel).
    feature=True adds which feature decided: -1 the start (t = 0), 0 .. 6 as FEATURES, 7 none."""
    v0, e1, e2, o, d = (np.asarray(x, T) for x in (v0, e1, e2, o, d))
    r, tmax = np.asarray(r, T), np.asarray(tmax, T)
    shape = np.broadcast_shapes(v0.shape[:-1], o.shape[:-1], d.shape[:-1], r.shape, tmax.shape)
    v0, e1, e2, o, d = (np.broadcast_to(x, shape + (3,)) for x in (v0, e1, e2, o, d))
    r, tmax = np.broadcast_to(r, shape), np.broadcast_to(tmax, shape)
    with np.errstate(all="ignore"):
        cu, cv, d2 = closest_on_tris(v0, e1, e2, o, T)
        start = np.sqrt(d2) <= r
        rr, dd = r * r, dot3(d, d)
        aa, ab, bb = dot3(e1, e1), dot3(e1, e2), dot3(e2, e2)
        det = aa * bb - ab * ab
        w0 = o - v0
        n = cross3(e1, e2)
        s0, sd, rn = dot3(n, w0), dot3(n, d), r * np.sqrt(dot3(n, n))
        t = _started((np.where(s0 > 0, rn, -rn) - s0) / sd)
        w = w0 + t[..., None] * d
        p1, p2 = dot3(w, e1), dot3(w, e2)
        u, v = (bb * p1 - ab * p2) / det, (aa * p2 - ab * p1) / det
        ok = (det > (aa * bb) * T(2.0 ** -16)) & (s0 * sd < 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
        zero, one = np.zeros(shape, T), np.ones(shape, T)
        q1, q2 = v0 + e1, v0 + e2
        cands = [(t, u, v, ok)]
        for q, uu, vv in ((None, zero, zero), (q1, one, zero), (q2, zero, one)):
            t, ok = _approach(w0 if q is None else o - q, d, dd, rr)
            cands.append((t, uu, vv, ok))
        t, s, ok = _edge(v0, e1, o, d, rr)
        cands.append((t, s, zero, ok))
        t, s, ok = _edge(v0, e2, o, d, rr)
        cands.append((t, zero, s, ok))
        t, s, ok = _edge(q1, e2 - e1, o, d, rr)
        cands.append((t, one - s, s, ok))
        bt, bu, bv, bf = np.full(shape, np.inf, T), zero, zero, np.full(shape, 7)
        for k, (t, u, v, ok) in enumerate(cands):
            take = ok & (t < bt)
            bt, bu, bv, bf = np.where(take, t, bt), np.where(take, u, bu), np.where(take, v, bv), np.where(take, k, bf)
        bt, bu, bv, bf = np.where(start, T(0), bt), np.where(start, cu, bu), np.where(start, cv, bv), np.where(start, -1, bf)
        miss = ~(bt <= tmax)
        out = np.where(miss, T(np.inf), bt).astype(T), np.where(miss, T(0), bu).astype(T), np.where(miss, T(0), bv).astype(T)
    return out + (np.where(miss, 7, bf),) if feature else out


def sweep_axis(M, o, d, r):
    """psm_sweep_dev.h sweep_axis for every row of the fit transform M [3, 4] (float32) and every sweep (o, d [n, 3], r [n]):
    inv, nlo, nhi [n, 3] in the kernel's float32 operation order"""
    M, o, d, r = (np.asarray(x, F) for x in (M, o, d, r))
    m = M[:, :3]
    with np.errstate(all="ignore"):
        P = ((m[:, 0] * o[:, None, 0] + m[:, 1] * o[:, None, 1]) + m[:, 2] * o[:, None, 2]) + M[:, 3]
        S = ((np.abs(m[:, 0] * o[:, None, 0]) + np.abs(m[:, 1] * o[:, None, 1])) + np.abs(m[:, 2] * o[:, None, 2])) + np.abs(M[:, 3])
        h = (F(2) + S) * F(2.0 ** -16)
        W = (np.abs(m[:, 0]) + np.abs(m[:, 1])) + np.abs(m[:, 2])
        H = h * F(33) + (W * r[:, None]) * F(1.00048828125)
        Dk = (m[:, 0] * d[:, None, 0] + m[:, 1] * d[:, None, 1]) + m[:, 2] * d[:, None, 2]
        Dk = np.where(np.abs(Dk) >= F(1e-20), Dk, np.copysign(F(1e-20), Dk))
        inv = F(1) / Dk
        nlo, nhi = -(P + H) * inv, (H - P) * inv
    assert nlo.dtype == F and nhi.dtype == F and inv.dtype == F
    return inv, nlo, nhi


def sweep_valid(o, d, r, tmax):
    """the sweeps that can touch at all: finite origin and normalised direction (a zero direction is not), 0 <= r < inf, tmax >= 0"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (r >= F(0)) & (r < F(np.inf)) & (tmax >= F(0))


def query(tris, cand, origins, directs, radius, tmax=np.inf):
    """psm_bvh_sweep_sphere_dev and psm_bvh_sweep_occluded_dev over the candidate triangle ids `cand` (the hierarchy's leaves,
    PSM_BVH_LEAF_TRI): the smallest t over the candidates, on a bit-equal t the lowest id. Returns (hits [R, 4] float32 as the
    kernel writes psm_hit -- u, v, t, tri bits; a miss is 0, 0, +inf, -1 --, occluded [R] bool)."""
    o = np.asarray(origins, F).reshape(-1, 3)
    R = o.shape[0]
    d = normalize3(np.asarray(directs, F).reshape(-1, 3))
    r = np.broadcast_to(np.asarray(radius, F), (R,)).astype(F)
    tm = np.broadcast_to(np.asarray(tmax, F), (R,)).astype(F)
    cand = np.sort(np.asarray(cand, np.int64).reshape(-1))
    v0, e1, e2 = PQ._split(np.asarray(tris, F).reshape(-1, 3, 3)[cand])
    hits = np.zeros((R, 4), F)
    hits[:, 2] = np.inf
    hits.view(np.int32)[:, 3] = -1
    found = np.zeros(R, bool)
    valid = sweep_valid(o, d, r, tm)
    if cand.size == 0:
        return hits, found

    def chunk(ab):
        a, b = ab
        t, u, v = sweep_tri(v0[None], e1[None], e2[None], o[a:b, None, :], d[a:b, None, :], r[a:b, None], tm[a:b, None])
        t = np.where(valid[a:b, None], t, F(np.inf))
        k = np.argmin(t, axis=1)            # the first of the smallest t: the lowest id (candidates sorted by id)
        i = np.arange(b - a)
        hit = np.isfinite(t[i, k])
        hits[a:b, 0] = np.where(hit, u[i, k], F(0))
        hits[a:b, 1] = np.where(hit, v[i, k], F(0))
        hits[a:b, 2] = np.where(hit, t[i, k], F(np.inf))
        hits.view(np.int32)[a:b, 3] = np.where(hit, cand[k], -1)
        found[a:b] = hit

    with ThreadPoolExecutor(max_workers=8) as pool:   # (numpy releases the GIL: sweep chunks on a few threads)
        list(pool.map(chunk, PQ._chunks(R, cand.size, 1 << 17)))
    return hits, found


# ---- the definitional reading -------------------------------------------------------------------------------------------------

def distance_f64(v0, e1, e2, p):
    """the distance of p to the triangle, pair by pair, in float64, by a method of its own: the smallest of the three segment
    distances (clamped projections) and, where p projects inside, the plane distance (a 2 x 2 solve)"""
    a, p = np.asarray(v0, D), np.asarray(p, D)
    b, c = a + np.asarray(e1, D), a + np.asarray(e2, D)

    def seg(x, y):
        e = y - x
        ee = np.sum(e * e, -1)
        with np.errstate(all="ignore"):
            s = np.where(ee > 0, np.sum((p - x) * e, -1) / ee, 0.0)
        q = x + np.clip(s, 0.0, 1.0)[..., None] * e
        return np.sqrt(np.sum((p - q) ** 2, -1))

    with np.errstate(all="ignore"):
        best = np.minimum(np.minimum(seg(a, b), seg(a, c)), seg(b, c))
        f1, f2, ap = b - a, c - a, p - a
        g11, g12, g22 = np.sum(f1 * f1, -1), np.sum(f1 * f2, -1), np.sum(f2 * f2, -1)
        r1, r2 = np.sum(f1 * ap, -1), np.sum(f2 * ap, -1)
        det = g11 * g22 - g12 * g12
        s, w = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
        inside = (det > 0) & (s >= 0) & (w >= 0) & (s + w <= 1)
        q = a + s[..., None] * f1 + w[..., None] * f2
        face = np.sqrt(np.sum((p - q) ** 2, -1))
    return np.where(inside, np.minimum(best, face), best)


def first_contact_by_definition(v0, e1, e2, o, d, r, length):
    """The smallest t in [0, length] with dist(o + t d, triangle) <= r, pair by pair in float64: the distance to a convex set
    along a line is convex, so a golden-section search finds its minimum and a bisection the first crossing before it. Returns
    (t, fmin): t = +inf where the minimum of dist - r stays above 0, fmin that minimum (how far the pair is from grazing)."""
    v0, e1, e2, o, d = (np.asarray(x, D) for x in (v0, e1, e2, o, d))
    r, length = np.asarray(r, D), np.asarray(length, D)

    def f(t):
        return distance_f64(v0, e1, e2, o + t[..., None] * d) - r

    g = (np.sqrt(5.0) - 1.0) / 2.0
    a, b = np.zeros(np.broadcast(r, length, o[..., 0]).shape), np.broadcast_to(length, np.broadcast(r, length, o[..., 0]).shape).copy()
    for _ in range(90):
        c1, c2 = b - g * (b - a), a + g * (b - a)
        left = f(c1) < f(c2)
        a, b = np.where(left, a, c1), np.where(left, c2, b)
    tm = 0.5 * (a + b)
    ends = np.minimum(f(np.zeros_like(tm)), f(np.broadcast_to(length, tm.shape)))
    fmin = np.minimum(f(tm), ends)
    tm = np.where(f(np.broadcast_to(length, tm.shape)) <= f(tm), np.broadcast_to(length, tm.shape), tm)
    f0 = f(np.zeros_like(tm))
    lo, hi = np.zeros_like(tm), tm.copy()
    for _ in range(70):
        mid = 0.5 * (lo + hi)
        inside = f(mid) <= 0
        lo, hi = np.where(inside, lo, mid), np.where(inside, mid, hi)
    t = np.where(f0 <= 0, 0.0, np.where(fmin <= 0, hi, np.inf))
    return t, fmin
