"""CPU tests (no GPU) of the clearance queries (psm_bvh_tri_closest_dev / psm_bvh_tri_within_dev, tri_dist.hip;
TriangleHierarchy.triClosest / triWithin): the float32 model (tests/tri_dist_query_model.py) on exact lattice
cases, against a float64 reading by a different method (least squares over the 7 x 7 pairs of faces), against tri_tri, on
degenerate triangles, ties and rmax; the prune's bound against every pair's d2 and a pruned walk over a real tree;
psm_tri_dist_dev.h itself on the host under the sanitizers; the exports and the refusals; what tri_dist.hip compiles to; and the
header layer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import point_query_model as PQ
import tri_dist_query_model as TD
import tri_query_model as TQ
from point_query_model import _split
from test_tri_query_cpu import _exact_meet, _fit_like, _lattice, _touching_queries
from util import ROOT, csrc_asm, kernel_asm, kernel_meta

F = np.float32
D = np.float64
EPS = 2.0 ** -24
# The model against the float64 reading on well-shaped triangles (smallest sine >= 0.2), relative to L, the largest coordinate
# difference among the pair's six vertices: the largest error measured over the soups below (three decades of size and of gap,
# an eighth of the pairs in contact, at the origin and moved by +1000) is 3.24e-7 L = 2^-21.6 L -- a pair in contact that
# tri_tri's float32 axes call met; away from contact the largest is 1.2e-7 L. Asserted at that rounded up to the next power of
# two, times 4 (a different seed moves a maximum of rounding errors by about that much): 2^-19 L.
TOL = 2.0 ** -21 * 4


def _model(tris, q, detail=False):
    """pair i = (stored triangle i, query triangle i), float32"""
    v0, e1, e2 = _split(tris)
    q = np.asarray(q, F).reshape(-1, 3, 3)
    return TD.tri_dist(v0, e1, e2, q[:, 0], q[:, 1], q[:, 2], detail=detail)


def _stored64(tris):
    """the stored triangle as the kernel reads it, in float64: v0, v0 + fl(v1 - v0), v0 + fl(v2 - v0)"""
    v0, e1, e2 = (x.astype(D) for x in _split(tris))
    return np.stack([v0, v0 + e1, v0 + e2], axis=1)


def _span(t, q):
    """L: the largest coordinate difference among the pair's six vertices"""
    p = np.concatenate([np.asarray(t, D), np.asarray(q, D)], axis=1)
    return (p.max(axis=1) - p.min(axis=1)).max(axis=1)


# the seven faces of a triangle: (first vertex, the vertices its affine hull's directions reach to)
FACES = ((0, ()), (1, ()), (2, ()), (0, (1,)), (0, (2,)), (1, (2,)), (0, (1, 2)))


def _feasible(x):
    """weights x [..., k] of a face's directions: inside the face (k = 1: the segment, k = 2: the triangle), to 1e-9"""
    return (x >= -1e-9).all(axis=-1) & (x.sum(axis=-1) <= 1 + 1e-9)


def _f64_reading(t, q, lstsq=False, meets=True):
    """The distance of triangle pairs t, q [n, 3, 3] in float64 by a different method: over the 7 x 7 pairs of faces (vertex,
    edge, face of each), the unconstrained least squares between the two affine hulls; the feasible solutions are kept and the
    minimum taken. lstsq: numpy.linalg.lstsq pair by pair; else the same minimum-norm solution batched (numpy.linalg.pinv).
    meets: 0 where an exact-style meet test in float64 says the pair meets (non-degenerate pairs only)."""
    t, q = np.asarray(t, D), np.asarray(q, D)
    n = t.shape[0]
    best = np.full(n, np.inf)
    for ft, dt in FACES:
        for fq, dq in FACES:
            r = q[:, fq] - t[:, ft]                                               # minimise |Dt x - Dq y - r|
            cols = [t[:, k] - t[:, ft] for k in dt] + [-(q[:, k] - q[:, fq]) for k in dq]
            if not cols:
                best = np.minimum(best, np.linalg.norm(r, axis=1))
                continue
            A = np.stack(cols, axis=2)                                            # [n, 3, k]
            if lstsq:
                x = np.stack([np.linalg.lstsq(A[i], r[i], rcond=None)[0] for i in range(n)])
            else:
                x = np.einsum("nkj,nj->nk", np.linalg.pinv(A), r)
            ok = _feasible(x[:, :len(dt)]) & _feasible(x[:, len(dt):])
            res = np.linalg.norm(np.einsum("njk,nk->nj", A, x) - r, axis=1)
            best = np.where(ok, np.minimum(best, res), best)
    if meets:
        solid = (np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1) > 0) & \
                (np.linalg.norm(np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]), axis=1) > 0)
        i = np.nonzero(solid)[0]
        met = np.zeros(n, bool)
        met[i] = _exact_meet(t[i], q[i])
        best = np.where(met, 0.0, best)
    return best


# ---- exact cases on the 1/8 lattice -------------------------------------------------------------------------------------------------

ORDERS = ([0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1])


def _both_roles(t, q):
    """(stored, query) in four vertex orders of each and both roles"""
    t, q = np.asarray(t, F), np.asarray(q, F)
    for o in ORDERS:
        yield t[o], q
        yield t, q[o]
        yield q[o], t
        yield q, t[o]


def _dist(t, q, detail=False):
    out = _model(np.asarray(t, F)[None], np.asarray(q, F)[None], detail=detail)
    return (np.sqrt(out[0][0]),) + tuple(x[0] for x in out[1:])


def _three_vertex_standin(t, q):
    """what closestPoint on the query's three vertices gives: the stand-in the clearance queries replace"""
    v0, e1, e2 = _split(np.asarray(t, F)[None])
    return np.sqrt(min(PQ.closest_on_tris(v0, e1, e2, np.asarray(q, F)[k][None])[2][0] for k in range(3)))


def test_exact_cases_on_the_lattice():
    tri = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]])                    # in the plane z = 0
    for t, q in _both_roles(tri, tri + [0, 0, 0.25]):                        # parallel triangles 0.25 apart
        assert _dist(t, q)[0] == 0.25
    for t, q in _both_roles(tri, [[0.125, 0.125, 0.5], [0.125, 0.25, 1], [0.25, 0.125, 1]]):   # a vertex 0.5 above the interior
        d, u, v, s, w = _dist(t, q)
        assert d == 0.5
    # two edges crossing skew at height 0.125: the stored edge v0 v1 along x, the query's along y above its middle
    skew = [[0.25, -0.5, 0.125], [0.25, 0.5, 0.125], [0.25, 0, 1]]
    for t, q in _both_roles([[0, 0, 0], [0.5, 0, 0], [0.25, 0, -1]], skew):
        d = _dist(t, q, detail=True)
        assert d[0] == 0.125 and d[5] >= 6, d                                # an edge pair wins: no vertex is that near
    # a small triangle under the middle of a large one: the face case. The three vertices of the large one are far away
    big = np.array([[-4, -4, 0.25], [4, -4, 0.25], [0, 4, 0.25]])
    small = np.array([[0, 0, 0], [0.125, 0, 0], [0, 0.125, 0]])
    for t, q in _both_roles(small, big):
        assert _dist(t, q)[0] == 0.25
    assert _three_vertex_standin(small, big) > 3.8                           # ... which is what the stand-in gets wrong: |(0, 4, 0.25) - (0, 0.125, 0)|
    # coplanar and disjoint, the bounding boxes overlap: the hypotenuse x + y = 0.5 against the vertex (0.375, 0.5)
    away = np.array([[0.5, 0.5, 0], [0.375, 0.5, 0], [0.5, 0.375, 0]])
    for t, q in _both_roles(tri, away):
        assert abs(_dist(t, q)[0] - 0.375 / np.sqrt(2)) <= 1e-7
    for t, q in _both_roles(tri, tri + [0.625, 0, 0]):                       # ... and along an axis: exactly a step apart
        assert _dist(t, q)[0] == 0.125


def test_closedness_fixtures_and_a_piercing_edge_are_at_distance_zero():
    tri = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]])
    step = 0.125
    touching = (([[0, 0, 0], [-0.5, -0.25, 0.5], [-0.25, -0.5, 0.5]], [0, 0, step]),              # a shared vertex only
                ([[0, 0, 0], [0.5, 0, 0], [0.25, 0, 0.5]], [0, -step, 0]),                       # a shared edge
                ([[0, 0, 0], [0.5, 0, 0], [0.25, -0.5, 0]], [0, -step, 0]),                      # coplanar, edge to edge
                ([[0.125, 0.125, 0], [0.125, 0.25, 0.5], [0.25, 0.125, 0.5]], [0, 0, step]),     # a vertex in the interior
                ([[0.125, 0.125, 0], [0.25, 0.125, 0], [0.125, 0.25, 0]], [0, 0, step]),         # coplanar, one inside the other
                ([[0.5, 0, 0], [1, -0.5, 0], [1, 0.5, 0]], [step, 0, 0]))                        # coplanar, vertex to vertex
    for q, apart in touching:                                                # the triangle tests' closedness fixtures
        q = np.array(q)
        for t, qq in _both_roles(tri, q):
            assert _dist(t, qq)[0] == 0
        for t, qq in _both_roles(tri, q + apart):                            # one lattice step apart: exactly that
            assert _dist(t, qq)[0] == step
    # an edge piercing the interior: no feature of the boundaries touches, the fifteen stay positive, the pair is at 0
    pierce = np.array([[0.125, 0.125, -0.5], [0.125, 0.125, 0.5], [2, 2, 0.5]])
    for t, q in _both_roles(tri, pierce):
        d = _dist(t, q, detail=True)
        assert d[0] == 0 and d[6] >= 0.125 ** 2 / 2, d
        v0, e1, e2 = _split(np.asarray(t, F)[None])
        qq = np.asarray(q, F)
        assert TQ.tri_tri(v0, e1, e2, qq[None, 0], qq[None, 1], qq[None, 2])[0]


# ---- against the float64 reading ---------------------------------------------------------------------------------------------------------

def _well_shaped(rng, n):
    """triangles whose three angles all have a sine >= 0.2 by construction (two angles in [0.25, 1.4], the third what is left:
    in [0.34, 2.65]), of edge length 10^-3 .. 1, randomly oriented, around the origin"""
    al, be = rng.uniform(0.25, 1.4, n), rng.uniform(0.25, 1.4, n)
    c = 10.0 ** rng.uniform(-3, 0, n)
    b = c * np.sin(be) / np.sin(np.pi - al - be)
    loc = np.zeros((n, 3, 3))
    loc[:, 1, 0] = c
    loc[:, 2, 0], loc[:, 2, 1] = b * np.cos(al), b * np.sin(al)
    rot = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    t = np.einsum("nvj,nkj->nvk", loc, rot)
    t -= t.mean(axis=1, keepdims=True)
    return np.take_along_axis(t, np.argsort(rng.uniform(size=(n, 3)), axis=1)[:, :, None], axis=1), c


def _soup(seed, n):
    """pairs of well-shaped triangles over three decades of size and of gap"""
    rng = np.random.RandomState(seed)
    t, ct = _well_shaped(rng, n)
    q, cq = _well_shaped(rng, n)
    way = rng.normal(size=(n, 1, 3))
    way /= np.linalg.norm(way, axis=2, keepdims=True)
    # a point of the query goes to a random point of the stored triangle, then off it by the gap, 10^-3 .. 2 of the larger
    # size (an eighth of the pairs stay in contact). Half of the pairs: a random point of the query, along a random direction
    # (many of them cross); the other half: the query's lowest vertex along the stored normal (the distance is the gap)
    gap = 10.0 ** rng.uniform(-3, 0.3, (n, 1, 1)) * rng.choice([0.0] + [1.0] * 7, (n, 1, 1)) * np.maximum(ct, cq)[:, None, None]
    on_t = np.einsum("nv,nvk->nk", rng.dirichlet([1, 1, 1], n), t)
    on_q = np.einsum("nv,nvk->nk", rng.dirichlet([1, 1, 1], n), q)
    up = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    up /= np.linalg.norm(up, axis=1, keepdims=True)
    low = np.take_along_axis(q, np.argmin(np.einsum("nvk,nk->nv", q, up), axis=1)[:, None, None], axis=1)[:, 0]
    half = (np.arange(n) % 2 == 0)[:, None]
    on_q, way = np.where(half, on_q, low), np.where(half[:, :, None], way, up[:, None, :])
    q = q + (on_t - on_q)[:, None, :] + way * gap
    where = rng.uniform(-1, 1, (n, 1, 3))
    return t + where, q + where


def _sines(t):
    t = np.asarray(t, D)
    out = []
    for k in range(3):
        a, b = t[:, (k + 1) % 3] - t[:, k], t[:, (k + 2) % 3] - t[:, k]
        out.append(np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)))
    return np.min(out, axis=0)


@pytest.mark.parametrize("shift", [0.0, 1000.0], ids=["soup", "soup_moved_by_1000"])
def test_model_against_the_float64_reading_on_well_shaped_triangles(shift):
    t, q = _soup(11, 1500)
    t, q = ((x.astype(F) + F(shift)).astype(F) for x in (t, q))
    t64 = _stored64(t)
    assert min(_sines(t64).min(), _sines(q).min()) >= 0.2                    # none need leaving out
    ref = _f64_reading(t64, q, lstsq=True)
    fast = _f64_reading(t64, q)                                              # the batched form the larger sets below use
    L = _span(t64, q)
    assert (np.abs(ref - fast) <= 1e-12 * L).all()
    d2 = _model(t, q)[0]
    err = np.abs(np.sqrt(d2.astype(D)) - ref) / L
    print("pairs %d, at distance 0: %d, gaps %.2g .. %.2g of L, the largest error %.3g L = 2^%.1f L (asserted: 2^%.0f L)"
          % (err.size, (ref == 0).sum(), (ref / L)[ref > 0].min(), (ref / L).max(), err.max(), np.log2(err.max()), np.log2(TOL)))
    assert err.max() <= TOL
    assert (ref == 0).sum() > 50 and ((ref > 0) & (ref < 1e-2 * L)).sum() > 50 and (ref > 0.1 * L).sum() > 50
    assert (d2[ref > TOL * L] > 0).all() and (d2[ref == 0] <= (TOL * L[ref == 0]) ** 2).all()


def test_slivers_and_collinear_triangles_keep_the_per_triangle_bound():
    """a sliver on either side: the error is within TOL L plus closest_on_tri's per-triangle bound of DESIGN.md 4.6 -- 8 eps / s^2
    of its longest edge while it has a face (s the sine of its smallest angle), its width s L once it is taken as its longest
    edge -- for each of the two triangles"""
    rng = np.random.RandomState(12)
    n = 1200
    ang = np.repeat(np.geomspace(1e-6, 0.2, 40), n // 40) * rng.uniform(0.8, 1.2, n)
    l1, l2 = rng.uniform(0.3, 1.5, n), rng.uniform(0.3, 1.5, n)
    loc = np.zeros((n, 3, 3))
    loc[:, 1, 0] = l1
    cap = rng.rand(n) < 0.3
    loc[:, 2, 0] = np.where(cap, -l2 * np.cos(ang), l2 * np.cos(ang))
    loc[:, 2, 1] = l2 * np.sin(ang)
    loc[::7, 2, 1] = 0                                                       # exactly collinear in the local frame
    rot = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    sliver = np.einsum("nvj,nkj->nvk", loc, rot)
    sliver = np.take_along_axis(sliver, np.argsort(rng.uniform(size=(n, 3)), axis=1)[:, :, None], axis=1)
    other, _ = _well_shaped(rng, n)
    other = other * 300 * rng.uniform(0.3, 1, (n, 1, 1)) + rng.normal(size=(n, 1, 3)) * 0.5
    for t, q in ((sliver, other), (other, sliver)):
        t, q = t.astype(F), q.astype(F)
        t64 = _stored64(t)
        ref = _f64_reading(t64, q, meets=False)
        d2 = _model(t, q)[0]
        assert np.isfinite(d2).all()
        tol = TOL * _span(t64, q)
        for x in (t64, q.astype(D)):
            s = _sines(x)
            edge = np.linalg.norm(x - np.roll(x, 1, axis=1), axis=2).max(axis=1)
            with np.errstate(divide="ignore"):
                tol = tol + np.minimum(8 * EPS / np.maximum(s, 1e-30) ** 2, np.maximum(s, 2.0 ** -8)) * edge
        far = np.sqrt(d2.astype(D)) - ref                                    # tri_tri's rounding may call a near-touching pair met
        assert (far <= tol).all(), (far - tol).max()
        assert (-far <= tol + (d2 == 0) * 1e-3 * _span(t64, q)).all()


def test_distance_is_zero_exactly_where_tri_tri_holds_on_the_lattice():
    """100 000 lattice pairs: all arithmetic of tri_tri is exact, so dist == 0 iff the pair meets; a disjoint pair is at a
    positive distance within the tolerance of the float64 reading. On the 1/8 lattice of [-1, 1]^3 (integers to +-8, edges to 16
    a component) the squared distance of a disjoint pair is, in lattice units, (r . n)^2 / |n|^2 with integer r and n a cross
    product of two lattice edges (vertex to face, edge to edge), or |r x d|^2 / |d|^2 (vertex to edge, to vertex): a positive
    integer over at most (3 x 16^2)^2. So d2 >= 1 / (64 x 768^2) = 2.6e-8 in squared length units, a distance of 1.6e-4, while
    the computed Q - P is within a few eps L = 1e-6 of the real one: 0 cannot be reached by rounding. (Observed: 2.2e-7.)"""
    ti, qi = _lattice(21, 100000)
    tris, q = (ti / 8.0).astype(F), (qi / 8.0).astype(F)
    v0, e1, e2 = _split(tris)
    meet = TQ.tri_tri(v0, e1, e2, q[:, 0], q[:, 1], q[:, 2])
    d2, u, v, s, t, k, low = _model(tris, q, detail=True)
    assert np.array_equal(d2 == 0, meet)
    assert 0.05 < meet.mean() < 0.8
    apart = ~meet
    assert d2[apart].min() >= 2.5e-8
    pierced = meet & (low > 0)
    print("pairs %d, meet %d, of them with all fifteen features positive %d, the smallest positive d2 %.3g"
          % (meet.size, meet.sum(), pierced.sum(), d2[apart].min()))
    assert pierced.sum() > 100
    ref = _f64_reading(_stored64(tris), q, meets=False)
    L = _span(tris, q)
    nt, nq = np.cross(ti[:, 1] - ti[:, 0], ti[:, 2] - ti[:, 0]), np.cross(qi[:, 1] - qi[:, 0], qi[:, 2] - qi[:, 0])
    solid = nt.any(axis=1) & nq.any(axis=1)
    err = np.abs(np.sqrt(d2.astype(D)) - ref)
    assert (err[apart & solid] <= TOL * L[apart & solid]).all()
    assert (ref[meet & solid] <= 1e-12).all() and (ref[apart & solid] > 1e-4).all()   # the reading finds the piercings itself
    for w in (u, v, s, t):
        assert ((w >= 0) & (w <= 1)).all()
    assert (u + v <= 1).all() and (s + t <= 1).all()


def _solid(ti):
    return np.cross(ti[:, 1] - ti[:, 0], ti[:, 2] - ti[:, 0]).any(axis=1)


def test_degenerate_triangles_get_finite_records():
    """point and segment queries against triangles with an area; stored triangles with two equal vertices, collinear, zero-area
    against query triangles with an area: finite records, the float64 reading of the segment or point within the tolerance
    (lattice coordinates: no sliver in between); a point query's dist is closestPoint's model's within the tolerance and never
    above it by more. Pairs with NO area on either side are finite too, but inherit tri_tri's missing axes: the next test."""
    rng = np.random.RandomState(13)
    n = 20000
    a, b = rng.randint(-8, 9, (n, 3)), rng.randint(-3, 4, (n, 3))
    kk = rng.randint(-2, 3, (n, 2))
    solid = rng.randint(-6, 7, (n, 1, 3)) + rng.randint(-3, 4, (n, 3, 3))
    solid = solid[_solid(solid)]
    n = solid.shape[0]
    a, b, kk = a[:n], b[:n], kk[:n]
    assert n > 19000
    segment, point = np.stack([a, a, a + b], axis=1), np.stack([a, a, a], axis=1)
    two_equal, collinear = np.stack([a, a + b, a + b], axis=1), np.stack([a, a + kk[:, :1] * b, a + kk[:, 1:] * b], axis=1)
    for ti, qi in ((solid, segment), (solid, segment[:, [2, 0, 1]]), (solid, point), (two_equal, solid), (two_equal[:, [1, 0, 2]], solid),
                   (collinear, solid), (solid, collinear), (point, solid), (segment, segment[::-1]), (point, point[::-1]), (collinear, point[::-1])):
        tris, q = (ti / 8.0).astype(F), (qi / 8.0).astype(F)
        d2, u, v, s, t = _model(tris, q)
        for w in (d2, u, v, s, t):
            assert np.isfinite(w).all()
        for w in (u, v, s, t):
            assert ((w >= 0) & (w <= 1)).all()
        if not (_solid(ti) | _solid(qi)).all():                              # no area on either side: finite, and the next test
            continue
        ref = _f64_reading(_stored64(tris), q, meets=False)
        err = np.abs(np.sqrt(d2.astype(D)) - ref)
        assert (err <= TOL * np.maximum(_span(tris, q), 0.125)).all(), err.max()
        assert (d2 == 0).any() and (d2 > 0).any()
    tris, q = (solid / 8.0).astype(F), (point / 8.0).astype(F)               # a point query against closestPoint's model
    v0, e1, e2 = _split(tris)
    pd = np.sqrt(PQ.closest_on_tris(v0, e1, e2, q[:, 0])[2])
    d = np.sqrt(_model(tris, q)[0])
    L = np.maximum(_span(tris, q), 0.125)
    assert (np.abs(d - pd) <= TOL * L).all() and (d <= pd + TOL * L).all()


def test_no_area_on_either_side_inherits_tri_tri_s_missing_axes():
    """tri_tri's axes are complete for two triangles with an area. Where neither has one (a segment against a segment or a
    point) most of its axes are zero and separate nothing, so it may hold for a pair that is apart; and for a segment in the
    plane of a triangle the segment's own in-plane normal is not among the 20. Such a pair is at distance 0 BY DEFINITION
    (psm_hip.h: tri_tri holds) -- the side a clearance check errs on -- while the fifteen features' own minimum is the real
    distance. Stated here so that it is not met by surprise; the triangle queries answer 1 for the same pairs."""
    seg = np.array([[-8, 0, 3], [-8, 0, 3], [-3, 3, 8]]) / 8.0                # a segment whose box holds the point
    pt = np.array([[-6, 3, 3]] * 3) / 8.0
    d = _dist(seg, pt, detail=True)
    assert d[0] == 0 and abs(np.sqrt(d[6]) - _f64_reading(seg[None], pt[None], meets=False)[0]) <= TOL and d[6] > 0.1
    tri = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]]) / 8.0                  # a coplanar segment past the corner, 1 / sqrt(5) steps off
    flat = np.array([[-3, 1, 0], [-3, 1, 0], [1, -1, 0]]) / 8.0
    d = _dist(tri, flat, detail=True)
    assert d[0] == 0 and abs(np.sqrt(d[6]) - 0.125 / np.sqrt(5)) <= TOL
    v0, e1, e2 = _split(tri.astype(F)[None])
    assert TQ.tri_tri(v0, e1, e2, *(flat.astype(F)[None, k] for k in range(3)))[0]
    d = _dist(tri, flat + [0, 0, 0.125], detail=True)                        # out of the plane the edge axes decide: exact again
    assert abs(d[0] - np.sqrt(0.125 ** 2 / 5 + 0.125 ** 2)) <= TOL


def test_ties_go_to_the_lowest_id_and_the_first_feature():
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    q = (tri + F([0.125, 0.125, 0.5])).astype(F)
    tris = np.stack([tri + F([0, 0, 1]), tri, tri, tri + F([0, 0, 1])])      # duplicates; and two at 0.5 on either side
    hits, within = TD.query(tris, [3, 2, 1, 0], q[None])
    assert hits.view(np.int32)[0, 3] == 0 and hits[0, 2] == 0.5 and within[0]      # equidistant from 0 / 3 and 1 / 2: the lowest id
    hits, _ = TD.query(tris, [3, 2, 1], q[None])
    assert hits.view(np.int32)[0, 3] == 1                                    # duplicates: the lower of the two
    hits, _ = TD.query(tris, [3, 2], q[None])                                # candidates are the leaves
    assert hits.view(np.int32)[0, 3] == 2
    # parallel translated copies: vertex a over the face, vertex 0 under the query's face, and several edge pairs all give
    # d2 = 0.25 bit for bit: the first feature in the order keeps it
    d2, u, v, s, t, k, low = _model(tri[None], (tri + F([0.25, 0.25, 0.5]))[None].astype(F), detail=True)
    feats = TD.features(*_split(tri[None]), *((tri + F([0.25, 0.25, 0.5])).astype(F)[None, j] for j in range(3)))[0][:, 0]
    assert d2[0] == 0.25 and (feats == 0.25).sum() >= 2 and k[0] == np.nonzero(feats == 0.25)[0][0] == 0
    assert (s[0], t[0]) == (0, 0) and (u[0], v[0]) == (0.25, 0.25)
    # and a bit-equal d2 that the first feature does not have: the first of those that do
    d2, u, v, s, t, k, low = _model(tri[None], (tri + F([-0.25, -0.25, 0.5]))[None].astype(F), detail=True)
    feats = TD.features(*_split(tri[None]), *((tri + F([-0.25, -0.25, 0.5])).astype(F)[None, j] for j in range(3)))[0][:, 0]
    assert d2[0] == 0.25 and (feats == 0.25).sum() >= 2 and feats[0] > 0.25 and k[0] == np.nonzero(feats == 0.25)[0][0] > 0


def test_rmax_is_closed_and_invalid_queries_miss():
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], F)
    q = np.repeat((tri + F([0, 0, 0.75])), 9, axis=0)
    q[7, 0, 0], q[8, 2, 1] = np.nan, np.inf
    below = np.nextafter(F(0.75), F(0))
    rmax = np.array([np.inf, 0.75, below, 0, -0.0, -1, np.nan, np.inf, np.inf], F)
    hits, within = TD.query(tri, [0], q, rmax)
    assert list(hits.view(np.int32)[:, 3]) == [0, 0, -1, -1, -1, -1, -1, -1, -1]
    assert list(within) == [True, True] + [False] * 7
    assert hits[1, 2] == 0.75 and np.array_equal(hits[2].view(np.uint32), TD.miss_records(1)[0].view(np.uint32))
    touching = np.repeat(tri + F([1, 0, 0]), 3, axis=0)                      # a shared vertex: distance 0
    hits, within = TD.query(tri, [0], touching, F([0.0, -0.0, -1e-30]))
    assert list(within) == [True, True, False] and hits[1, 2] == 0           # -0 is 0
    rng = np.random.RandomState(14)                                          # within(q, r) == (closest(q, r).tri >= 0), whatever r
    tris = (rng.uniform(-1, 1, (60, 1, 3)) + rng.uniform(-0.2, 0.2, (60, 3, 3))).astype(F)
    qq = (rng.uniform(-1.5, 1.5, (400, 1, 3)) + rng.uniform(-0.3, 0.3, (400, 3, 3))).astype(F)
    free, _ = TD.query(tris, np.arange(60), qq)
    r = rng.choice(F([0.05, 0.2, 0.6, np.inf, np.nan, -1.0]), 400)
    r[:100] = free[:100, 2]                                                  # exactly the distance: counts
    r[100:200] = np.nextafter(free[100:200, 2], F(0))                        # a float below it: does not (unless it is 0)
    hits, within = TD.query(tris, np.arange(60), qq, r)
    assert np.array_equal(within, hits.view(np.int32)[:, 3] >= 0)
    assert within[:100].all() and np.array_equal(hits[:100].view(np.uint32), free[:100].view(np.uint32))
    assert np.array_equal(within[100:200], free[100:200, 2] == 0) and (free[100:200, 2] > 0).sum() > 50
    with np.errstate(invalid="ignore"):
        assert np.array_equal(within[200:], free[200:, 2] <= r[200:]) and within[200:].any() and not within[200:].all()


def test_the_record_reproduces_the_distance():
    """(tri, u, v, s, t) of a record give back the value the query reports, bit for bit, by tri_dist_d2"""
    rng = np.random.RandomState(15)
    tris = (rng.uniform(-1, 1, (64, 1, 3)) + rng.uniform(-0.3, 0.3, (64, 3, 3))).astype(F)
    q = (rng.uniform(-1.5, 1.5, (300, 1, 3)) + rng.uniform(-0.3, 0.3, (300, 3, 3))).astype(F)
    hits, within = TD.query(tris, np.arange(64), q)
    assert within.all()
    tri = hits.view(np.int32)[:, 3]
    v0, e1, e2 = _split(tris[tri])
    A, B, C = q[:, 0] - v0, q[:, 1] - v0, q[:, 2] - v0
    d2 = TD.d2_of(e1, e2, A, B - A, C - A, hits[:, 0], hits[:, 1], hits[:, 4], hits[:, 5])
    apart = hits[:, 2] > 0
    assert np.array_equal(np.sqrt(d2)[apart].view(np.uint32), hits[apart, 2].view(np.uint32)) and apart.sum() > 100
    pm, pq = TD.points_of(tris, q, hits)                                     # the two world points: the distance to rounding
    assert np.abs(np.linalg.norm(pm.astype(D) - pq, axis=1)[apart] - hits[apart, 2]).max() <= 1e-6


# ---- the prune (psm_query_dev.h point_bound) -----------------------------------------------------------------------

def _shear_like(rng, tris):
    """a fit-like transform whose 3 x 3 part is a shear (condition number up to 16): the max form of the bound"""
    A = np.eye(3)
    A[0, 1], A[1, 2], A[2, 0] = rng.uniform(0.3, 1.2), rng.uniform(-1.2, -0.3), rng.uniform(0.2, 0.8)
    y = tris.reshape(-1, 3).astype(D) @ A.T
    lo, ext = y.min(0), np.full(3, (y.max(0) - y.min(0)).max())
    M = np.zeros((3, 4))
    M[:, :3] = A / ext[:, None]
    M[:, 3] = -lo / ext
    return M.astype(F)


def test_prune_bound_is_below_every_pair_s_d2():
    """plain, rotating, rotate-and-scale and shearing transforms (condition numbers to 16) over six decades of magnitude: for
    every (query, triangle) pair LB^2, by the kernel's formula in float32 against the triangle's exact UNPADDED normalised box,
    is <= the pair's d2: a leaf is never dropped while its triangle could still win. The largest LB^2 / d2 observed: 0.99999."""
    rng = np.random.RandomState(16)
    worst, total, conds, forms = 0.0, 0, [], set()
    for mag in range(-3, 4):
        scale = 10.0 ** mag
        for kind in (0, 1, 2, 3):
            c = rng.uniform(-1, 1, (120, 1, 3))
            tris = ((c + rng.uniform(-0.2, 0.2, (120, 3, 3)) * rng.uniform(0.02, 1, (120, 1, 1))) * scale).astype(F)
            M = _fit_like(rng, tris, kind) if kind < 3 else _shear_like(rng, tris)
            conds.append(np.linalg.cond(M[:, :3].astype(D)))
            bound = TD.point_bound(M)
            forms.add(bound[2])
            qc = rng.uniform(-1.6, 1.6, (150, 1, 3))
            q = ((qc + rng.uniform(-1, 1, (150, 3, 3)) * 10.0 ** rng.uniform(-3, 0, (150, 1, 1))) * scale).astype(F)
            pairs = [(tris[None], q[:, None]), _touching_queries(rng, tris, scale, 6)]
            for t, qq in pairs:
                t, qq = np.broadcast_arrays(t, qq)
                shape = t.shape[:-2]
                t, qq = t.reshape(-1, 3, 3), qq.reshape(-1, 3, 3)
                d2 = _model(t, qq)[0]
                img = _stored64(t) @ M[:, :3].astype(D).T + M[:, 3].astype(D)       # the exact image of the stored triangle
                mn, mx = img.min(axis=1), img.max(axis=1)
                # the box a leaf can be at its smallest: float32 corners rounded inward never occur; take them to nearest
                gl, gh = TD.box_rows(M, qq)
                lb = TD.lb2(bound, gl, gh, mn.astype(F), mx.astype(F))
                with np.errstate(all="ignore"):
                    assert (lb <= d2).all(), (mag, kind, np.max(lb / d2))
                    ratio = np.where(d2 > 0, lb / np.where(d2 > 0, d2, 1), 0)
                worst = max(worst, float(ratio.max()))
                total += d2.size
                assert (lb[d2 == 0] == 0).all(), (mag, kind, shape)
    print("pairs %d; the largest LB^2 / d2: %.6f; condition numbers up to %.1f" % (total, worst, max(conds)))
    assert max(conds) > 12 and total > 400000 and forms == {True, False} and 0.9 < worst <= 1.0


@pytest.mark.parametrize("kind", [0, 2, 3], ids=["plain", "rotate_scale", "shear"])
def test_a_pruned_walk_over_a_real_tree_is_the_brute_force(kind):
    rng = np.random.RandomState(17 + kind)
    c = rng.uniform(-1, 1, (200, 1, 3))
    tris = (c + rng.uniform(-0.15, 0.15, (200, 3, 3))).astype(F)
    tris[50] = tris[20]                                                      # a duplicate: the lower id wins
    cand = np.delete(np.arange(200), [3, 77])
    M = _fit_like(rng, tris[cand], kind) if kind < 3 else _shear_like(rng, tris[cand])
    tree = TD.build_tree(M, tris, cand)
    q = (rng.uniform(-1.5, 1.5, (120, 1, 3)) + rng.uniform(-1, 1, (120, 3, 3)) * 10.0 ** rng.uniform(-2.5, 0, (120, 1, 1))).astype(F)
    q[:10] = tris[rng.choice(cand, 10)] + F([0, 0, 0.01])
    q[10:14] = tris[[20, 50, 20, 50]]
    q[14:20] = (rng.normal(size=(6, 1, 3)) * 50 + rng.uniform(-1, 1, (6, 3, 3))).astype(F)   # far outside
    rmax = rng.choice(F([np.inf, np.inf, 0.0, 0.05, 0.3]), 120)
    q[20, 0, 0], rmax[21], rmax[22] = np.nan, -1, np.nan
    want, want_in = TD.query(tris, cand, q, rmax)
    tested = 0
    for i in range(120):
        rec, n = TD.walk(M, tris, tree, q[i], rmax[i])
        flag, _ = TD.walk(M, tris, tree, q[i], rmax[i], within=True)
        assert np.array_equal(rec.view(np.uint32), want[i].view(np.uint32)), (i, rec, want[i])
        assert flag == want_in[i], i
        tested += n
    print("leaves tested per query: %.1f of %d" % (tested / 120.0, cand.size))
    assert tested < 0.5 * 120 * cand.size and want_in.sum() > 40 and (~want_in).sum() > 10


# ---- psm_tri_dist_dev.h itself, on the host --------------------------------------------------------------------------------------------

def _host_pairs():
    """(v0, e1, e2, a, b, c) of a few hundred thousand pairs: lattice, soup, moved soup, touching, degenerate, NaN and inf"""
    rng = np.random.RandomState(18)
    ti, qi = _lattice(19, 110000)
    sets = [((ti / 8.0).astype(F), (qi / 8.0).astype(F))]
    t, q = _soup(20, 60000)
    sets.append((t.astype(F), q.astype(F)))
    sets.append(((t.astype(F) + F(1000)).astype(F), (q.astype(F) + F(1000)).astype(F)))
    c = rng.uniform(-1, 1, (4000, 1, 3))
    base = (c + rng.uniform(-0.2, 0.2, (4000, 3, 3))).astype(F)
    sets.append(_touching_queries(rng, base, 1.0, 10))
    a, b = rng.randint(-4, 5, (30000, 3)), rng.randint(-3, 4, (30000, 3))
    solid = rng.randint(-4, 5, (30000, 1, 3)) + rng.randint(-3, 4, (30000, 3, 3))
    seg, pt = np.stack([a, a, a + b], axis=1), np.stack([a, a, a], axis=1)
    sets.append(((solid[:10000] / 8.0).astype(F), (seg[:10000] / 8.0).astype(F)))
    sets.append(((seg[10000:20000] / 8.0).astype(F), (solid[10000:20000] / 8.0).astype(F)))
    sets.append(((solid[20000:25000] / 8.0).astype(F), (pt[20000:25000] / 8.0).astype(F)))
    sets.append(((pt[25000:] / 8.0).astype(F), (seg[25000:] / 8.0).astype(F)))
    big = (rng.uniform(-1, 1, (2000, 3, 3)) * 10.0 ** rng.uniform(10, 19.4, (2000, 1, 1))).astype(F)   # squares that overflow
    sets.append((big, big[::-1].copy()))
    t, q = np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])
    q[::997, 0, 0] = np.nan                                                # what the kernel never sees: still one answer
    q[1::997, 2, 1] = np.inf
    t[2::997, 1, 2] = -np.inf
    with np.errstate(all="ignore"):
        v0, e1, e2 = _split(t)
    return v0, e1, e2, q[:, 0], q[:, 1], q[:, 2]


def test_kernel_tri_dist_on_the_host_is_the_model(tmp_path):
    """psm_tri_dist_dev.h itself as a stand-alone host program with its own main, built with -ffp-contract=off and the address
    and undefined-behaviour sanitizers and run as a process of its own on the CPU: d2 and the four weights of every pair are
    the model's bit for bit (two NaNs count as equal)"""
    hipcc = "/opt/rocm/bin/hipcc"
    exe, fin, fout = (str(tmp_path / x) for x in ("tri_dist_host", "pairs.bin", "out.bin"))
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "prismarine-core_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "tri_dist_host.cpp"), "-o", exe])
    v0, e1, e2, a, b, c = _host_pairs()
    rec = np.concatenate([v0, e1, e2, a, b, c], axis=1).astype(F)
    assert rec.shape[1] == 18 and rec.shape[0] >= 300000
    rec.tofile(fin)
    done = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode(errors="replace")
    got = np.fromfile(fout, F).reshape(-1, 5)
    want = np.stack(TD.tri_dist(v0, e1, e2, a, b, c), axis=1).astype(F)
    assert got.shape == want.shape
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    bad = np.nonzero(~same.all(axis=1))[0]
    assert bad.size == 0, "%d differ, first %d: %s got %s want %s" % (bad.size, bad[0], rec[bad[0]], got[bad[0]], want[bad[0]])
    finite = np.isfinite(rec).all(axis=1)
    assert np.isfinite(want[finite][:, 1:]).all()                           # finite weights for every finite input
    assert 0.05 < (want[:, 0] == 0).mean() < 0.8 and np.isnan(want[:, 0]).any() and np.isinf(want[:, 0]).any()


# ---- the library, the headers, the kernels ---------------------------------------------------------------------------------------

ENTRIES = ("psm_bvh_tri_closest_dev", "psm_bvh_tri_within_dev")
METHODS = ("triClosest", "triWithin")


def test_library_exports_the_clearance_queries(psm):
    lib = psm.lib()
    header = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    for s in ENTRIES:
        assert hasattr(lib, s) and s in psm.EXPORTS and re.search(r"\b%s\(" % s, header), s
    assert re.search(r"float a\[3\], rmax;\s+float b\[3\], pad0;\s+float c\[3\], pad1;\s+} psm_tri_dist_query;", header)
    assert re.search(r"float u, v, dist;[^}]*int32_t tri;\s+float s, t, zero0, zero1;\s+} psm_tri_hit;", header)
    assert "clearance queries against a built hierarchy (new; no reference counterpart; DESIGN.md 4.23)" in header
    assert "not a point of the intersection" in header
    dt = psm.TRI_DIST_QUERY_DT
    assert dt.itemsize == 48 and [dt.fields[f][1] for f in ("a", "rmax", "b", "c")] == [0, 12, 16, 32]
    ht = psm.TRI_HIT_DT
    assert ht.itemsize == 32 and [ht.fields[f][1] for f in ("u", "v", "dist", "tri", "s", "t")] == [0, 4, 8, 12, 16, 20]
    assert [ht.fields[f][1] for f in ("u", "v", "tri")] == [psm.HIT_DT.fields[f][1] for f in ("u", "v", "tri")]
    for m in METHODS:
        assert callable(getattr(psm.TriangleHierarchy, m)), m
        for other in (psm.QueryScene, psm.InstancedScene, psm.InstanceWorld):                  # a single hierarchy's only
            assert not hasattr(other, m), (other, m)
    hpp = open(os.path.join(ROOT, "include", "Prismarine", "TriangleHierarchy.hpp")).read()
    inl = open(os.path.join(ROOT, "include", "Prismarine", "TriangleHierarchy.inl")).read()
    for m, s in zip(METHODS, ENTRIES):
        assert re.search(r"int %s\(const psm_tri_dist_query \*" % m, hpp) and "TriangleHierarchy::%s(" % m in inl and s + "(bvh," in inl
    dev = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "psm_tri_dist_dev.h")).read()
    assert "0x1p-16f" in dev and "not a point of the intersection" in dev
    makefile = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "Makefile")).read()
    assert " tri_dist.hip " in makefile and re.search(r"tri_dist\.o:.*psm_tri_dist_dev\.h", makefile)


def test_clearance_refusals_without_a_hierarchy(psm):
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for fn in (lib.psm_bvh_tri_closest_dev, lib.psm_bvh_tri_within_dev):   # no hierarchy: refused before anything is touched
        assert fn(None, p, ctypes.c_size_t(1), p) == -1
        assert fn(None, None, ctypes.c_size_t(0), None) == -1
    assert not any(buf)

    class NoCall:   # the packing of the Python layer, seen by a hierarchy that cannot make a call
        ctx = None
        _scene = False
        seen = []

        def _launch_np(self, packed, out, name):
            self.seen.append((packed, out, name))
            raise AssertionError("a launch was made")
        _tri_dist_query = psm.TriangleHierarchy._tri_dist_query
        triClosest = psm.TriangleHierarchy.triClosest
        triWithin = psm.TriangleHierarchy.triWithin
    q = np.arange(18, dtype=F)
    for shape in ((2, 3, 3), (2, 9)):
        for call, out, name in ((lambda x: NoCall().triClosest(x), "trihits", ENTRIES[0]),
                                (lambda x: NoCall().triClosest(x, F([0.5, 2])), "trihits", ENTRIES[0]),
                                (lambda x: NoCall().triWithin(x, 0.25), "bool", ENTRIES[1])):
            with pytest.raises(AssertionError, match="a launch was made"):
                call(q.reshape(shape))
            packed, got_out, got_name = NoCall.seen[-1]
            assert (got_out, got_name) == (out, name) and packed.shape == (2, 12) and packed.dtype == F
            assert np.array_equal(packed.reshape(2, 3, 4)[:, :, :3].reshape(2, 9), q.reshape(2, 9)) and not packed[:, [7, 11]].any()
    assert list(NoCall.seen[-1][0][:, 3]) == [0.25, 0.25] and list(NoCall.seen[-2][0][:, 3]) == [0.5, 2] and np.isinf(NoCall.seen[-3][0][:, 3]).all()
    hits = psm.QueryTriHits(TD.miss_records(2))
    assert list(hits.tri) == [-1, -1] and np.isinf(hits.dist).all() and len(hits) == 2
    pm, pq = hits.points(np.zeros((1, 3, 3), F), q.reshape(2, 3, 3))
    assert np.isnan(pm).all() and np.isnan(pq).all()


# What each kernel reaches with the Makefile's flags, as ceilings: VGPRs, SGPRs, the waves per SIMD its
# __launch_bounds__ ask for (what the unforced figure gives: 512 / VGPRs rounded up to 8), no scratch, no spills, no lane writes,
# the LDS of the 16-entry stack.
CLEARANCE_KERNELS = {"bvh_query_tri_closest": (113, 82, 4), "bvh_query_tri_within": (143, 72, 3)}


def test_clearance_kernels_codegen():
    asm = csrc_asm("tri_dist.hip")
    assert asm.count(".amdhsa_kernel ") == 2
    src = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "tri_dist.hip")).read()
    bounds = re.search(r"TRI_DIST_WAVES = (\d+), TRI_DIST_WITHIN_WAVES = (\d+)", src)
    assert [int(x) for x in bounds.groups()] == [v[2] for v in CLEARANCE_KERNELS.values()]
    for name, (vgprs, sgprs, waves) in CLEARANCE_KERNELS.items():
        blk, body = kernel_asm(asm, "_ZN3psm%d%sENS_9QueryArgsE" % (len(name), name))

        def meta(key):
            return kernel_meta(blk, key)
        assert meta("vgpr_count") <= vgprs and meta("sgpr_count") <= sgprs, (name, meta("vgpr_count"), meta("sgpr_count"))
        assert 512 // ((vgprs + 7) // 8 * 8) == waves, name                    # the bound asks for what the registers give
        assert meta("vgpr_spill_count") == 0 and meta("sgpr_spill_count") == 0, name
        assert meta("private_segment_fixed_size") == 0 and "scratch_" not in body, name
        assert "v_writelane_b32" not in body, name                            # no SGPR parked in a VGPR lane either
        assert meta("group_segment_fixed_size") == 16 * 64 * 4, name          # the stack
        assert "v_div_fixup_f32" in body and "v_sqrt_f32" in body and "v_pk_" not in body, name   # IEEE division and sqrtf, nothing paired


def test_clearance_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "tri_dist_query_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "tri_dist_query_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)
