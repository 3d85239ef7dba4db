"""CPU tests (no GPU) of the triangle queries (psm_bvh_tri_overlaps_dev / psm_bvh_tri_count_dev / psm_bvh_tri_triangles_dev,
tri.hip; TriangleHierarchy.triOverlaps / triCount / triTriangles): the float32 model (tests/tri_query_model.py)
against the same formulas in float64 and against an exact integer test on the lattice, closedness and degenerate triangles, the
rows' order and prefixes, the prune's margin in float64, psm_tri_dev.h itself on the host under the sanitizers, the exports and
the refusals, what tri.hip compiles to, and the header layer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import point_query_model as PQ
import tri_query_model as TQ
from point_query_model import _split
from util import ROOT, csrc_asm, kernel_asm, kernel_meta

F = np.float32
D = np.float64
U = np.uint32


def _f64_reading(tris, q):
    """pair i = (stored triangle i, query triangle i): the float32 answer, the float64 answer of the same formulas on the same
    stored (v0, e1, e2), and the float64 gap on the deciding axis in length units (the largest gap / axis length over the axes
    that have a length)"""
    v0, e1, e2 = _split(tris)
    q = np.asarray(q, F).reshape(-1, 3, 3)
    got = TQ.tri_tri(v0, e1, e2, q[:, 0], q[:, 1], q[:, 2])
    with np.errstate(all="ignore"):
        sep, gap, length = TQ.axes(*(x.astype(D) for x in (v0, e1, e2, q[:, 0], q[:, 1], q[:, 2])))
        decide = np.where(length > 0, gap / np.where(length > 0, length, 1), -np.inf).max(axis=0)
    return got, ~sep.any(axis=0), decide


# ---- an independent exact test on integer coordinates: an edge of one triangle against the other triangle --------------------

def _cross_i(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot_i(a, b):
    return (a * b).sum(axis=-1)


def _orient2(a, b, c):
    return (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0])


def _in_tri2(p, t):
    """p [n, 2] in the closed 2-D triangle t [n, 3, 2] (not degenerate): the three orientation signs agree"""
    o = np.stack([_orient2(t[:, i], t[:, (i + 1) % 3], p) for i in range(3)])
    return (o >= 0).all(axis=0) | (o <= 0).all(axis=0)


def _seg_seg2(p, q, r, s):
    """closed 2-D segments p q and r s (neither a point) meet"""
    o1, o2, o3, o4 = _orient2(p, q, r), _orient2(p, q, s), _orient2(r, s, p), _orient2(r, s, q)
    straddle = (np.sign(o1) * np.sign(o2) <= 0) & (np.sign(o3) * np.sign(o4) <= 0)
    collinear = (o1 == 0) & (o2 == 0) & (o3 == 0) & (o4 == 0)
    boxes = (np.maximum(np.minimum(p, q), np.minimum(r, s)) <= np.minimum(np.maximum(p, q), np.maximum(r, s))).all(axis=-1)
    return np.where(collinear, boxes, straddle)


def _seg_tri_exact(s0, s1, t):
    """closed segment s0 s1 (int64 [n, 3], not a point) against the closed triangle t (int64 [n, 3, 3], not degenerate)"""
    n_pairs = s0.shape[0]
    q0 = t[:, 0]
    N = _cross_i(t[:, 1] - q0, t[:, 2] - q0)
    d0, d1 = _dot_i(N, s0 - q0), _dot_i(N, s1 - q0)
    inplane = (d0 == 0) & (d1 == 0)
    crossing = ~inplane & (np.sign(d0) * np.sign(d1) <= 0)
    Dn = d0 - d1                                              # where the segment crosses the plane: q0 + X / Dn
    X = (s0 - q0) * Dn[:, None] + d0[:, None] * (s1 - s0)
    w = []
    for i in range(3):
        ri, rj = t[:, i] - q0, t[:, (i + 1) % 3] - q0
        w.append(_dot_i(N, _cross_i(rj - ri, X - ri * Dn[:, None])))
    w = np.stack(w)
    pierce = crossing & ((w >= 0).all(axis=0) | (w <= 0).all(axis=0))
    # the segment lies in the triangle's plane: in 2-D, without the normal's largest component
    drop = np.abs(N).argmax(axis=1)
    keep = np.array([[1, 2], [0, 2], [0, 1]])[drop]
    rows = np.arange(n_pairs)[:, None]
    a2, b2 = s0[rows, keep], s1[rows, keep]
    t2 = np.stack([t[:, i][rows, keep] for i in range(3)], axis=1)
    flat = _in_tri2(a2, t2) | _in_tri2(b2, t2)
    for i in range(3):
        flat |= _seg_seg2(a2, b2, t2[:, i], t2[:, (i + 1) % 3])
    return np.where(inplane, flat, pierce)


def _exact_meet(t1, t2):
    """two closed triangles on integer coordinates (int64 [n, 3, 3], neither degenerate) meet: some edge of one meets the
    other (coplanar pairs: the edges lie in the other's plane and are judged in 2-D by orientation signs)"""
    out = np.zeros(t1.shape[0], bool)
    for a, b in ((t1, t2), (t2, t1)):
        for i in range(3):
            out |= _seg_tri_exact(a[:, i], a[:, (i + 1) % 3], b)
    return out


def _lattice(seed, n):
    """pairs with vertices on the 1/8 lattice of [-1, 1]^3, in lattice units (int64): half of the pairs small and near each
    other, an eighth forced coplanar (one shared coordinate)"""
    rng = np.random.RandomState(seed)
    t = rng.randint(-8, 9, (n, 3, 3))
    q = rng.randint(-8, 9, (n, 3, 3))
    h = n // 2
    t[:h, 1:] = t[:h, :1] + rng.randint(-2, 3, (h, 2, 3))
    q[:h, :1] = t[:h, :1] + rng.randint(-3, 4, (h, 1, 3))
    q[:h, 1:] = q[:h, :1] + rng.randint(-2, 3, (h, 2, 3))
    e = n // 8
    k = rng.randint(0, 3, e)
    val = t[np.arange(e), 0, k]
    for v in range(3):
        t[np.arange(e), v, k] = val
        q[np.arange(e), v, k] = val
    return np.clip(t, -8, 8).astype(np.int64), np.clip(q, -8, 8).astype(np.int64)


def test_model_on_the_lattice_is_the_float64_answer_and_the_exact_one():
    """all arithmetic exact: float32 equals float64 for every pair, none left out, and both equal an exact integer test on
    every non-degenerate pair; a good part of the pairs touch exactly or are coplanar"""
    ti, qi = _lattice(1, 200000)
    tris, q = (ti / 8.0).astype(F), (qi / 8.0).astype(F)
    got, want, decide = _f64_reading(tris, q)
    assert np.array_equal(got, want)
    nt, nq = _cross_i(ti[:, 1] - ti[:, 0], ti[:, 2] - ti[:, 0]), _cross_i(qi[:, 1] - qi[:, 0], qi[:, 2] - qi[:, 0])
    solid = np.nonzero(nt.any(axis=1) & nq.any(axis=1))[0]
    exact = _exact_meet(ti[solid], qi[solid])
    bad = solid[got[solid] != exact]
    assert solid.size >= 20000 and bad.size == 0, (bad.size, ti[bad[:1]], qi[bad[:1]])
    coplanar = (_dot_i(nt[solid][:, None, :], qi[solid] - ti[solid][:, :1]) == 0).all(axis=1)
    touch = decide[solid] == 0
    print("pairs %d, non-degenerate %d, meet %.1f %%, touch exactly %d, coplanar %d (of them meet %d)"
          % (got.size, solid.size, 100 * got.mean(), touch.sum(), coplanar.sum(), (coplanar & exact).sum()))
    assert touch.sum() > 2000 and coplanar.sum() > 1000
    assert 0.05 < got.mean() < 0.8 and (coplanar & exact).any() and (coplanar & ~exact).any()


def _soup(seed, n):
    rng = np.random.RandomState(seed)
    c = rng.uniform(-1, 1, (n, 1, 3))
    tris = c + rng.uniform(-0.3, 0.3, (n, 3, 3))
    qc = c + rng.uniform(-0.4, 0.4, (n, 1, 3))
    return tris, qc + rng.uniform(-0.3, 0.3, (n, 3, 3))


@pytest.mark.parametrize("shift", [0.0, 1000.0], ids=["soup", "soup_moved_by_1000"])
def test_model_on_a_random_soup_is_the_float64_answer_outside_the_band(shift):
    """equal for every pair whose float64 gap on the deciding axis exceeds 1e-5 length units; at most 2 % of the pairs may lie
    inside that band"""
    tris, q = _soup(2, 200000)
    tris, q = ((x.astype(F) + F(shift)).astype(F) for x in (tris, q))
    got, want, decide = _f64_reading(tris, q)
    band = np.abs(decide) <= 1e-5
    print("pairs %d, differ %d, in the band %.4f %%, meet %.1f %%" % (got.size, (got != want).sum(), 100 * band.mean(), 100 * want.mean()))
    assert band.mean() <= 0.02
    assert np.array_equal(got[~band], want[~band])
    assert 0.03 < want.mean() < 0.5


def _counts(tri, q):
    v0, e1, e2 = _split(np.asarray(tri, F).reshape(1, 3, 3))
    q = np.asarray(q, F).reshape(1, 3, 3)
    return bool(TQ.tri_tri(v0, e1, e2, q[:, 0], q[:, 1], q[:, 2])[0])


def test_model_is_closed_and_handles_degenerate_triangles():
    tri = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]])                    # in the plane z = 0
    step = 0.125
    touching = (([[0, 0, 0], [-0.5, -0.25, 0.5], [-0.25, -0.5, 0.5]], [0, 0, step]),              # a shared vertex only
                ([[0, 0, 0], [0.5, 0, 0], [0.25, 0, 0.5]], [0, -step, 0]),                       # a shared edge
                ([[0, 0, 0], [0.5, 0, 0], [0.25, -0.5, 0]], [0, -step, 0]),                      # coplanar, edge to edge
                ([[0.125, 0.125, 0], [0.125, 0.25, 0.5], [0.25, 0.125, 0.5]], [0, 0, step]),     # a vertex in the interior
                ([[0.125, 0.125, 0], [0.25, 0.125, 0], [0.125, 0.25, 0]], [0, 0, step]),         # coplanar, one inside the other
                ([[0.5, 0, 0], [1, -0.5, 0], [1, 0.5, 0]], [step, 0, 0]))                        # coplanar, vertex to vertex
    for q, apart in touching:
        q = np.array(q)
        for order in ([0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1]):
            assert _counts(tri[order], q) and _counts(q[order], tri), q                  # either one stored, any vertex first
            assert not _counts(tri[order], q + apart) and not _counts(q[order] + apart, tri), q   # one lattice step apart
    away = np.array([[0.5, 0.5, 0], [0.375, 0.5, 0], [0.5, 0.375, 0]])      # coplanar and disjoint, the bounding boxes overlap
    assert not _counts(tri, away) and not _counts(away, tri)
    assert _counts(tri, away - [2 * step, step, 0])                         # ... until an edge of it reaches the hypotenuse
    # degenerate triangles on the lattice: the float64 answer of the same formulas, both outcomes present
    rng = np.random.RandomState(3)
    n = 30000
    a, b = rng.randint(-4, 5, (n, 3)), rng.randint(-3, 4, (n, 3))
    solid = rng.randint(-4, 5, (n, 1, 3)) + rng.randint(-3, 4, (n, 3, 3))
    segment, point, two_equal = np.stack([a, a, a + b], axis=1), np.stack([a, a, a], axis=1), np.stack([a, a + b, a + b], axis=1)
    for tris, q in ((solid, segment), (solid, segment[:, [2, 0, 1]]), (solid, point), (two_equal, solid), (two_equal[:, [1, 0, 2]], solid),
                    (segment, segment[::-1]), (point, solid)):
        got, want, _ = _f64_reading((tris / 8.0).astype(F), (q / 8.0).astype(F))
        assert np.array_equal(got, want) and got.any() and not got.all()
    # A point query counts iff the point lies on the triangle: exactly, by integers (in the plane, and inside in 2-D), and as
    # the point queries' model sees it. That model divides (u = 2 / 3 rounds), so a point on the triangle gets d2 = 0 or the
    # square of its quotients' rounding (observed: 5 of 29 704 points at d2 ~ 1e-15), while a lattice point off a lattice
    # triangle of this size is at least 1 / 680 of a step away (|n . (p - v0)| >= 1 and |n| < 680 in lattice units): d2 > 3e-8.
    # Every point the model puts at distance 0 counts, and the query counts iff d2 is below 1e-10, between the two.
    normal = _cross_i(solid[:, 1] - solid[:, 0], solid[:, 2] - solid[:, 0])
    flat = normal.any(axis=1)
    ti, pi, normal = solid[flat], a[flat], normal[flat]
    tris, p = (ti / 8.0).astype(F), (pi / 8.0).astype(F)
    got, _, _ = _f64_reading(tris, np.stack([p, p, p], axis=1))
    keep = np.array([[1, 2], [0, 2], [0, 1]])[np.abs(normal).argmax(axis=1)]
    rows = np.arange(ti.shape[0])[:, None]
    on = (_dot_i(normal, pi - ti[:, 0]) == 0) & _in_tri2(pi[rows, keep], np.stack([ti[:, i][rows, keep] for i in range(3)], axis=1))
    assert np.array_equal(got, on) and got.sum() > 50
    v0, e1, e2 = _split(tris)
    d2 = PQ.closest_on_tris(v0, e1, e2, p)[2]
    print("points on their triangle %d, of them at d2 == 0 %d, the largest d2 among them %.3g, the smallest off %.3g"
          % (got.sum(), (got & (d2 == 0)).sum(), d2[got].max(), d2[~got].min()))
    assert got[d2 == 0].all() and np.array_equal(got, d2 < 1e-10)


def test_model_rows_are_sorted_prefixes_and_counts_agree():
    rng = np.random.RandomState(4)
    c = rng.uniform(-1, 1, (300, 1, 3))
    tris = (c + rng.uniform(-0.2, 0.2, (300, 3, 3))).astype(F)
    cand = rng.permutation(300)[:280]
    q = (rng.uniform(-1, 1, (500, 1, 3)) + rng.uniform(-0.7, 0.7, (500, 3, 3))).astype(F)
    q[4:44] = (rng.uniform(-0.3, 0.3, (40, 1, 3)) + rng.uniform(-3, 3, (40, 3, 3))).astype(F)     # large ones: more than 16 meet
    q[0, 0, 0], q[1, 1, 1], q[2, 2], q[3, 0, 2] = np.nan, np.inf, -np.inf, -np.inf
    flag, count, big, nbig = TQ.query(tris, cand, q, 16)
    ok, ids = TQ.counts_matrix(tris, cand, q)
    assert np.array_equal(count, ok.sum(axis=1)) and np.array_equal(flag, count > 0) and (count[:4] == 0).all()
    assert (count > 16).any() and ((count > 0) & (count < 16)).any() and (count == 0).sum() > 4
    for k in (1, 2, 3, 8, 16):
        f, c_, rows, nrows = TQ.query(tris, cand, q, k)
        assert np.array_equal(rows, big[:, :k]) and np.array_equal(nrows, np.minimum(count, k)) and np.array_equal(c_, count)
        assert np.array_equal(rows >= 0, np.arange(k)[None] < nrows[:, None]) and np.array_equal(nrows > 0, f)
        assert np.isin(rows[rows >= 0], cand).all()
        assert ((rows[:, :-1] < rows[:, 1:]) | (rows[:, 1:] < 0)).all()
    for i in np.nonzero(count)[0][:50]:                                 # the k lowest ids that count, by a sort
        assert list(big[i, :nbig[i]]) == sorted(ids[ok[i]])[:16]


# ---- the prune's margin (the chain is 4.15's) -------------------------------------------------------------------

def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def _fit_like(rng, tris, kind):
    """a fit transform as the build makes them, as float32: the vertices' image lies in [0, 1]^3. kind 0: the plain fit (diagonal,
    the bounds of each axis to [0, 1]); kind 1: a rotation; kind 2: rotate-and-scale with condition number up to 16 -- for both
    the image is scaled uniformly into the unit cube, which keeps the condition number"""
    v = tris.reshape(-1, 3).astype(D)
    if kind == 0:
        A = np.eye(3)
    else:
        s = np.ones(3) if kind == 1 else np.array([1.0, rng.uniform(1, 16), 16.0])[rng.permutation(3)]
        A = _rotation(rng) @ np.diag(s) @ _rotation(rng)
    y = v @ A.T
    lo, ext = y.min(0), y.max(0) - y.min(0)
    if kind != 0:
        ext = np.full(3, ext.max())
    M = np.zeros((3, 4))
    M[:, :3] = A / ext[:, None]
    M[:, 3] = -lo / ext
    return M.astype(F)


def _prune_figures(M, tris, q):
    """For stored / query triangle arrays that broadcast against each other ([..., 3, 3]): which pairs count (float32), whether
    the kernel's float32 prune keeps the stored triangle's exact image (a leaf box with no padding at all), and per normalised
    axis the observed distance of the exact images (the stored triangle's and the query's bounding box's), the bound claimed
    for it, and the margin granted"""
    v0, e1, e2 = _split(tris)
    v0, e1, e2 = (x.reshape(tris.shape[:-2] + (3,)) for x in (v0, e1, e2))
    counts = TQ.tri_tri(v0, e1, e2, q[..., 0, :], q[..., 1, :], q[..., 2, :])
    lo, hi = q.min(axis=-2), q.max(axis=-2)                          # exact: selections
    Md = M.astype(D)
    V = np.stack([v0.astype(D), v0.astype(D) + e1.astype(D), v0.astype(D) + e2.astype(D)], axis=-2)   # the stored triangle
    img = V @ Md[:, :3].T + Md[:, 3]
    tmin, tmax = img.min(axis=-2), img.max(axis=-2)
    pa, pb = lo.astype(D)[..., None, :] * Md[:, :3], hi.astype(D)[..., None, :] * Md[:, :3]           # [..., axis, j]
    elo, ehi = np.minimum(pa, pb).sum(-1) + Md[:, 3], np.maximum(pa, pb).sum(-1) + Md[:, 3]
    S = np.maximum(np.abs(pa), np.abs(pb)).sum(-1) + np.abs(Md[:, 3])
    observed = np.maximum(0, np.maximum(tmin - ehi, elo - tmax))
    lam = np.sqrt((Md[:, :3] ** 2).sum(axis=1))
    size = np.abs(np.concatenate([e1, e2], axis=-1).astype(D)).max(axis=-1)
    bound = lam * 2.0 ** -20 * size[..., None]                       # |row| x 16 eps x the triangle's size (eps = 2^-24)
    granted = (2 + S) * 2.0 ** -16 - 4 * 2.0 ** -24 * S              # h less the rounding of the float32 image (4 operations)
    # the prune as tri.hip computes it with box_row, in float32
    fa, fb = lo[..., None, :] * M[:, :3], hi[..., None, :] * M[:, :3]
    mn, mx, ab = np.minimum(fa, fb), np.maximum(fa, fb), np.maximum(np.abs(fa), np.abs(fb))
    ilo = ((mn[..., 0] + mn[..., 1]) + mn[..., 2]) + M[:, 3]
    ihi = ((mx[..., 0] + mx[..., 1]) + mx[..., 2]) + M[:, 3]
    h = (F(2) + (((ab[..., 0] + ab[..., 1]) + ab[..., 2]) + np.abs(M[:, 3]))) * F(2.0 ** -16)
    assert ilo.dtype == F and h.dtype == F
    kept = (~(tmax < (ilo - h).astype(D)) & ~(tmin > (ihi + h).astype(D))).all(axis=-1)
    shape = observed.shape
    return counts, kept, observed, np.broadcast_to(bound, shape), np.broadcast_to(granted, shape)


def _touching_queries(rng, tris, scale, per):
    """`per` query triangles for each stored triangle that touch it or miss it by a few ulps: a vertex of the query, or a point
    of one of its edges, on a vertex, a point of an edge or an interior point of the stored triangle, the rest of the query
    reaching away from it, the whole moved by -8 .. 8 ulps"""
    t = np.repeat(tris.astype(D), per, axis=0)
    n = t.shape[0]
    w = rng.uniform(0, 1, (n, 3))
    kind = rng.randint(0, 3, n)
    w[kind == 0] = np.eye(3)[rng.randint(0, 3, (kind == 0).sum())]
    w[kind == 1, rng.randint(0, 3, (kind == 1).sum())] = 0
    w /= w.sum(axis=1, keepdims=True)
    p = (t * w[:, :, None]).sum(axis=1)
    away = -np.sign(t.mean(axis=1) - p)
    away[away == 0] = 1
    ext = 10.0 ** rng.uniform(-3, 0.5, (n, 2, 3)) * scale
    nudge = rng.randint(-8, 9, (n, 1)) * np.spacing(np.abs(p).astype(F)).astype(D)
    q = np.empty((n, 3, 3))
    q[:, 0] = p
    q[:, 1], q[:, 2] = p + away * ext[:, 0], p + away * ext[:, 1]
    edge = rng.uniform(size=n) < 0.5                                   # the contact on an edge of the query, not a vertex
    u = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 0.5, (n, 1)) * scale
    s = rng.uniform(0.1, 2.0, (n, 1))
    q[edge, 0], q[edge, 1] = (p + u)[edge], (p - s * u)[edge]
    q += (away * nudge)[:, None, :]
    return np.repeat(tris, per, axis=0), q[:, rng.permutation(3)].astype(F)


def test_prune_margin_covers_every_triangle_that_counts():
    """DESIGN.md 4.15's chain for the triangle queries, in float64, over plain, rotating and rotate-and-scale (condition number
    up to 16) fit transforms and six decades of magnitude: for every pair that counts under tri_tri, on every normalised axis,
        the distance of the exact images <= |row| 16 eps size(triangle) <= h less the image's rounding,
    and tri.hip's float32 interval keeps the stored triangle's exact image even with no leaf padding at all."""
    rng = np.random.RandomState(5)
    worst, total, conds = 0.0, 0, []
    for mag in range(-3, 4):
        scale = 10.0 ** mag
        for kind in (0, 1, 2):
            c = rng.uniform(-1, 1, (250, 1, 3))
            tris = ((c + rng.uniform(-0.2, 0.2, (250, 3, 3)) * rng.uniform(0.02, 1, (250, 1, 1))) * scale).astype(F)
            M = _fit_like(rng, tris, kind)
            conds.append(np.linalg.cond(M[:, :3].astype(D)))
            qc = rng.uniform(-1.1, 1.1, (250, 1, 3))
            q = ((qc + rng.uniform(-1, 1, (250, 3, 3)) * 10.0 ** rng.uniform(-3, 0, (250, 1, 1))) * scale).astype(F)
            pairs = [(tris[None], q[:, None])]                                                    # every query x every triangle
            pairs.append(_touching_queries(rng, tris, scale, 12))                                 # and the close calls
            for t, qq in pairs:
                counts, kept, observed, bound, granted = _prune_figures(M, t, qq)
                assert counts.any() and kept[counts].all(), (mag, kind)
                assert (observed[counts] <= bound[counts]).all(), (mag, kind, (observed[counts] / bound[counts]).max())
                assert (bound <= granted).all(), (mag, kind, (bound / granted).max())
                worst = max(worst, (observed[counts] / bound[counts]).max())
                total += counts.sum()
    print("pairs that count: %d; the largest observed / bound: %.3g; condition numbers up to %.1f" % (total, worst, max(conds)))
    assert max(conds) > 12 and total > 20000


# ---- psm_tri_dev.h itself, on the host -----------------------------------------------------------------------------------------

def _host_pairs():
    """(v0, e1, e2, a, b, c) of at least 300 000 pairs: lattice, soup, moved soup, touching, degenerate"""
    rng = np.random.RandomState(7)
    ti, qi = _lattice(8, 120000)
    sets = [((ti / 8.0).astype(F), (qi / 8.0).astype(F))]
    t, q = _soup(9, 80000)
    sets.append((t.astype(F), q.astype(F)))
    sets.append(((t.astype(F) + F(1000)).astype(F), (q.astype(F) + F(1000)).astype(F)))
    c = rng.uniform(-1, 1, (5000, 1, 3))
    base = (c + rng.uniform(-0.2, 0.2, (5000, 3, 3))).astype(F)
    sets.append(_touching_queries(rng, base, 1.0, 12))
    a, b = rng.randint(-4, 5, (30000, 3)), rng.randint(-3, 4, (30000, 3))
    solid = rng.randint(-4, 5, (30000, 1, 3)) + rng.randint(-3, 4, (30000, 3, 3))
    seg = np.stack([a, a, a + b], axis=1)
    sets.append(((solid[:15000] / 8.0).astype(F), (seg[:15000] / 8.0).astype(F)))
    sets.append(((seg[15000:] / 8.0).astype(F), (solid[15000:] / 8.0).astype(F)))
    t, q = np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])
    q[::997, 0, 0] = np.nan                                                # what the kernel never sees: still one answer
    q[1::997, 2, 1] = np.inf
    v0, e1, e2 = _split(t)
    return v0, e1, e2, q[:, 0], q[:, 1], q[:, 2]


def test_kernel_tri_tri_on_the_host_is_the_model(tmp_path):
    """psm_tri_dev.h itself as a stand-alone host program with its own main, built with -ffp-contract=off and the address and
    undefined-behaviour sanitizers and run as a process of its own on the CPU: the flag of every pair is the model's"""
    hipcc = "/opt/rocm/bin/hipcc"
    exe, fin, fout = (str(tmp_path / x) for x in ("tri_tri_host", "pairs.bin", "out.bin"))
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "prismarine-core_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "tri_tri_host.cpp"), "-o", exe])
    v0, e1, e2, a, b, c = _host_pairs()
    rec = np.concatenate([v0, e1, e2, a, b, c], axis=1).astype(F)
    assert rec.shape[1] == 18 and rec.shape[0] >= 300000
    rec.tofile(fin)
    done = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode(errors="replace")
    got = np.fromfile(fout, np.uint8).astype(bool)
    want = TQ.tri_tri(v0, e1, e2, a, b, c)
    bad = np.nonzero(got != want)[0] if got.shape == want.shape else np.zeros(1, int)
    assert got.shape == want.shape and bad.size == 0, "%d differ, first %d: %s" % (bad.size, bad[0], rec[bad[0]])
    assert 0.05 < want.mean() < 0.8


# ---- the library, the headers, the kernels ---------------------------------------------------------------------------------------

TRI_ENTRIES = ("psm_bvh_tri_overlaps_dev", "psm_bvh_tri_count_dev", "psm_bvh_tri_triangles_dev")
TRI_METHODS = ("triOverlaps", "triCount", "triTriangles")


def test_library_exports_the_triangle_queries(psm):
    lib = psm.lib()
    header = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    for s in TRI_ENTRIES:
        assert hasattr(lib, s) and s in psm.EXPORTS and re.search(r"\b%s\(" % s, header), s
    assert re.search(r"float a\[3\], pad0;\s+float b\[3\], pad1;\s+float c\[3\], pad2;\s+} psm_tri_query;", header)
    assert psm.TRI_QUERY_DT.itemsize == 48 and [psm.TRI_QUERY_DT.fields[f][1] for f in ("a", "b", "c")] == [0, 16, 32]
    assert "triangle queries against a built hierarchy" in header and psm.QUERY_K_MAX == 16 == TQ.K_MAX
    for m in TRI_METHODS:
        assert callable(getattr(psm.TriangleHierarchy, m)), m
        for other in (psm.QueryScene, psm.InstancedScene, psm.InstanceWorld):                  # a single hierarchy's only
            assert not hasattr(other, m), (other, m)
    hpp = open(os.path.join(ROOT, "include", "Prismarine", "TriangleHierarchy.hpp")).read()
    inl = open(os.path.join(ROOT, "include", "Prismarine", "TriangleHierarchy.inl")).read()
    for m, s in zip(TRI_METHODS, TRI_ENTRIES):
        assert re.search(r"int %s\(const psm_tri_query \*" % m, hpp) and "TriangleHierarchy::%s(" % m in inl and s + "(bvh," in inl


def test_tri_refusals_without_a_hierarchy(psm):
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for fn in (lib.psm_bvh_tri_overlaps_dev, lib.psm_bvh_tri_count_dev):   # no hierarchy: refused before anything is touched
        assert fn(None, p, ctypes.c_size_t(1), p) == -1
        assert fn(None, None, ctypes.c_size_t(0), None) == -1
    assert lib.psm_bvh_tri_triangles_dev(None, p, ctypes.c_size_t(1), ctypes.c_uint32(1), p, p) == -1
    assert lib.psm_bvh_tri_triangles_dev(None, None, ctypes.c_size_t(0), ctypes.c_uint32(0), None, None) == -1
    assert not any(buf)

    class NoCall:   # the Python layer refuses k = 0 and k > 16 before any call: a hierarchy that cannot make one
        ctx = None
        _scene = False

        def _launch_np(self, packed, *a):
            assert packed.shape == (2, 12) and packed.dtype == F and not packed[:, 3::4].any()
            assert np.array_equal(packed.reshape(2, 3, 4)[:, :, :3].reshape(2, 9), np.arange(18, dtype=F).reshape(2, 9))
            raise AssertionError("a launch was made")
        _tri_query = psm.TriangleHierarchy._tri_query
        triTriangles = psm.TriangleHierarchy.triTriangles
    q = np.arange(18, dtype=F)
    for k in (0, 17, 1 << 20):
        with pytest.raises(psm.PsmError, match="k must be 1 .. 16"):
            NoCall().triTriangles(q.reshape(2, 3, 3), k)
    with pytest.raises(ValueError):
        NoCall().triTriangles(q.reshape(2, 3, 3), 2.5)
    for shape in ((2, 3, 3), (2, 9)):
        with pytest.raises(AssertionError, match="a launch was made"):
            NoCall().triTriangles(q.reshape(shape), 16)


# The VGPRs each kernel reaches with the Makefile's flags, as ceilings, and the LDS it declares (the 16-entry stack; the id list is
# dynamic, k x 256 B, and does not show here). The body does not fit the box kernels' 64: __launch_bounds__(64, 7) for the flag
# and the count (72 allocated: 7 waves per SIMD), (64, 6) for the list (80: 6 waves) -- DESIGN.md 4.19.
TRI_VGPRS = {"bvh_query_tri_any": (70, 72), "bvh_query_tri_count": (69, 72), "bvh_query_tri_tris": (80, 80)}


def test_tri_kernels_codegen():
    asm = csrc_asm("tri.hip")
    assert asm.count(".amdhsa_kernel ") == 3
    for name, (ceiling, allocated) in TRI_VGPRS.items():
        blk, body = kernel_asm(asm, "_ZN3psm%d%sENS_9QueryArgsE" % (len(name), name))

        def meta(key):
            return kernel_meta(blk, key)
        assert meta("vgpr_count") <= ceiling <= allocated, (name, meta("vgpr_count"))
        assert meta("vgpr_spill_count") == 0 and meta("sgpr_spill_count") == 0, name
        assert meta("private_segment_fixed_size") == 0 and "scratch_" not in body, name
        assert "v_writelane_b32" not in body, name                            # no SGPR parked in a VGPR lane either
        assert meta("group_segment_fixed_size") == 16 * 64 * 4, name          # the stack; the list is the launch's k x 64 x 4 B
        assert "v_rcp_f32" not in body and "v_sqrt_f32" not in body and "v_div_" not in body, name   # no division, no square root
        assert "v_fma_f32" not in body and "v_fmac_f32" not in body, name     # nothing contracted: one rounding per operation
        assert ("ds_read_b32" in body and "ds_write_b32" in body) or name != "bvh_query_tri_tris", name
    assert 16 * 64 * 4 + TQ.K_MAX * 64 * 4 == 8192                            # the most LDS a launch asks for: stack + 16 slots


def test_tri_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "tri_query_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "tri_query_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)
