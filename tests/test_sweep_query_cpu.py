"""CPU tests (no GPU) of the sphere sweeps (psm_bvh_sweep_sphere_dev / psm_bvh_sweep_occluded_dev, sweep.hip, psm_sweep_dev.h;
TriangleHierarchy.sweepSphere / sweepOccluded): sweep_tri (tests/sweep_query_model.py) in float64 against the
definition of a first contact, in float32 against float64, the residual of a float32 contact, the prune's margin chain in
float64, the contract's cases, the exports and refusals, what sweep.hip compiles to, the header layer, and the kernel's own
sweep_tri as a stand-alone host program under the sanitizers, bit for bit against the model."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import point_query_model as PQ
import sweep_query_model as SQ
from query_model import normalize3
from util import ROOT, csrc_asm, kernel_asm, kernel_meta

F = np.float32
D = np.float64
EPS = 2.0 ** -24


def _soup(seed, n, shift=0.0):
    """pair i = (triangle i, sweep i): triangles of size ~0.3 in [-1.3, 1.3]^3, sweeps from [-2, 2]^3 aimed near their triangle,
    radii over 1e-3 .. 0.5; everything moved by `shift`. Returns v0, e1, e2 as the build stores them, o, the unit d, r."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(-1, 1, (n, 3))
    V = ((c[:, None] + rng.uniform(-0.3, 0.3, (n, 3, 3))) + shift).astype(F)
    v0, e1, e2 = PQ._split(V)
    o = (rng.uniform(-2, 2, (n, 3)) + shift).astype(F)
    d = normalize3(((c + shift + rng.uniform(-0.4, 0.4, (n, 3))) - o).astype(F))
    r = (10 ** rng.uniform(-3, -0.3, n)).astype(F)
    return v0, e1, e2, o, d, r


def _unit(v0, e1, e2, o, r):
    """eps (|o|_inf + |triangle|_inf + r) per pair: what the residual and the grazing band are measured in"""
    V = np.stack([v0.astype(D), v0.astype(D) + e1, v0.astype(D) + e2], axis=-2)
    return EPS * (np.abs(o.astype(D)).max(-1) + np.abs(V).max((-1, -2)) + r)


PATH = 10.0   # the soups' tmax: every contact of theirs lies well before it


@functools.lru_cache(maxsize=None)
def _readings(shift):
    """the three readings of one soup, computed once: float32 and float64 sweep_tri, and the definition"""
    pairs = _soup(1, 20000, shift)
    r32 = SQ.sweep_tri(*pairs, PATH, T=F, feature=True)
    r64 = SQ.sweep_tri(*pairs, PATH, T=D, feature=True)
    td, fmin = SQ.first_contact_by_definition(*pairs, PATH)
    return pairs, r32, r64, td, fmin


SHIFTS = pytest.mark.parametrize("shift", [0.0, 1000.0], ids=["soup", "soup_moved_by_1000"])


@SHIFTS
def test_float64_sweep_tri_is_the_first_contact_by_definition(shift):
    """hit and miss agree wherever the definitional minimum of dist - r is further than 1e-9 from 0, and t to 1e-9 of the path"""
    pairs, _, (t64, _, _, feat), td, fmin = _readings(shift)
    clear = np.abs(fmin) > 1e-9
    assert clear.mean() > 0.999
    assert np.array_equal(np.isfinite(t64)[clear], np.isfinite(td)[clear])
    both = np.isfinite(t64) & np.isfinite(td) & clear
    worst = np.abs(t64[both] - td[both]).max() / PATH
    print("contacts %d of %d, at t = 0 %d, by feature %s; worst |t - t_def| / path %.3g" % (both.sum(), t64.size, (t64 == 0).sum(), np.bincount(feat[both] + 1), worst))
    assert worst <= 1e-9
    assert both.sum() > 4000 and (np.bincount(feat[both] + 1, minlength=8)[:8] > 10).all()     # the start and every feature decide some
    # the contact point the record names is where the sphere touches: |c(t) - contact| = r
    v0, e1, e2, o, d, r = (x.astype(D) for x in pairs)
    _, u, v, _ = _readings(shift)[2]
    pos = both & (t64 > 0)
    gap = np.linalg.norm((o + t64[:, None] * d) - ((v0 + u[:, None] * e1) + v[:, None] * e2), axis=1) - r
    assert np.abs(gap[pos]).max() <= 1e-9


# The grazing band: a float32 answer may differ from the float64 one in hit or miss only where the definitional minimum of
# dist - r is within 64 eps (|o|_inf + |triangle|_inf + r) of 0 -- 16 times the residual bound below, which is what the rounding of
# a contact's position comes to. On the soup at the origin: the one moved by 1000 has eps |o| = 6e-5, a band that a twentieth of
# its pairs lie in, and says nothing.
BAND = 64.0


def test_float32_sweep_tri_is_the_float64_answer_outside_the_grazing_band():
    pairs, (t32, _, _, _), (t64, _, _, _), _, fmin = _readings(0.0)
    band = np.abs(fmin) <= BAND * _unit(pairs[0], pairs[1], pairs[2], pairs[3], pairs[5])
    flips = np.isfinite(t32) != np.isfinite(t64)
    print("pairs %d, in the band %.4f %%, flips %d (outside the band %d)" % (t32.size, 100 * band.mean(), flips.sum(), (flips & ~band).sum()))
    assert band.mean() <= 0.01
    assert not (flips & ~band).any()
    assert np.array_equal(t32 == 0, t64 == 0) or (((t32 == 0) != (t64 == 0)) & ~band).sum() == 0


# ---- sweeps that start at contact: where every sweep leaves its sphere ------------------------------------------------------------

def _from_contact(seed, n):
    """every first contact of a soup, issued again from where it ended: o2 = fl(o + t d), the same d and r. The sphere rests on
    the triangle within rounding of its radius and moves into it."""
    v0, e1, e2, o, d, r = _soup(seed, n)
    t, _, _ = SQ.sweep_tri(v0, e1, e2, o, d, r)
    k = np.isfinite(t)
    return v0[k], e1[k], e2[k], (o[k] + t[k, None] * d[k]).astype(F), d[k], r[k]


def _at_radius(seed, n):
    """starts at r (1 + k ulp), k in -16 .. 16, from a vertex, a point of an edge or an interior point of the triangle, along a
    direction of that feature's normal cone (the face normal tilted outwards by up to 1.2 rad for an edge or a vertex), heading
    into it within 0.5 rad of straight: the closest point of the triangle to the start is the chosen point"""
    rng = np.random.RandomState(seed)
    c = rng.uniform(-1, 1, (n, 1, 3))
    V = (c + rng.uniform(-0.3, 0.3, (n, 3, 3))).astype(F).astype(D)
    kind = rng.randint(0, 3, n)                                   # 0 a vertex, 1 an edge, 2 the face
    i = rng.randint(0, 3, n)
    a, b, cc = (np.take_along_axis(V, ((i + j) % 3)[:, None, None], 1)[:, 0] for j in range(3))
    s = rng.uniform(0.1, 0.9, (n, 1))
    w = rng.dirichlet([2, 2, 2], n)
    q = np.where((kind == 0)[:, None], a, np.where((kind == 1)[:, None], a + s * (b - a), (V * w[:, :, None]).sum(axis=1)))
    nrm = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm *= np.where(rng.uniform(size=(n, 1)) < 0.5, 1.0, -1.0)
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    e = unit(b - a)
    out_edge = unit((a - cc) - ((a - cc) * e).sum(1, keepdims=True) * e)          # in the plane, across the edge, away from the third vertex
    out_vertex = unit(-(unit(b - a) + unit(cc - a)))                                # the outward bisector at the vertex
    out = np.where((kind == 0)[:, None], out_vertex, out_edge)
    tilt = np.where(kind == 2, 0.0, rng.uniform(0, 1.2, n))[:, None]
    x = nrm * np.cos(tilt) + out * np.sin(tilt)
    r = (10 ** rng.uniform(-3, -0.3, n)).astype(F)
    dist = (r + rng.randint(-16, 17, n) * np.spacing(r)).astype(D)
    o = (q + x * dist[:, None]).astype(F)
    side = unit(np.cross(x, rng.normal(size=(n, 3))))
    ang = rng.uniform(0, 0.5, (n, 1))
    d = normalize3((-x * np.cos(ang) + side * np.sin(ang)).astype(F))
    v0, e1, e2 = PQ._split(V.astype(F))
    return v0, e1, e2, o, d, r


CONTACT_SETS = pytest.mark.parametrize("make", [_from_contact, _at_radius], ids=["reissued_from_the_contact", "at_the_radius_plus_k_ulps"])


@CONTACT_SETS
def test_a_sphere_that_starts_at_contact_and_moves_in_is_found(make):
    """the start test and the features round independently; a sphere within rounding of its radius of the triangle that moves
    into it must be seen by one of them. Hit and miss of float32 against float64 and against the definition outside the grazing
    band, the band's share, and where the reported contact leaves the sphere (the residual bound, t = 0 included when a feature
    found it)"""
    pairs = make(2, 60000 if make is _from_contact else 20000)
    v0, e1, e2, o, d, r = pairs
    t32, _, _, feat = SQ.sweep_tri(*pairs, PATH, T=F, feature=True)
    t64, _, _ = SQ.sweep_tri(*pairs, PATH, T=D)
    td, fmin = SQ.first_contact_by_definition(*pairs, PATH)
    unit = _unit(v0, e1, e2, o, r)
    band = np.abs(fmin) <= BAND * unit
    flips = (np.isfinite(t32) != np.isfinite(t64)) | (np.isfinite(t32) != np.isfinite(td))
    found = np.isfinite(t32) & (feat >= 0)                          # by a feature: the sphere is left at r, t = 0 included
    c = o.astype(D) + np.where(found, t32, 0).astype(D)[:, None] * d.astype(D)
    res = (np.abs(SQ.distance_f64(v0, e1, e2, c) - r.astype(D)) / unit)[found]
    start = np.isfinite(t32) & (feat < 0)                           # by the start test: within r, and no further out than rounding
    over = ((SQ.distance_f64(v0, e1, e2, o.astype(D)) - r.astype(D)) / unit)[start]
    print("pairs %d, in the band %.3f %%, flips %d (outside the band %d); found by the start test %d, by a feature at t = 0 %d, later %d; "
          "the largest residual %.3g units, the start test's largest excess %.3g units" % (
              t32.size, 100 * band.mean(), flips.sum(), (flips & ~band).sum(), start.sum(), (found & (t32 == 0)).sum(), (found & (t32 > 0)).sum(),
              res.max(), over.max()))
    assert t32.size > 10000 and band.mean() <= 0.01
    assert not (flips & ~band).any()
    assert (found & (t32 == 0)).sum() > 100 and start.sum() > 100 and (found & (t32 > 0)).sum() > 100
    assert res.max() <= RESIDUAL and over.max() <= RESIDUAL


# The residual: at a float32 contact with t > 0 the centre c(t) = o + t d (exact, from the float32 t) is at a float64 distance from
# the triangle that differs from r by at most RESIDUAL x eps (|o|_inf + |triangle|_inf + r). Measured on these soups: 3.33 units
# (5.8e-7 length units at coordinates up to 2; the soup moved by 1000 reaches 0.005 units: its subtractions are exact); on
# the sweeps that start at contact (above) 1.43. Asserted: four times the 3.33 this file itself observes, rounded up (on 400 000
# further pairs of the same recipe, seeds 10 .. 29, which no test runs, the largest observed was 4.50). DESIGN.md 4.17.
RESIDUAL = 14.0


@SHIFTS
def test_float32_contact_leaves_the_sphere_on_the_triangle(shift):
    pairs, (t32, _, _, _), _, _, _ = _readings(shift)
    v0, e1, e2, o, d, r = pairs
    pos = np.isfinite(t32) & (t32 > 0)
    c = o.astype(D) + np.where(pos, t32, 0).astype(D)[:, None] * d.astype(D)
    res = np.abs(SQ.distance_f64(v0, e1, e2, c) - r.astype(D))[pos] / _unit(v0, e1, e2, o, r)[pos]
    print("contacts with t > 0: %d; the largest residual %.3g units of eps (|o| + |triangle| + r)" % (pos.sum(), res.max()))
    assert pos.sum() > 4000
    assert res.max() <= RESIDUAL
    if shift == 0.0:
        assert 4 * res.max() <= RESIDUAL < 4 * res.max() + 1        # four times what is observed here, no more


# ---- the prune's margin chain ---------------------------------------------------------------------------------

def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def _fit_like(rng, tris, kind):
    """a fit transform as the build makes them, as float32: the vertices' image lies in [0, 1]^3. kind 0: the plain fit
    (diagonal); kind 1: a rotation; kind 2: rotate-and-scale with condition number up to 16 (ray_axis's range), the image scaled
    uniformly into the unit cube"""
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


def _grazing_sweeps(rng, tris, scale, per):
    """`per` sweeps for each triangle that graze it or miss it by a few ulps of the radius: past a vertex (the line passes the
    vertex at the radius), along an edge (the line passes the edge's line at the radius, above a point of the edge) and onto
    the face at a shallow angle (the path ends where the sphere touches an interior point); the radius moved by -8 .. 8 ulps"""
    t = np.repeat(tris.astype(D), per, axis=0)
    n = t.shape[0]
    kind = rng.randint(0, 3, n)
    w = rng.uniform(0.05, 1, (n, 3))
    w[kind == 0] = np.eye(3)[rng.randint(0, 3, (kind == 0).sum())]
    edge = rng.randint(0, 3, n)
    w[(kind == 1), edge[kind == 1]] = 0
    w /= w.sum(axis=1, keepdims=True)
    q = (t * w[:, :, None]).sum(axis=1)
    e = np.take_along_axis(t, ((edge + 2) % 3)[:, None, None], 1)[:, 0] - np.take_along_axis(t, ((edge + 1) % 3)[:, None, None], 1)[:, 0]
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    r = 10.0 ** rng.uniform(-3, -0.3, n) * scale
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    perp = np.cross(d, rng.normal(size=(n, 3)))                                   # a vertex: any offset across the path
    perp[kind == 1] = np.cross(d, e)[kind == 1]                                    # an edge: across the path and the edge
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    back = 10.0 ** rng.uniform(-2, 0.5, n) * scale                                 # how far before the closest approach it starts
    o = q + perp * r[:, None] - d * back[:, None]
    # the face: the direction dips into the plane at an angle of 1e-3 .. 0.3, the centre ends r above q
    f = kind == 2
    inplane = np.cross(nrm, rng.normal(size=(n, 3)))
    inplane /= np.linalg.norm(inplane, axis=1, keepdims=True)
    dip = 10.0 ** rng.uniform(-3, -0.5, n)
    side = np.where(rng.uniform(size=n) < 0.5, 1.0, -1.0)
    df = inplane * np.cos(dip)[:, None] - nrm * (side * np.sin(dip))[:, None]
    d[f] = df[f]
    o[f] = (q + nrm * (side * r)[:, None] - df * back[:, None])[f]
    r32 = r.astype(F)
    r32 = (r32 + rng.randint(-8, 9, n) * np.spacing(r32)).astype(F)
    return np.repeat(tris, per, axis=0), o.astype(F), normalize3(d.astype(F)), r32, kind


def _fmaf(a, b, c):
    return (a.astype(D) * b.astype(D) + c.astype(D)).astype(F)       # (the product is exact in float64; one more rounding of the sum)


def _chain_figures(M, tris, o, d, r):
    """For pairs (triangle i, sweep i) under the fit transform M: which count (float32 sweep_tri, no tmax), per normalised axis
    how far the exact image of c(t) lies outside the triangle's exact image box beyond the sphere's share W r -- or, where that
    is less, the image W (dist - r) of the contact's residual, which an unluckier direction would put there --, the slack granted
    for that, and whether sweep.hip's float32 slab test keeps the unpadded box with the limit at t"""
    v0, e1, e2 = PQ._split(tris)
    t, _, _ = SQ.sweep_tri(v0, e1, e2, o, d, r)
    counts = np.isfinite(t)
    Md = M.astype(D)
    V = np.stack([v0.astype(D), v0.astype(D) + e1, v0.astype(D) + e2], axis=-2)
    img = V @ Md[:, :3].T + Md[:, 3]
    bmin, bmax = img.min(axis=-2), img.max(axis=-2)
    tt = np.where(counts, t, 0).astype(D)
    y = (o.astype(D) + tt[:, None] * d.astype(D)) @ Md[:, :3].T + Md[:, 3]
    W = np.abs(Md[:, :3]).sum(axis=1)
    S = (np.abs(o.astype(D))[:, None, :] * np.abs(Md[:, :3])).sum(-1) + np.abs(Md[:, 3])
    Wr = W * r.astype(D)[:, None]
    observed = np.maximum(bmin - y, y - bmax) - Wr                     # what the slack has to cover (negative: nothing) ...
    resid = np.maximum(SQ.distance_f64(v0, e1, e2, o.astype(D) + tt[:, None] * d.astype(D)) - r.astype(D), 0)
    observed = np.maximum(observed, W * resid[:, None])                # ... and at least the image of the residual (step 2 to 3)
    # the slack less the roundings it shares the grant with: the image's P (4 operations on S), H's own sum (3 on H)
    H = (2 + S) * 2.0 ** -16 * 33 + Wr * (1 + 2.0 ** -11)
    granted = 2.0 ** -11 * (2 + S + Wr) - EPS * (4 * S + 3 * H)
    # sweep_axis and slab in float32, as sweep.hip computes them
    inv, nlo, nhi = SQ.sweep_axis(M, o, d, r)
    lo32, hi32 = np.nextafter(bmin.astype(F), F(np.inf)), np.nextafter(bmax.astype(F), F(-np.inf))   # inside the exact box: smaller
    lo32, hi32 = np.minimum(lo32, hi32), np.maximum(lo32, hi32)
    a, b = _fmaf(lo32, inv, nlo), _fmaf(hi32, inv, nhi)
    near, far = np.minimum(a, b).max(axis=1), np.maximum(a, b).min(axis=1)
    kept = ~(near > far) & ~(near > t) & ~(far < 0)
    need = 4 * RESIDUAL * W * _unit(v0, e1, e2, o, r)[:, None]         # four times the asserted residual bound, its image
    return counts, observed, granted, kept, need


def test_prune_margin_chain_keeps_every_candidate_that_counts():
    """DESIGN.md 4.17's chain in float64, over plain, rotating and rotate-and-scale (condition number up to 16) fit transforms,
    seven decades of size, random sweeps and sweeps that graze a vertex, an edge and a face within -8 .. 8 ulps of the radius:
    for every pair that counts, on every normalised axis, the exact image of c(t) lies outside the triangle's exact image box
    (no leaf padding at all) by at most W r plus a quarter of the slack granted, the slack covers four times the image of the
    asserted residual bound, and the float32 slab test with the limit at t keeps that box"""
    rng = np.random.RandomState(5)
    worst, cover, total, conds, grazes = -1.0, 0.0, 0, [], np.zeros(3, int)
    for mag in range(-3, 4):
        scale = 10.0 ** mag
        for kind in (0, 1, 2):
            c = rng.uniform(-1, 1, (250, 1, 3))
            tris = ((c + rng.uniform(-0.2, 0.2, (250, 3, 3)) * rng.uniform(0.02, 1, (250, 1, 1))) * scale).astype(F)
            M = _fit_like(rng, tris, kind)
            conds.append(np.linalg.cond(M[:, :3].astype(D)))
            k = rng.randint(0, 250, 4000)
            o = (rng.uniform(-2, 2, (4000, 3)) * scale).astype(F)
            d = normalize3(((c[k, 0] + rng.uniform(-0.3, 0.3, (4000, 3))) * scale - o).astype(F))
            pairs = [(tris[k], o, d, (10.0 ** rng.uniform(-3, -0.3, 4000) * scale).astype(F), None)]
            pairs.append(_grazing_sweeps(rng, tris, scale, 16))
            for t, o, d, r, feature in pairs:
                counts, observed, granted, kept, need = _chain_figures(M, t, o, d, r)
                assert counts.sum() > 300 and (~counts).sum() > 100, (mag, kind, counts.sum())
                assert (granted > 0).all() and (need <= granted).all(), (mag, kind, (need / granted).max())
                cover = max(cover, (need / granted).max())
                ratio = (observed / granted)[counts].max()
                assert ratio <= 0.25, (mag, kind, ratio)
                assert kept[counts].all(), (mag, kind)
                worst = max(worst, ratio)
                total += counts.sum()
                if feature is not None:
                    grazes += np.bincount(feature[counts], minlength=3)
    print("pairs that count: %d (grazing a vertex / an edge / a face: %s); the largest observed / granted slack: %.3g; "
          "four times the asserted residual bound / granted: %.3g; condition numbers up to %.1f" % (total, grazes, worst, cover, max(conds)))
    assert max(conds) > 12 and total > 40000 and (grazes > 2000).all()


# ---- the contract's cases ------------------------------------------------------------------------------------------------------

TRI = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], F)      # in the plane z = 0; every sweep below is exact in float32


def _one(tri, o, d, r, tmax=np.inf):
    v0, e1, e2 = PQ._split(np.asarray(tri, F).reshape(1, 3, 3))
    t, u, v = SQ.sweep_tri(v0, e1, e2, np.asarray(o, F).reshape(1, 3), normalize3(np.asarray(d, F).reshape(1, 3)), F(r), F(tmax))
    return float(t[0]), float(u[0]), float(v[0])


def test_contract_features_and_closedness_on_exact_cases():
    assert _one(TRI, [0.25, 0.25, 2], [0, 0, -1], 0.5) == (1.5, 0.25, 0.25)                   # the face
    assert _one(TRI, [0.25, 0.25, -2], [0, 0, 3], 0.5) == (1.5, 0.25, 0.25)                   # ... from below, any length of d
    assert _one(TRI, [-2, -2, 0], [1, 1, 0], 0.25) == (pytest.approx(2 * np.sqrt(2) - 0.25, rel=1e-6), 0.0, 0.0)   # vertex v0 (d rounds)
    assert _one(TRI, [0.25, 0.25, 2], [0, 0, -1], 0.0) == (2.0, 0.25, 0.25)                   # radius 0: a ray
    assert _one(TRI, [1, 0, 2], [0, 0, -1], 0.0) == (2.0, 1.0, 0.0) and _one(TRI, [0.5, 0.5, 2], [0, 0, -1], 0.0) == (2.0, 0.5, 0.5)   # ... closed
    assert _one(TRI, [1.125, 0, 2], [0, 0, -1], 0.0)[0] == np.inf
    assert _one(TRI, [0.5, -2, 0], [0, 1, 0], 0.5) == (1.5, 0.5, 0.0)                         # the edge v0 v1
    assert _one(TRI, [-2, 0.5, 0], [1, 0, 0], 0.5) == (1.5, 0.0, 0.5)                         # the edge v0 v2
    t, u, v = _one(TRI, [2, 2, 0], [-1, -1, 0], 0.5)                                          # the edge v1 v2 (d rounds)
    assert (t, u, v) == (pytest.approx(1.5 * np.sqrt(2) - 0.5, rel=1e-6), pytest.approx(0.5, abs=1e-6), pytest.approx(0.5, abs=1e-6))
    assert _one(TRI, [3, 0, 0], [-1, 0, 0], 0.5) == (1.5, 1.0, 0.0)                           # vertex v1
    assert _one(TRI, [0, 3, 0], [0, -1, 0], 0.5) == (1.5, 0.0, 1.0)                           # vertex v2
    assert _one(TRI, [0.25, 0.25, 2], [0, 0, 1], 0.5)[0] == np.inf                            # moving away
    assert _one(TRI, [0.25, 0.25, 0.25], [0, 0, 1], 0.5) == (0.0, 0.25, 0.25)                 # touching at the start: t = 0, the closest point
    assert _one(TRI, [0.25, 0.25, 0.5], [1, 0, 0], 0.5) == (0.0, 0.25, 0.25)                  # ... exactly at the radius (closed)
    assert _one(TRI, [0.25, 0.25, 0.625], [1, 0, 0], 0.5)[0] == np.inf                        # sliding past above the plane
    # closed at tmax: a sweep that ends exactly at contact hits, one float shorter misses
    for o, d, r in (([0.25, 0.25, 2], [0, 0, -1], 0.5), ([0.5, -2, 0], [0, 1, 0], 0.5), ([3, 0, 0], [-1, 0, 0], 0.5)):
        t = _one(TRI, o, d, r)[0]
        assert _one(TRI, o, d, r, t)[0] == t and _one(TRI, o, d, r, np.nextafter(F(t), F(0)))[0] == np.inf
    assert _one(TRI, [0.25, 0.25, 0.25], [0, 0, 1], 0.5, 0.0)[0] == 0.0                       # tmax = 0: the start alone


def test_contract_start_is_the_within_query_and_closedness_on_a_soup():
    """t == 0 iff the point queries' model counts the triangle within (o, r); every hit is kept by tmax = t and lost (or, at
    t = 0, unchanged) by the float before it; radius 0 and the invalid queries"""
    rng = np.random.RandomState(7)
    c = rng.uniform(-1, 1, (300, 1, 3))
    tris = (c + rng.uniform(-0.2, 0.2, (300, 3, 3))).astype(F)
    cand = rng.permutation(300)[:280]
    n = 600
    o = rng.uniform(-1.5, 1.5, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)
    r = (10 ** rng.uniform(-2.5, -0.3, n)).astype(F)
    r[:40] = 0
    tm = np.full(n, np.inf, F)
    o[40, 0], d[41, 1], o[42, 2], d[43] = np.nan, np.inf, -np.inf, 0
    r[44], r[45], r[46], tm[47], tm[48] = np.nan, -1, np.inf, np.nan, -1e-3
    hits, any_ = SQ.query(tris, cand, o, d, r, tm)
    t, tri = hits[:, 2], hits.view(np.int32)[:, 3]
    assert not any_[40:49].any() and (tri[40:49] == -1).all() and np.isinf(t[40:49]).all()
    assert np.array_equal(any_, np.isfinite(t)) and np.array_equal(any_, tri >= 0) and np.isin(tri[any_], cand).all()
    assert 50 < any_.sum() < n - 50 and any_[:40].any() and (t == 0).sum() > 20
    within = PQ.query(tris, cand, o, r)[1]
    valid = SQ.sweep_valid(o, normalize3(d), r, tm)
    assert np.array_equal(t == 0, within & valid)
    same, _ = SQ.query(tris, cand, o, d, r, np.where(any_, t, tm))                     # tmax = t: the same record
    assert np.array_equal(same.view(np.uint32), hits.view(np.uint32))
    before, _ = SQ.query(tris, cand, o, d, r, np.where(any_ & (t > 0), np.nextafter(t, F(0)), np.where(any_, t, tm)))
    gone = any_ & (t > 0)
    assert np.isinf(before[gone, 2]).all() and np.array_equal(before[~gone].view(np.uint32), hits[~gone].view(np.uint32))


def test_contract_degenerate_triangles_and_ties():
    """two equal vertices in each position, a collinear triangle, a point: finite, deterministic, and what geometry says of a
    segment or a point in float64; two coincident triangles tie and the lower id wins"""
    rng = np.random.RandomState(8)
    n = 4000
    a, b = rng.randint(-8, 9, (n, 3)), rng.randint(-3, 4, (n, 3))
    b[(b == 0).all(axis=1)] = [1, 0, 0]
    k = rng.randint(2, 4, (n, 1))
    two_equal = np.stack([a, a, a + b], axis=1)
    collinear = np.stack([a, a + b, a + k * b], axis=1)
    point = np.stack([a, a, a], axis=1)
    o = rng.uniform(-2, 2, (n, 3)).astype(F)
    d = normalize3(((a / 8.0 + rng.uniform(-0.3, 0.3, (n, 3))) - o).astype(F))
    r = (10 ** rng.uniform(-2, -0.5, n)).astype(F)
    for tris, ends in ((two_equal, (a, a + b)), (two_equal[:, [2, 0, 1]], (a, a + b)), (two_equal[:, [0, 2, 1]], (a, a + b)),
                       (collinear, (a, a + k * b)), (point, (a, a))):
        v0, e1, e2 = PQ._split((tris / 8.0).astype(F))
        t, u, v = SQ.sweep_tri(v0, e1, e2, o, d, r)
        assert not np.isnan(t).any() and not np.isnan(u).any() and not np.isnan(v).any()
        # the same shape as a sliver of a triangle whose third vertex is the first: its float64 reading by definition
        p, q = (x / 8.0 for x in ends)
        td, fmin = SQ.first_contact_by_definition(p, q - p, np.zeros_like(p), o, d, r, 10.0)
        clear = np.abs(fmin) > 1e-5
        assert np.array_equal(np.isfinite(t)[clear], np.isfinite(td)[clear]) and clear.mean() > 0.99
        both = np.isfinite(t) & np.isfinite(td) & clear
        assert both.sum() > 500 and np.abs(t[both] - td[both]).max() < 1e-4
        c = (v0 + u[:, None] * e1) + v[:, None] * e2                                # the contact point lies on the segment
        gap = np.linalg.norm((o.astype(D) + t[:, None].astype(D) * d) - c, axis=1)[both & (t > 0)] - r[both & (t > 0)]
        assert np.abs(gap).max() < 1e-4
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    tris = np.stack([tri + F(5), tri, tri, tri + F(5)])
    for cand, want in (([0, 1, 2, 3], 1), ([3, 2, 0], 2)):
        hits, _ = SQ.query(tris, cand, [[0.25, 0.25, 2], [0.5, -2, 0]], [[0, 0, -1], [0, 1, 0]], 0.5)
        assert list(hits.view(np.int32)[:, 3]) == [want, want] and list(hits[:, 2]) == [1.5, 1.5]


# ---- the library, the headers, the kernels ---------------------------------------------------------------------------------------

SWEEP_ENTRIES = ("psm_bvh_sweep_sphere_dev", "psm_bvh_sweep_occluded_dev")


def test_library_exports_the_sweep_queries(psm):
    lib = psm.lib()
    header = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    for s in SWEEP_ENTRIES:
        assert hasattr(lib, s) and s in psm.EXPORTS and re.search(r"\b%s\(" % s, header), s
    assert re.search(r"float origin\[3\], radius;\s+float direct\[3\], tmax;\s+} psm_sweep_query;", header)
    assert psm.SWEEP_QUERY_DT.itemsize == 32 == psm.QUERY_RAY_DT.itemsize and psm.SWEEP_QUERY_DT.names == ("origin", "radius", "direct", "tmax")
    assert "sweep queries against a built hierarchy" in header and header.index("sweep queries against") > header.index("box queries against")
    for m in ("sweepSphere", "sweepOccluded"):
        assert callable(getattr(psm.TriangleHierarchy, m)), m
        for other in (psm.QueryScene, psm.InstancedScene, psm.InstanceWorld):               # a single hierarchy's only
            assert not hasattr(other, m), (other, m)
    hpp = open(os.path.join(ROOT, "include", "Prismarine", "TriangleHierarchy.hpp")).read()
    inl = open(os.path.join(ROOT, "include", "Prismarine", "TriangleHierarchy.inl")).read()
    for m, s in zip(("sweepSphere", "sweepOccluded"), SWEEP_ENTRIES):
        assert re.search(r"int %s\(const psm_sweep_query \*" % m, hpp) and "TriangleHierarchy::%s(" % m in inl and s + "(bvh," in inl
    dev = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "psm_query_dev.h")).read()
    assert "int sweep_launch(psm_ctx* c, bool any, uint32_t grid, const QueryArgs& a);" in dev


def test_sweep_refusals_without_a_hierarchy(psm):
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for fn in (lib.psm_bvh_sweep_sphere_dev, lib.psm_bvh_sweep_occluded_dev):   # no hierarchy: refused before anything is touched
        assert fn(None, p, ctypes.c_size_t(1), p) == -1
        assert fn(None, None, ctypes.c_size_t(0), None) == -1
    assert not any(buf)

    class NoCall:   # the Python layer refuses mismatched arguments before any call: a hierarchy that cannot make one
        ctx = None
        _scene = False

        def _launch_np(self, packed, out, name, *extra):
            raise AssertionError("a launch was made: %s %s %s" % (packed.shape, out, name))
        _query = psm.TriangleHierarchy._query
        sweepSphere = psm.TriangleHierarchy.sweepSphere
        sweepOccluded = psm.TriangleHierarchy.sweepOccluded
    o = np.zeros((3, 3), F)
    for call in (NoCall().sweepSphere, NoCall().sweepOccluded):
        with pytest.raises(ValueError, match="3 against 2"):
            call(o, o[:2], 0.5)
        with pytest.raises(ValueError):
            call(o, o, np.zeros(2, F))                      # a radius per sweep: [n]
        with pytest.raises(ValueError):
            call(o, o, 0.5, np.zeros(4, F))
        with pytest.raises(TypeError):
            call(o, o)                                      # the radius has no default
    with pytest.raises(AssertionError, match=r"\(3, 8\) hits psm_bvh_sweep_sphere_dev"):
        NoCall().sweepSphere(o, o, np.ones(3, F), 2.0)
    with pytest.raises(AssertionError, match=r"\(3, 8\) bool psm_bvh_sweep_occluded_dev"):
        NoCall().sweepOccluded(o, o, 0.25)


# The VGPRs and SGPRs each kernel reaches with the Makefile's flags, as ceilings (hipcc's figures for this code), and the LDS it
# declares (the 16-entry stack). __launch_bounds__(64, 6): the leaf test holds closest_on_tri and seven features' operands; at
# (64, 8) -- 64 VGPRs -- the compiler spills 38 / 17 registers to scratch, at 80 it spills nothing and 6 waves per SIMD stay
# open.
SWEEP_REGS = {"bvh_query_sweep": (80, 96), "bvh_query_sweep_any": (80, 96)}


def test_sweep_kernels_codegen():
    asm = csrc_asm("sweep.hip")
    assert asm.count(".amdhsa_kernel ") == 2
    for name, (vgprs, sgprs) in SWEEP_REGS.items():
        blk, body = kernel_asm(asm, "_ZN3psm%d%sENS_9QueryArgsE" % (len(name), name))

        def meta(key):
            return kernel_meta(blk, key)
        assert meta("vgpr_count") <= vgprs <= 80, (name, meta("vgpr_count"))          # 80: six waves per SIMD
        assert meta("sgpr_count") <= sgprs, (name, meta("sgpr_count"))
        assert meta("vgpr_spill_count") == 0 and meta("sgpr_spill_count") == 0, name
        assert meta("private_segment_fixed_size") == 0 and "scratch_" not in body, name
        assert "v_writelane_b32" not in body, name                            # no SGPR parked in a VGPR lane either
        assert meta("group_segment_fixed_size") == 16 * 64 * 4, name          # the stack
        assert "v_fma_mix_f32" in body, name                                  # the slab planes straight from the fp16 record
        assert "v_sqrt_f32" in body and "v_div_scale_f32" in body, name       # correctly rounded division and square root


def test_sweep_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "sweep_query_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "sweep_query_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)


def _host_pairs():
    """lattice, soup, soup moved by 1000, starts at contact, grazing: v0, e1, e2, o, d, r"""
    rng = np.random.RandomState(9)
    n = 4000
    a = rng.randint(-8, 9, (n, 1, 3))
    lat = (np.clip(a + rng.randint(-2, 3, (n, 3, 3)), -8, 8) / 8.0).astype(F)
    axes = np.concatenate([np.eye(3), -np.eye(3), [[1, 1, 0], [0, -1, 1], [1, 1, 1], [-1, 1, -1]]])
    sets = [PQ._split(lat) + ((rng.randint(-16, 17, (n, 3)) / 8.0).astype(F), normalize3(axes[rng.randint(0, 10, n)].astype(F)),
                              (rng.randint(0, 9, n) / 16.0).astype(F))]
    sets += [_soup(3, n), _soup(3, n, 1000.0), _from_contact(3, n), _at_radius(3, n)]
    c = rng.uniform(-1, 1, (n // 16, 1, 3))
    tris = (c + rng.uniform(-0.2, 0.2, (n // 16, 3, 3))).astype(F)
    t, o, d, r, _ = _grazing_sweeps(rng, tris, 1.0, 16)
    sets.append(PQ._split(t) + (o, d, r))
    return tuple(np.concatenate([s[k] for s in sets]) for k in range(6))


def test_kernel_sweep_tri_on_the_host_is_the_model_bit_for_bit(tmp_path):
    """psm_sweep_dev.h itself as a stand-alone host program with its own main, built with -ffp-contract=off and the address and
    undefined-behaviour sanitizers and run as a process of its own on the CPU: t, u, v of every pair bit for bit the model's"""
    hipcc = "/opt/rocm/bin/hipcc"
    exe, fin, fout = (str(tmp_path / x) for x in ("sweep_tri_host", "pairs.bin", "out.bin"))
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "prismarine-core_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sweep_tri_host.cpp"), "-o", exe])
    v0, e1, e2, o, d, r = _host_pairs()
    cu, cv, d2 = PQ.closest_on_tris(v0, e1, e2, o)
    rec = np.concatenate([v0, e1, e2, o, d, r[:, None], d2[:, None], cu[:, None], cv[:, None]], axis=1).astype(F)
    assert rec.shape[1] == 19
    rec.tofile(fin)
    done = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode(errors="replace")
    got = np.fromfile(fout, F).reshape(-1, 3)
    t, u, v, feat = SQ.sweep_tri(v0, e1, e2, o, d, r, feature=True)
    want = np.stack([t, u, v], axis=1)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    assert got.shape == want.shape and bad.size == 0, "%d differ, first %d: %s against %s" % (bad.size, bad[0], got[bad[0]], want[bad[0]])
    assert (np.bincount(feat + 1, minlength=9) > 50).all(), np.bincount(feat + 1, minlength=9)    # the start, every feature, misses
    assert ((feat >= 0) & (feat < 7) & (t == 0)).sum() > 100                                       # and features that found the start touching
    # sweep_axis, the prune's set-up: rows of plain, rotating and rotate-and-scale fit transforms over six decades of size
    rng = np.random.RandomState(10)
    rows, oo, dd, rr = [], [], [], []
    for mag in range(-3, 4):
        for kind in (0, 1, 2):
            scale = 10.0 ** mag
            tris = (rng.uniform(-1.2, 1.2, (50, 3, 3)) * scale).astype(F)
            M = _fit_like(rng, tris, kind)
            k = rng.randint(0, 3, 300)
            rows.append(M[k])
            oo.append((rng.uniform(-2, 2, (300, 3)) * scale).astype(F))
            dd.append(normalize3(rng.normal(size=(300, 3)).astype(F)))
            rr.append((10.0 ** rng.uniform(-3, -0.3, 300) * scale).astype(F))
    rows, oo, dd, rr = (np.concatenate(x) for x in (rows, oo, dd, rr))
    dd[::50, 0] = 0                                                                                  # directions along a plane: the 1e-20 rule
    np.concatenate([rows, oo, dd, rr[:, None]], axis=1).astype(F).tofile(fin)
    done = subprocess.run([exe, fin, fout, "axis"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode(errors="replace")
    got = np.fromfile(fout, F).reshape(-1, 3)
    want = np.stack([np.stack(SQ.sweep_axis(np.stack([rows[i]] * 3), oo[i:i + 1], dd[i:i + 1], rr[i:i + 1]), axis=-1)[0, 0] for i in range(rows.shape[0])])
    assert got.shape == want.shape == (6300, 3) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
