"""CPU tests (no GPU) of the point queries (psm_bvh_closest_point_dev / psm_bvh_within_dev, query.hip): the numpy model the GPU
tests hold the kernels to (tests/point_query_model.py) against a float64 second reading by a different method, its finiteness on
degenerate triangles, the library's new exports, the kernels' code generation and the header layer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import point_query_model as PQ
import query_model as Q
from util import check_query_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EPS = 2.0 ** -24
# The model against a float64 reading, per pair: |dist - dist64| <= 1e-6 (|p - v0| + |e1| + |e2|) + shape * L, L the longest edge,
# s the sine of the angle at v0 (s^2 = det / (aa bb), det = aa bb - ab^2, in float64), by the model's own face / sliver decision:
#   face (float32 det > 2^-16 aa bb): shape = 8 eps / s^2 -- det rounds by ~14 eps aa bb and the barycentrics carry it (the point
#     moves in the plane; measured <= 3.5 eps / s^2 L);
#   sliver: shape = s -- the triangle lies within its width (<= s L) of its longest edge, the clamped projection it is taken as
#     (measured <= 0.82 s L).
# Well-shaped triangles: 1e-6 of the scale. Near the threshold s = 2^-8 the two meet: up to ~2^-7 L measured (5.3e-3 L), 2^-5 L
# by the bound; a collinear or zero-area triangle (s = 0) is its segment again to 1e-6 of the scale.
TOL = 1e-6


def _model_dist(tris, p):
    v0, e1, e2 = PQ._split(tris)
    u, v, d2 = PQ.closest_on_tris(v0[None], e1[None], e2[None], np.asarray(p, F)[:, None, :])
    return u, v, np.sqrt(d2)


def _scale(tris, p):
    t = np.asarray(tris, np.float64)
    return (np.linalg.norm(np.asarray(p, np.float64)[:, None, :] - t[None, :, 0], axis=-1)
            + np.linalg.norm(t[:, 1] - t[:, 0], axis=-1)[None] + np.linalg.norm(t[:, 2] - t[:, 0], axis=-1)[None])


def _shape(tris):
    """per triangle: (longest edge L, s, the model's face decision)"""
    t = np.asarray(tris, np.float64)
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    aa, ab, bb = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
    with np.errstate(all="ignore"):
        s = np.sqrt(np.clip(np.where(aa * bb > 0, (aa * bb - ab * ab) / (aa * bb), 0.0), 0.0, 1.0))
    L = np.linalg.norm(np.stack([e1, e2, e2 - e1], 1), axis=-1).max(1)
    _, f1, f2 = PQ._split(tris)
    faa, fab, fbb = Q.dot3(f1, f1), Q.dot3(f1, f2), Q.dot3(f2, f2)
    face = (faa * fbb - fab * fab) > faa * fbb * PQ.SLIVER
    return L, s, face


def _tolerance(tris, p):
    """[R, T]: the stated bound (above) for every point against every triangle"""
    L, s, face = _shape(tris)
    with np.errstate(divide="ignore"):
        shape = np.where(face, 8 * EPS / np.maximum(s, 1e-30) ** 2, s)
    return TOL * _scale(tris, p) + (shape * L)[None]


def _slivers(rng, n, angles):
    """needles (two long legs at v0, a small angle between them) and caps (v0 inside the long edge: an angle near 180 degrees),
    unit-ish size, random orientation and vertex order, at the angles given; one point per triangle in its plane inside it or
    off the plane by 1e-4 .. 0.3"""
    ang = np.repeat(np.asarray(angles, np.float64), n) * rng.uniform(0.8, 1.2, n * len(angles))
    m = ang.size
    l1, l2 = rng.uniform(0.3, 1.5, m), rng.uniform(0.3, 1.5, m)
    loc = np.zeros((m, 3, 3))
    loc[:, 1, 0] = l1
    cap = rng.rand(m) < 0.3
    loc[:, 2, 0] = np.where(cap, -l2 * np.cos(ang), l2 * np.cos(ang))
    loc[:, 2, 1] = l2 * np.sin(ang)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    t = loc @ q.T + rng.uniform(-2, 2, (m, 1, 3))
    t = np.take_along_axis(t, np.array([rng.permutation(3) for _ in range(m)])[:, :, None], 1)
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    z = rng.choice([0.0, 0.0, 1e-4, 1e-2, 0.3], (m, 1)) * rng.choice([-1.0, 1.0], (m, 1))
    p = np.einsum("ij,ijk->ik", rng.dirichlet([1, 1, 1], m), t) + nrm * z
    return t.astype(F), p.astype(F)


def _adversarial(rng):
    """triangles and points that cover every region of Ericson's test, points on vertices, edges and the plane, and degenerate
    triangles: slivers of several widths, exactly and nearly collinear, two or three equal vertices. Returns (tris, points,
    targets): targets[i] = the triangle point i was placed on or near (-1: a point of the random cloud)."""
    base = rng.uniform(-1, 1, (40, 3, 3)).astype(F)
    tris = [base]
    a, b = rng.uniform(-1, 1, (40, 3)), rng.uniform(-1, 1, (40, 3))
    for w in (1e-1, 1e-2, 1e-3, 1e-5, 1e-7, 0.0):                                          # slivers and collinear (rounded)
        c = a + rng.uniform(-0.5, 1.5, (40, 1)) * (b - a) + w * rng.normal(size=(40, 3))
        tris.append(np.stack([a, b, c], 1).astype(F))
    ai, di = rng.randint(-3, 4, (40, 3)), rng.randint(-2, 3, (40, 3))                         # exactly collinear, small integers
    k = rng.randint(-2, 3, (40, 2))
    tris.append(np.stack([ai, ai + k[:, :1] * di, ai + k[:, 1:] * di], 1).astype(F))
    tris += [np.stack(x, 1).astype(F) for x in ((ai, ai, ai + di), (ai, ai + di, ai), (ai + di, ai, ai), (ai, ai, ai))]
    tris = np.concatenate(tris)
    t = base
    ids = np.arange(40)
    pts, tgt = [rng.uniform(-2, 2, (200, 3)).astype(F)], [np.full(200, -1)]
    pts.append(t.reshape(-1, 3))                                                                # on the vertices
    tgt.append(np.repeat(ids, 3))
    s = rng.uniform(0, 1, (40, 1)).astype(F)
    pts += [t[:, 0] + s * (t[:, 1] - t[:, 0]), t[:, 0] + s * (t[:, 2] - t[:, 0]), t[:, 1] + s * (t[:, 2] - t[:, 1])]   # edges
    tgt += [ids] * 3
    uv = rng.dirichlet([1, 1, 1], 40).astype(F)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    pts.append(np.einsum("ij,ijk->ik", uv, t))                                                  # in the plane, inside
    pts.append(np.einsum("ij,ijk->ik", uv, t) + n * rng.uniform(-1, 1, (40, 1)))               # above the face
    pts.append(np.einsum("ij,ijk->ik", (uv * 3 - 1), t))                                        # in the plane, outside
    tgt += [ids] * 3
    # every sliver, collinear and zero-area triangle: a point in its plane inside it, and one slightly off the plane
    deg = tris[40:].astype(np.float64)
    w = rng.dirichlet([1, 1, 1], deg.shape[0])
    inside = np.einsum("ij,ijk->ik", w, deg)
    nd = np.cross(deg[:, 1] - deg[:, 0], deg[:, 2] - deg[:, 0])
    with np.errstate(all="ignore"):
        nd = np.where(np.linalg.norm(nd, axis=1, keepdims=True) > 0, nd / np.linalg.norm(nd, axis=1, keepdims=True), 0.0)
    pts += [inside.astype(F), (inside + nd * rng.uniform(-1e-2, 1e-2, (deg.shape[0], 1))).astype(F)]
    tgt += [40 + np.arange(deg.shape[0])] * 2
    return tris, np.concatenate(pts).astype(F), np.concatenate(tgt)


def test_model_against_float64_random_triangles():
    rng = np.random.RandomState(1)
    tris = rng.uniform(-1, 1, (300, 3, 3)).astype(F)
    p = rng.uniform(-2, 2, (300, 3)).astype(F)
    _, _, d = _model_dist(tris, p)
    ref = PQ.closest_f64(tris, p)
    assert (np.abs(d - ref) <= TOL * _scale(tris, p)).all(), np.max(np.abs(d - ref) / _scale(tris, p))


def test_model_against_float64_adversarial():
    rng = np.random.RandomState(2)
    tris, p, tgt = _adversarial(rng)
    u, v, d = _model_dist(tris, p)
    assert np.isfinite(d).all() and np.isfinite(u).all() and np.isfinite(v).all()
    assert (u >= 0).all() and (v >= 0).all() and (u <= 1).all() and (v <= 1).all()
    ref = PQ.closest_f64(tris, p)
    tol = _tolerance(tris, p)
    assert (np.abs(d - ref) <= tol).all(), np.unravel_index(np.argmax(np.abs(d - ref) - tol), d.shape)
    # the points placed on the degenerate triangles reach them: in or near the plane of a sliver, where the bound is its own
    on = np.nonzero(tgt >= 40)[0]
    err = np.abs(d[on, tgt[on]] - ref[on, tgt[on]])
    assert on.size == 2 * (tris.shape[0] - 40) and (err <= tol[on, tgt[on]]).all()
    # the chosen triangle is as near as the float64 minimum over all triangles, to the chosen and the nearest one's bounds
    k = np.argmin(d, axis=1)
    r = np.arange(p.shape[0])
    j = np.argmin(ref, axis=1)
    assert (d[r, k] <= ref[r, j] + tol[r, j]).all() and (d[r, k] >= ref[r, k] - tol[r, k]).all()


def test_model_regions_on_targeted_points():
    """Each point placed on a vertex, an edge or the face of a well-shaped triangle lands, against that triangle, in the region
    it was placed in, at the distance it has there"""
    rng = np.random.RandomState(2)
    tris, p, tgt = _adversarial(rng)
    sel = np.nonzero((tgt >= 0) & (tgt < 40))[0]
    v0, e1, e2 = PQ._split(tris[tgt[sel]])
    u, v, d2 = PQ.closest_on_tris(v0, e1, e2, p[sel])
    d = np.sqrt(d2.astype(np.float64))
    ref = np.array([PQ.closest_f64(tris[tgt[i]:tgt[i] + 1], p[i:i + 1])[0, 0] for i in sel])
    scale = _scale(tris[tgt[sel]], p[sel]).diagonal()
    assert (np.abs(d - ref) <= TOL * scale).all()
    vert = slice(0, 120)
    e_1, e_2, e_12, face, above = (slice(120 + 40 * i, 160 + 40 * i) for i in range(5))
    corner = np.tile(np.array([[0, 0], [1, 0], [0, 1]], F), (40, 1))
    assert np.array_equal(np.c_[u[vert], v[vert]], corner)                                 # vertices: exactly that vertex,
    assert (d[vert] <= 1e-6 * scale[vert]).all()                                            # at distance ~0 (v0 + e1 rounds)
    # edges: on the edge (a point placed there in float32 lies a rounding off it, so the face may take it: the barycentric off the
    # edge is then a rounding away from 0), at distance ~0
    for sl, off_edge in ((e_1, v[e_1]), (e_2, u[e_2]), (e_12, np.abs(u[e_12] + v[e_12] - 1))):
        assert (off_edge <= 1e-5).all() and (d[sl] <= 1e-6 * scale[sl]).all()
    for sl in (face, above):                                                                # the face: inside it
        assert ((u[sl] > 0) & (v[sl] > 0) & (u[sl] + v[sl] < 1)).all()
    assert (d[face] <= 1e-6 * scale[face]).all()


def test_model_sliver_threshold_sweep():
    """Needles and caps whose angle at v0 runs across the 2^-16 face threshold, points in and near their plane: the stated
    bound holds, and its largest value, near the threshold, is ~2^-7 of the longest edge"""
    rng = np.random.RandomState(8)
    tris, p = _slivers(rng, 60, np.geomspace(1e-6, 0.5, 40))
    v0, e1, e2 = PQ._split(tris)
    u, v, d2 = PQ.closest_on_tris(v0, e1, e2, p)
    d = np.sqrt(d2.astype(np.float64))
    ref = np.array([PQ.closest_f64(tris[i:i + 1], p[i:i + 1])[0, 0] for i in range(p.shape[0])])
    L, s, face = _shape(tris)
    tol = np.diagonal(_tolerance(tris, p))
    err = np.abs(d - ref)
    assert (err <= tol).all(), (err - tol).max()
    assert face.any() and (~face).any()
    assert (err / L).max() <= 2.0 ** -6
    assert (err[s > 0.2] <= TOL * np.diagonal(_scale(tris, p))[s > 0.2]).all()   # well-shaped again away from the threshold


def test_model_degenerates_are_finite_everywhere():
    """Every degenerate kind against points all around it, near and far: finite u, v, dist"""
    rng = np.random.RandomState(3)
    tris, _, _ = _adversarial(rng)
    tris = tris[40:]
    p = np.concatenate([rng.uniform(-4, 4, (300, 3)), rng.uniform(-1e4, 1e4, (50, 3)), tris.reshape(-1, 3)[:200]]).astype(F)
    u, v, d = _model_dist(tris, p)
    assert np.isfinite(u).all() and np.isfinite(v).all() and np.isfinite(d).all()


def test_point_of_reproduces_the_distance():
    """(tri, u, v) of a result give back the point whose distance the query reports, bit for bit"""
    rng = np.random.RandomState(4)
    tris = rng.uniform(-1, 1, (64, 3, 3)).astype(F)
    p = rng.uniform(-1.5, 1.5, (500, 3)).astype(F)
    hits, within = PQ.query(tris, np.arange(64), p)
    assert within.all()
    tri = hits.view(np.int32)[:, 3]
    c = PQ.point_of(tris, tri, hits[:, 0], hits[:, 1])
    dp = p - c
    d2 = (dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1]) + dp[:, 2] * dp[:, 2]
    assert np.array_equal(np.sqrt(d2).view(np.uint32), hits[:, 2].view(np.uint32))


def test_query_model_rmax_ties_and_invalid():
    """dist <= rmax counts; a bit-equal d2 goes to the lowest id; NaN / negative rmax and non-finite points miss"""
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], F)
    tris = np.concatenate([tri, tri, tri + F([0, 0, 2])])
    p = np.array([[0.25, 0.25, 1]] * 6 + [[np.nan, 0, 0], [np.inf, 0, 0]], F)
    rmax = np.array([np.inf, 1, np.nextafter(F(1), F(0)), 0, -1, np.nan, np.inf, np.inf], F)
    hits, within = PQ.query(tris, [2, 1, 0], p, rmax)
    assert list(hits.view(np.int32)[:, 3]) == [0, 0, -1, -1, -1, -1, -1, -1]
    assert list(within) == [True, True, False, False, False, False, False, False]
    assert hits[0, 2] == 1 and np.isinf(hits[2, 2]) and hits[2, 0] == 0
    hits, _ = PQ.query(tris, [1, 2], p[:1])   # candidates are the leaves: triangle 0 is not one
    assert hits.view(np.int32)[0, 3] == 1
    hits, _ = PQ.query(tris, [2, 1, 0], np.array([[0.25, 0.25, 1]], F), F(-0.0))   # -0 is 0: nothing is at distance 0
    assert hits.view(np.int32)[0, 3] == -1


def test_library_exports_the_point_queries(psm):
    lib = psm.lib()
    for s in ("psm_bvh_closest_point_dev", "psm_bvh_within_dev"):
        assert hasattr(lib, s) and s in psm.EXPORTS
    assert psm.POINT_QUERY_DT.itemsize == 16


def test_point_queries_reject_null_without_device(psm):
    if psm.lib().psm_device_count() > 0:
        pytest.skip("a GPU is present")
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    for fn in (lib.psm_bvh_closest_point_dev, lib.psm_bvh_within_dev):
        assert fn(None, ctypes.cast(buf, ctypes.c_void_p), ctypes.c_size_t(1), ctypes.cast(buf, ctypes.c_void_p)) == -1
        assert fn(None, None, ctypes.c_size_t(0), None) == -1


def test_point_query_kernels_codegen():
    """the two point kernels, and the ray kernels still at their ceilings"""
    check_query_kernels(["bvh_query_point", "bvh_query_within", "bvh_query_closest", "bvh_query_any"])


def test_point_query_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "point_query_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "point_query_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)
