"""The ray queries on the GPU under build (`optimization`) matrices and grazing rays (TriangleHierarchy.intersect / occluded /
countHits / firstHits / inside / signedDistance; query.hip, kbest.hip). The yardstick is the well-posed contract of
tests/ray_prune_model.py: bit for bit against the brute-force models on every fully well-posed ray, sound
two-sided bounds on the others, and a cap on how many rays the rule leaves to the bounds -- recomputed here from the transform
the GPU's own build reports. tests/test_ray_prune_cpu.py proves on the CPU that the prune cannot lose a well-posed hit."""
import functools

import numpy as np
import pytest

import inside_query_model as IQ
import query_model as Q
import ray_prune_model as RP
from test_gpu_fuzz import fuzz_opt
from test_gpu_point_query import ROT_SCALE, SHEAR, _hier, _leaves
from test_gpu_query import _camera_rays, _windows

pytestmark = pytest.mark.gpu

F = np.float32
N_RAYS = 2048
MATRICES = [("identity", None), ("rotate_scale", ROT_SCALE), ("shear", SHEAR)] + [
    ("fuzz_opt%d" % s, fuzz_opt(np.random.RandomState(5000 + s))) for s in range(4)]
SHAPES = ["sponza_like", "cornell", "deep", "tiny1", "tiny2", "tiny3"]


def _shape(name, oracle, scenes):
    """(tris, own origins, own directions): the smallest shapes that hold every case -- 3001 and 32 triangles with their camera's
    rays, the deep fixture (1344 triangles: the stack spills) with its own, and 1, 2 and 3 triangles (the lone-leaf path and the
    smallest trees) with rays aimed at them"""
    if name in ("sponza_like", "cornell"):
        sc = scenes.sponza_like(3001) if name == "sponza_like" else scenes.cornell()
        return (sc["tris"].reshape(-1, 3, 3),) + _camera_rays(oracle, scenes, sc, 64, 32)
    if name == "deep":
        return Q.deep_fixture(rays=N_RAYS)
    # (in no axis' plane: a scene without extent in an axis is stretched to the unit box along it, and so is the rounding of a hit)
    tri = np.array([[[1, -1, -1], [1.5, 1, -1], [0.8, 0, 1]]], F)
    tris = np.concatenate([tri, tri * F(0.5) + F([0.5, 0.2, 0]), tri[:, ::-1] + F([0.25, -0.3, 0.1])])[:int(name[4:])]
    rng = np.random.RandomState(4)
    o = rng.uniform(-0.5, 0.5, (N_RAYS, 3)).astype(F)
    return tris, o, (F([2, 0, 0]) + rng.uniform(-1, 1, (N_RAYS, 3)).astype(F) - o).astype(F)


@functools.lru_cache(maxsize=None)
def _cases(name, oracle, scenes):
    """a shape's triangles and, per class of rays, the rays and their accepted pairs (which depend on neither matrix nor window:
    computed once and shared by the matrices; nothing changes them)"""
    tris, oo, od = _shape(name, oracle, scenes)
    rng = np.random.RandomState(900 + SHAPES.index(name))
    return tris, {c: (o, d, RP.accepted_pairs(tris, o, d)) for c, (o, d) in RP.ray_classes(rng, tris, oo, od, N_RAYS).items()}


def _check_rays(psm, th, tris, o, d, pairs, tmin=0.0, tmax=np.inf):
    """every ray query of one batch against the contract; returns the batch's RaySets"""
    n = o.shape[0]
    lo = np.broadcast_to(np.asarray(tmin, F), (n,)).copy()
    hi = np.broadcast_to(np.asarray(tmax, F), (n,)).copy()
    S = RP.RaySets(tris, _leaves(psm, th), np.array(th.info().transform, F), o, d, lo, hi, pairs=pairs)
    RP.check_intersect(S, th.intersect(o, d, lo, hi).buffer)
    RP.check_occluded(S, th.occluded(o, d, lo, hi))
    RP.check_count(S, th.countHits(o, d, lo, hi))
    for k in (1, 4, 16):
        got = th.firstHits(o, d, k, lo, hi)
        RP.check_first_hits(S, k, got.buffer, got.count)
    return S


def _check_classes(psm, th, name, mname, tris, cases, seed):
    """all classes of rays with the default window (and the share caps) and with the window shrunk to the closest hit's own t on
    every ray that has one (the tightest window: the box must admit t itself, not merely overlap [0, inf)), then random per-ray
    windows -- tmin = tmax = an exact hit's t, empty, -inf, NaN -- on the shape's own rays and on the flattest tilted class"""
    for c, (o, d, pairs) in cases.items():
        S = _check_rays(psm, th, tris, o, d, pairs)
        t = S.closest()[:, 2]
        _check_rays(psm, th, tris, o, d, pairs, np.where(np.isfinite(t), t, F(0)), t)
        what = "%s %s %s" % (name, mname, c)
        if (name, c) in RP.NO_SHARE:   # (a class that is degenerate on this shape: listed there with its reason)
            pass
        elif c in RP.SHARE_CAP:
            RP.check_shares(S, RP.SHARE_CAP[c], what)
        elif name == "sponza_like":
            RP.check_shares(S, RP.FLAT_CAP[c], what, at_least=1)
        if c in ("own", "tilt1e-7"):
            rng = np.random.RandomState(seed)
            tmin, tmax = _windows(rng, S.closest()[:, 2].copy(), o.shape[0])
            _check_rays(psm, th, tris, o, d, pairs, tmin, tmax)
            _check_rays(psm, th, tris, o, d, pairs, -np.inf, np.inf)


@pytest.mark.parametrize("mname", [m for m, _ in MATRICES])
def test_ray_queries_under_a_build_matrix(psm, ctx, oracle, scenes, mname):
    opt = dict(MATRICES)[mname]
    for name in SHAPES:
        tris, cases = _cases(name, oracle, scenes)
        th = _hier(psm, ctx, tris, opt)
        try:
            assert name == "deep" or th.info().leaf_count == tris.shape[0]   # (deep: its smallest triangles are no leaves)
            _check_classes(psm, th, name, mname, tris, cases, 31 + SHAPES.index(name))
        finally:
            th.close()


def _closed_points(rng, tris, n):
    """points around a closed mesh: in its box grown by a tenth, on its surface, at its vertices; NaN / inf"""
    t = np.asarray(tris, F).reshape(-1, 3, 3)
    lo, hi = t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0)
    k = n // 8
    surf = np.einsum("ij,ijk->ik", rng.dirichlet([1, 1, 1], k).astype(F), t[rng.randint(0, t.shape[0], k)]).astype(F)
    vert = t.reshape(-1, 3)[rng.randint(0, 3 * t.shape[0], k)]
    p = np.concatenate([surf, vert, rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (n - 2 * k, 3))]).astype(F)
    p[-1], p[-2] = [np.nan, 0, 0], [0, np.inf, 0]
    return p


@functools.lru_cache(maxsize=None)
def _closed_case(which):
    """a closed mesh, points, and the accepted pairs of each point's five vote rays"""
    tris = IQ.icosphere(3) if which == "icosphere" else IQ.torus()
    p = _closed_points(np.random.RandomState(41), tris, N_RAYS)
    return tris, p, [RP.accepted_pairs(tris, p, np.broadcast_to(IQ.INSIDE_DIRECTIONS[k], p.shape)) for k in range(5)]


@pytest.mark.parametrize("mname", ["rotate_scale", "shear"])
def test_inside_and_signed_distance_under_a_build_matrix(psm, ctx, mname):
    """A point whose vote rays are all fully well-posed answers exactly as the model (the parity of |A| per ray, then the vote); for
    the other points only the vote and the sign are exempt: the unsigned part is closestPoint()'s record on every point"""
    for which in ("icosphere", "torus"):
        tris, p, pairs = _closed_case(which)
        th = _hier(psm, ctx, tris, dict(MATRICES)[mname])
        try:
            M, leaves = np.array(th.info().transform, F), _leaves(psm, th)
            sets = [RP.RaySets(tris, leaves, M, None, None, 0.0, np.inf, pairs=pr) for pr in pairs]
            par = np.stack([(S.nA & 1) == 1 for S in sets])
            plain = th.closestPoint(p)
            found = plain.tri >= 0
            for s in (1, 3, 5):
                sure = np.all([S.full for S in sets[:s]], axis=0)
                assert (~sure).sum() <= 0.01 * p.shape[0], (which, mname, s, int((~sure).sum()))
                exp_in = IQ.vote(par, s)
                got_in = th.inside(p, s)
                assert got_in.dtype == np.bool_ and np.array_equal(got_in[sure], exp_in[sure]), (which, mname, s)
                sd = th.signedDistance(p, np.inf, s)
                unsigned = sd.buffer.copy()
                unsigned.view(np.uint32)[found, 2] &= np.uint32(0x7FFFFFFF)
                assert np.array_equal(unsigned.view(np.uint32), plain.buffer.view(np.uint32)), (which, mname, s)
                assert np.array_equal(np.signbit(sd.t)[sure & found], exp_in[sure & found]), (which, mname, s)
                assert not np.signbit(sd.t)[~found].any()
            assert found[:-2].all() and par.any() and not par.all()
        finally:
            th.close()


@pytest.mark.parametrize("mname", ["rotate_scale", "shear"])
def test_ray_queries_after_refit_under_a_build_matrix(psm, ctx, oracle, scenes, mname):
    """triangles moved within the build's bounds and refitted: the transform is the build's, the answers are the moved triangles'"""
    sc = scenes.cornell()
    tris = sc["tris"].reshape(-1, 3, 3).copy()
    th = _hier(psm, ctx, tris, dict(MATRICES)[mname])
    try:
        before = np.array(th.info().transform, F)
        moved = tris.copy()
        rng = np.random.RandomState(9)
        k = rng.choice(tris.shape[0], 8, replace=False)
        c = moved[k].mean(axis=1, keepdims=True)
        moved[k] = (c + (moved[k] - c) * F(0.5)).astype(F)      # shrunk about their centres: inside their own old extent
        th.clearTribuffer()
        th.loadTriangles(moved.reshape(-1, 9))
        th.refit()
        assert np.array_equal(np.array(th.info().transform, F), before)
        oo, od = _camera_rays(oracle, scenes, sc, 64, 32)
        cases = {c: (o, d, RP.accepted_pairs(moved, o, d)) for c, (o, d) in RP.ray_classes(rng, moved, oo, od, N_RAYS).items()}
        _check_classes(psm, th, "cornell", mname, moved, cases, 57)
        assert np.isin(th.intersect(*cases["own"][:2]).tri, k).any()
    finally:
        th.close()
