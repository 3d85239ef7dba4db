"""The scene queries on the GPU (psm_scene_*_dev, query.hip; QueryScene): all seven queries over several hierarchies at once.
The yardsticks are tests/scene_query_model.py over each hierarchy's own leaves (PSM_BVH_LEAF_TRI) and the numpy combination of
the single-hierarchy queries' own answers. Every comparison is exact: floats by their bits, ids, counts and votes as integers."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import inside_query_model as IQ
import query_model as Q
import ray_prune_model as RP
import scene_query_model as SQ
from test_gpu_fuzz import fuzz_case
from test_gpu_inside_query import _scene_points
from test_gpu_point_query import ROT_SCALE, SHEAR
from test_gpu_point_query import _hier as _hier_opt
from test_gpu_query import _camera_rays, _hier, _leaves, _nonfinite, _random_rays, _windows

try:   # (imported before the library loads its HIP runtime, as tests/test_gpu_query.py)
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu
# (a package without the scene queries has no such name: this module then does not import)
MAX_GEOMETRIES = importlib.import_module("prismarine-core_amd").SCENE_MAX_GEOMETRIES

F = np.float32
U = np.uint32


class _Scene:
    """hierarchies over the parts of a mesh, the scene over them, and the model's geometries (tris, leaves)"""

    def __init__(self, psm, ctx, parts, opts=None):
        self.psm, self.parts = psm, [np.ascontiguousarray(t, F).reshape(-1, 3, 3) for t in parts]
        self.ths = [_hier(psm, ctx, t) for t in self.parts] if opts is None else [_hier_opt(psm, ctx, t, m) for t, m in zip(self.parts, opts)]
        self.scene = psm.QueryScene(ctx, self.ths)

    def geoms(self):
        return [(t, _leaves(self.psm, th)) for t, th in zip(self.parts, self.ths)]

    def close(self):
        for th in self.ths:
            th.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype.itemsize == exp.dtype.itemsize, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    if got.dtype.itemsize == 4:   # floats by their bits
        got, exp = got.view(U), exp.view(U)
    bad = np.nonzero((got != exp).reshape(got.shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, (what, bad.size, bad[:4], got[bad[:4]], exp[bad[:4]])


def _check_rays(sc, o, d, tmin=0.0, tmax=np.inf):
    """intersect, occluded, countHits of the scene: the scene model's, and the combination of every hierarchy's own answers"""
    o = np.ascontiguousarray(o, F).reshape(-1, 3)
    d = np.ascontiguousarray(d, F).reshape(-1, 3)
    n = o.shape[0]
    lo = np.broadcast_to(np.asarray(tmin, F), (n,)).copy()
    hi = np.broadcast_to(np.asarray(tmax, F), (n,)).copy()
    geoms = sc.geoms()
    got, occ, cnt = sc.scene.intersect(o, d, lo, hi), sc.scene.occluded(o, d, lo, hi), sc.scene.countHits(o, d, lo, hi)
    assert got.geom.dtype == np.int32 and got.geom.shape == (n,) and occ.dtype == np.bool_ and cnt.dtype == np.uint32
    exp, egeom, eany = SQ.intersect(geoms, o, d, lo, hi)
    _same(got.buffer, exp, "intersect")
    _same(got.geom, egeom, "intersect geom")
    _same(occ, eany, "occluded")
    _same(cnt, SQ.count(geoms, o, d, lo, hi), "countHits")
    own, ogeom = SQ.combine_closest([th.intersect(o, d, lo, hi).buffer for th in sc.ths])
    _same(got.buffer, own, "intersect against the hierarchies' own")
    _same(got.geom, ogeom, "geom against the hierarchies' own")
    _same(occ, np.logical_or.reduce([th.occluded(o, d, lo, hi) for th in sc.ths]), "occluded against the hierarchies' own")
    _same(cnt, np.sum([th.countHits(o, d, lo, hi) for th in sc.ths], axis=0, dtype=np.uint32), "countHits against the hierarchies' own")
    return got


def _check_points(sc, p, rmax=np.inf, samples=(1, 3, 5)):
    """closestPoint, within, inside, signedDistance of the scene: the scene model's, and the combination of every hierarchy's own"""
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    rm = np.broadcast_to(np.asarray(rmax, F), (p.shape[0],)).copy()
    geoms = sc.geoms()
    got, wi = sc.scene.closestPoint(p, rm), sc.scene.within(p, rm)
    exp, egeom, ewi = SQ.closest_point(geoms, p, rm)
    _same(got.buffer, exp, "closestPoint")
    _same(got.geom, egeom, "closestPoint geom")
    _same(wi, ewi, "within")
    own, ogeom = SQ.combine_points(geoms, p, [th.closestPoint(p, rm).buffer for th in sc.ths])
    _same(got.buffer, own, "closestPoint against the hierarchies' own")
    _same(got.geom, ogeom, "geom against the hierarchies' own")
    _same(wi, np.logical_or.reduce([th.within(p, rm) for th in sc.ths]), "within against the hierarchies' own")
    par = SQ.parities(geoms, p, max(samples))
    dirs = IQ.INSIDE_DIRECTIONS
    out = {}
    for s in samples:
        ins = sc.scene.inside(p, s)
        assert ins.dtype == np.bool_
        _same(ins, IQ.vote(par, s), "inside %d" % s)
        # ... and from the hierarchies' own hit counts of the same rays: the parity of the sum, then the vote
        own_par = np.array([(np.sum([th.countHits(p, np.broadcast_to(dirs[k], p.shape)) for th in sc.ths], axis=0) & 1) == 1 for k in range(s)])
        _same(ins, IQ.vote(own_par, s), "inside %d against the hierarchies' own counts" % s)
        sd = sc.scene.signedDistance(p, rm, s)
        esd = exp.copy()
        esd.view(U)[(egeom >= 0) & ins, 2] |= U(0x80000000)
        _same(sd.buffer, esd, "signedDistance %d" % s)
        _same(sd.geom, egeom, "signedDistance geom")
        out[s] = ins
    k = min(p.shape[0], 1024)
    msd, mgeom = SQ.signed_distance(geoms, p[:k], rm[:k], samples[-1])
    sd = sc.scene.signedDistance(p[:k], rm[:k], samples[-1])
    _same(sd.buffer, msd, "signedDistance against the model's own statement")
    _same(sd.geom, mgeom, "signedDistance geom")
    return out


def _all_cases(sc, tris, o, d, seed):
    rng = np.random.RandomState(seed)
    got = _check_rays(sc, o, d)
    _check_rays(sc, o, d, -np.inf, np.inf)
    _check_rays(sc, *_random_rays(rng, tris, 384))
    _check_rays(sc, *_random_rays(rng, tris, 384, outside=True))
    tmin, tmax = _windows(rng, got.t.copy(), o.shape[0])
    _check_rays(sc, o, d, tmin, tmax)
    miss = _check_rays(sc, *_nonfinite(o[:64], d[:64]))
    assert (miss.geom[:6] == -1).all()
    p = _scene_points(rng, tris, 512)
    _check_points(sc, p)
    diag = float(np.linalg.norm(tris.reshape(-1, 3).max(0) - tris.reshape(-1, 3).min(0)))
    r = rng.uniform(0, 0.05 * diag, p.shape[0]).astype(F)
    r[:8] = [np.inf, 0, -0.0, -1, np.nan, np.inf, 0, -1]
    _check_points(sc, p, r, samples=(3,))
    return got


# how a mesh of n triangles is cut into 2, 3 and 8 consecutive parts of unequal size, one of them a single triangle
def _sizes(n, parts):
    if parts == 2:
        return (max(1, n // 3),)
    if parts == 3:
        return (1, max(1, n // 4))
    w = np.array([5, 1, 9, 2, 14, 3, 7], np.float64)
    s = np.maximum(1, (w / w.sum() * n * 0.8).astype(np.int64))
    s[1] = 1
    return tuple(int(x) for x in s)


@pytest.mark.parametrize("parts", [2, 3, 8])
def test_scene_sponza_like(psm, ctx, oracle, scenes, parts):
    sm = scenes.sponza_like(30011)
    tris = sm["tris"].reshape(-1, 3, 3)
    o, d = _camera_rays(oracle, scenes, sm, 32, 18)
    pieces, _ = SQ.split(tris, _sizes(tris.shape[0], parts))
    assert len(pieces) == parts and (parts == 2 or min(t.shape[0] for t in pieces) == 1)   # (3 and 8: with a one-triangle part)
    with _Scene(psm, ctx, pieces) as sc:
        got = _all_cases(sc, tris, o, d, 40 + parts)
        assert len(set(got.geom[got.geom >= 0])) >= 2


@pytest.mark.parametrize("opt", [ROT_SCALE, SHEAR], ids=["rotate_scale", "shear"])
def test_a_member_built_with_an_optimisation_matrix(psm, ctx, oracle, scenes, opt):
    """One of three members built with a matrix: the file's yardsticks, bit for bit, on the rays that are fully well-posed in
    every member and on the points whose vote rays all are (tests/ray_prune_model.py: the contract of the other rays is the
    single hierarchy's, tests/test_gpu_ray_matrix.py); at most 1 % of the rays and of the points are left out"""
    sm = scenes.sponza_like(3001)
    tris = sm["tris"].reshape(-1, 3, 3)
    pieces, _ = SQ.split(tris, _sizes(tris.shape[0], 3))
    with _Scene(psm, ctx, pieces, [None, opt, None]) as sc:
        t = np.array(sc.ths[1].info().transform).reshape(4, 4)[:3, :3]
        assert np.abs(t - np.diag(np.diag(t))).max() > 0.01

        members = [(tr, _leaves(psm, th), np.array(th.info().transform, F), None) for tr, th in zip(sc.parts, sc.ths)]
        rng = np.random.RandomState(61)
        oo, od = _camera_rays(oracle, scenes, sm, 32, 16)
        rays = RP.ray_classes(rng, tris, oo, od, 512)
        o, d = (np.concatenate([rays[c][k] for c in ("own", "random", "outside", "tilt1e-3", "tilt1e-5")]) for k in (0, 1))
        keep = RP.fully_well_posed(members, o, d)
        assert (~keep).sum() <= 0.01 * keep.size, int((~keep).sum())
        o, d = o[keep], d[keep]
        got = _check_rays(sc, o, d)
        assert (got.geom == 1).sum() > 50 and (got.geom == 2).sum() > 50   # (the member with the matrix is hit, and another)
        _check_rays(sc, o, d, *_windows(rng, got.t.copy(), o.shape[0]))
        p = _scene_points(rng, tris, 512)
        sure = RP.vote_rays_well_posed(members, p, IQ.INSIDE_DIRECTIONS)
        assert (~sure).sum() <= 0.01 * sure.size, int((~sure).sum())
        _check_points(sc, p[sure])
        _check_points(sc, p[sure], rng.uniform(0, 2.0, int(sure.sum())).astype(F), samples=(3,))


@pytest.mark.parametrize("seed,parts", [(0, 2), (1, 3), (2, 8), (3, 3), (4, 2), (5, 8), (6, 3), (7, 2)])
def test_scene_fuzz_soups(psm, ctx, seed, parts):
    tris, o, d, _ = fuzz_case(seed)
    if tris.shape[0] < parts:   # a soup of fewer triangles than parts: repeated, so that every part has one
        tris = np.concatenate([tris] * parts)
    pieces, _ = SQ.split(tris, _sizes(tris.shape[0], parts))
    assert len(pieces) == parts
    with _Scene(psm, ctx, pieces) as sc:
        _all_cases(sc, tris, o[:192], d[:192], 300 + seed)


def _merged_cases(psm, ctx, tris, sizes, o, d, p, rmax):
    """(b): a single hierarchy over the concatenated triangles gives the scene's answers, ids by the part's offset -- where no
    build drops a triangle, which is asserted for every hierarchy involved"""
    pieces, offs = SQ.split(tris, sizes)
    with _Scene(psm, ctx, pieces) as sc:
        whole = _hier(psm, ctx, tris)
        try:
            for th, t in zip(sc.ths + [whole], pieces + [tris]):
                assert th.info().leaf_count == t.shape[0] == th.triangleCount
            rng = np.random.RandomState(77)
            exact = whole.intersect(o, d)
            for lo, hi in ((0.0, np.inf), _windows(rng, exact.t.copy(), o.shape[0])):
                got = sc.scene.intersect(o, d, lo, hi)
                _same(SQ.merged_ids(got.buffer, got.geom, offs), whole.intersect(o, d, lo, hi).buffer, "merged intersect")
                _same(sc.scene.occluded(o, d, lo, hi), whole.occluded(o, d, lo, hi), "merged occluded")
                _same(sc.scene.countHits(o, d, lo, hi), whole.countHits(o, d, lo, hi), "merged countHits")
            assert (got.geom >= 0).any()
            for rm in (np.inf, rmax):
                got = sc.scene.closestPoint(p, rm)
                _same(SQ.merged_ids(got.buffer, got.geom, offs), whole.closestPoint(p, rm).buffer, "merged closestPoint")
                _same(sc.scene.within(p, rm), whole.within(p, rm), "merged within")
                for s in (1, 3, 5):
                    _same(sc.scene.inside(p, s), whole.inside(p, s), "merged inside")
                    sd = sc.scene.signedDistance(p, rm, s)
                    _same(SQ.merged_ids(sd.buffer, sd.geom, offs), whole.signedDistance(p, rm, s).buffer, "merged signedDistance")
        finally:
            whole.close()


@pytest.mark.parametrize("mesh", ["icosphere", "torus", "sponza_coarse"])
def test_scene_equals_the_merged_hierarchy(psm, ctx, scenes, mesh):
    rng = np.random.RandomState(8)
    if mesh == "sponza_coarse":
        tris = scenes.sponza_like(3000)["tris"].reshape(-1, 3, 3)
    else:
        tris = IQ.icosphere(3) if mesh == "icosphere" else IQ.torus()
    n = tris.shape[0]
    o, d = _random_rays(rng, tris, 1024)
    p = _scene_points(rng, tris, 1024)
    diag = float(np.linalg.norm(tris.reshape(-1, 3).max(0) - tris.reshape(-1, 3).min(0)))
    r = rng.uniform(0, 0.1 * diag, p.shape[0]).astype(F)
    _merged_cases(psm, ctx, tris, (n // 5, n // 2), o, d, p, r)


@functools.lru_cache(maxsize=None)
def _cases():
    return IQ.geometry_cases()


@pytest.mark.parametrize("case,sizes", [(0, (400,)), (0, (100, 700)), (1, (1000,)), (1, (300, 1500)), (3, (1280,)), (3, (640, 800)),
                                        (4, (1280,))],
                         ids=["icosphere2", "icosphere3", "torus2", "torus3", "shell_by_body", "shell3", "shell_flipped_by_body"])
def test_inside_closed_surfaces_split_across_geometries(psm, ctx, case, sizes):
    """(c): a closed surface cut by triangle index into two or three geometries. inside with 3 and 5 rays is the analytic answer on
    every seeded point (no mismatch allowed, as for the unsplit surface); the sign of the distance is that answer; and inside of
    every single part differs from it somewhere -- what is tested is the parity summed over the geometries."""
    name, tris, p, truth, clearance, gap = _cases()[case]
    assert gap < clearance
    pieces, _ = SQ.split(tris, sizes)
    assert len(pieces) == len(sizes) + 1
    with _Scene(psm, ctx, pieces) as sc:
        for th, t in zip(sc.ths, pieces):
            assert th.info().leaf_count == t.shape[0]
        for s in (3, 5):
            ins = sc.scene.inside(p, s)
            bad = np.nonzero(ins != truth)[0]
            assert bad.size == 0, (name, s, bad.size, p[bad[:4]])
            sd = sc.scene.signedDistance(p, samples=s)
            assert (sd.geom >= 0).all() and np.array_equal(np.signbit(sd.t), truth)
            for th in sc.ths:
                assert (th.inside(p, s) != truth).any()
        band = sc.scene.signedDistance(p, rmax=F(0.05))
        near = band.geom >= 0
        assert near.any() and (~near).any() and np.array_equal(np.signbit(band.t[near]), truth[near])
        assert np.array_equal(band.tri >= 0, near) and np.isposinf(band.t[~near]).all()
        _check_points(sc, p[:1500], samples=(1, 3, 5))


def test_the_same_hierarchy_twice_answers_with_geometry_zero(psm, ctx, scenes):
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3)
    th = _hier(psm, ctx, tris)
    try:
        rng = np.random.RandomState(5)
        o, d = _random_rays(rng, tris, 2048)
        for k in (2, MAX_GEOMETRIES):
            scene = psm.QueryScene(ctx, [th] * k)
            got, one = scene.intersect(o, d), th.intersect(o, d)
            _same(got.buffer, one.buffer, "twice: intersect")
            assert (got.tri >= 0).sum() > 500 and np.array_equal(got.geom, np.where(one.tri >= 0, 0, -1))
            pg, p1 = scene.closestPoint(o), th.closestPoint(o)
            _same(pg.buffer, p1.buffer, "twice: closestPoint")
            assert (pg.geom == 0).all()
            _same(scene.countHits(o, d), (k * th.countHits(o, d)).astype(np.uint32), "twice: countHits")
            assert not scene.inside(o, 3).any()          # every crossing counted an even number of times
            _same(scene.occluded(o, d), th.occluded(o, d), "twice: occluded")
    finally:
        th.close()


def test_coplanar_duplicates_and_mirrored_parts_on_the_gpu(psm, ctx):
    """the tie cases of the CPU test through the kernels: the same triangle in two geometries (the lower geometry wins whatever
    the ids), mirror images with a bit-equal d2"""
    t = np.array([[[-1, -1, 1], [1, -1, 1], [0, 1, 1]]], F)
    rng = np.random.RandomState(8)
    far = ((rng.uniform(-1, 1, (7, 1, 3)) + rng.uniform(-0.25, 0.25, (7, 3, 3))) + [0, 0, 5]).astype(F)
    a, b = np.concatenate([far, t]), np.concatenate([t, far[:1], t])
    o = np.concatenate([np.zeros((1, 3), F), rng.uniform(-0.3, 0.3, (255, 3)).astype(F) * F([1, 1, 0])])
    d = np.tile(F([0, 0, 1]), (256, 1))
    for parts, tri in (((a, b), 7), ((b, a), 0)):
        with _Scene(psm, ctx, parts) as sc:
            got = _check_rays(sc, o, d)
            assert (got.geom == 0).all() and (got.tri == tri).all()
            pg = sc.scene.closestPoint(o)
            assert (pg.geom == 0).all() and (pg.tri == tri).all()
            _check_points(sc, o, samples=(3,))
    m = np.array([[[0.5, -1, -1], [0.5, 1, -1], [0.75, 0, 1]]], F)
    p = rng.uniform(-1, 1, (256, 3)).astype(F) * F([0, 1, 1])
    for parts in ((m, m * F([-1, 1, 1])), (m * F([-1, 1, 1]), m)):
        with _Scene(psm, ctx, parts) as sc:
            _check_points(sc, p, samples=(3,))
            assert (sc.scene.closestPoint(p).geom == 0).all()


def test_scene_after_refit_and_rebuild_of_one_geometry(psm, ctx):
    """(d): one geometry refitted, then rebuilt with other triangles (and reallocated: a new native handle), the others untouched;
    the scene object is the same throughout"""
    outer, inner = IQ.icosphere(3), IQ.icosphere(2, 0.5)
    rng = np.random.RandomState(21)
    p = rng.uniform(-1.2, 1.2, (2000, 3)).astype(F)
    o, d = p[:1024], rng.normal(size=(1024, 3)).astype(F)
    rad = np.linalg.norm(p.astype(np.float64), axis=1)
    with _Scene(psm, ctx, [outer, inner]) as sc:
        _check_rays(sc, o, d)
        ins = _check_points(sc, p, samples=(3,))[3]
        clear = (np.abs(rad - 1.0) > 0.02) & (np.abs(rad - 0.5) > 0.02)
        assert np.array_equal(ins[clear], ((rad < 1.0) & (rad > 0.5))[clear])
        moved = (inner * F(0.8)).astype(F)              # within the build's bounds
        sc.ths[1].clearTribuffer()
        sc.ths[1].loadTriangles(moved.reshape(-1, 9))
        sc.ths[1].refit()
        sc.parts[1] = moved
        _check_rays(sc, o, d)
        ins = _check_points(sc, p, samples=(3,))[3]
        clear = (np.abs(rad - 1.0) > 0.02) & (np.abs(rad - 0.4) > 0.02)
        assert np.array_equal(ins[clear], ((rad < 1.0) & (rad > 0.4))[clear])
        other = (IQ.torus() * F(0.5)).astype(F)
        sc.ths[1].allocate(other.shape[0])
        sc.ths[1].loadTriangles(other.reshape(-1, 9))
        sc.ths[1].build()
        sc.parts[1] = other
        got = _check_rays(sc, o, d)
        assert (got.geom == 1).any() and (got.geom == 0).any()
        _check_points(sc, p, samples=(3,))


def test_scene_deep_geometry_beside_a_shallow_one(psm, ctx, scenes):
    """(e): the deep fixture (its walk leaves the 16 stack entries kept in LDS) as one geometry, before and after a shallow one: a
    small box across the row of clusters, its near face at x = 0.004 -- about half of the rays meet a cluster's triangle before
    it, the others the box first (tests/scene_query_model.py gives 141 against 115 of the 256)"""
    deep, o, d = Q.deep_fixture()
    box = (scenes.cornell()["tris"].reshape(-1, 3, 3) * F(0.002) + F([0.006, 0, 0])).astype(F)
    rng = np.random.RandomState(12)
    p = rng.normal(0, 1e-3, (256, 3)).astype(F)
    for parts in ((deep, box), (box, deep), (deep, box, deep)):
        with _Scene(psm, ctx, parts) as sc:
            got = _check_rays(sc, o, d)
            first_deep, first_box = [[k for k, t in enumerate(parts) if t is which][0] for which in (deep, box)]
            assert (got.geom >= 0).all() and (got.geom == first_deep).any() and (got.geom == first_box).any()
            assert set(got.geom.tolist()) == {first_deep, first_box}      # (deep, box, deep): the second copy of the deep one never wins
            _check_rays(sc, o, d, 0.25, 1.0)
            _check_points(sc, p, samples=(3,))
            assert sc.scene.countHits(o, d).max() >= 8


def test_scene_host_checks(psm, ctx):
    tri = np.eye(3, dtype=F).reshape(1, 9)
    built = _hier(psm, ctx, tri)
    unbuilt = psm.TriangleHierarchy(ctx)
    unbuilt.allocate(4)
    unbuilt.loadTriangles(tri)
    other_ctx = psm.Context(0)
    foreign = _hier(psm, other_ctx, tri)
    try:
        lib = psm.lib()
        h = ctx.buf_alloc(256)
        p = ctx.buf_ptr(h)[0]
        P, one, zero, three, u32 = ctypes.c_void_p, ctypes.c_size_t(1), ctypes.c_size_t(0), ctypes.c_uint32(3), ctypes.c_uint32
        err = lambda: lib.psm_last_error(ctx._h).decode()

        def lst(*ths):
            return (ctypes.c_void_p * len(ths))(*[t._h if t is not None else None for t in ths])

        for n in (one, zero):   # the list is checked for n = 0 too
            assert lib.psm_scene_intersect_dev(lst(built, None), u32(2), P(p), n, P(p), P(p + 64)) == -1
            assert err() == "psm_scene_intersect_dev: geometry 1 is NULL"
            assert lib.psm_scene_within_dev(lst(None, built), u32(2), P(p), n, P(p)) == -1
            assert err() == "psm_scene_within_dev: geometry 0 is NULL"
            assert lib.psm_scene_count_hits_dev(lst(built, built, foreign), u32(3), P(p), n, P(p)) == -1
            assert err() == "psm_scene_count_hits_dev: geometry 2 belongs to another context"
            assert lib.psm_scene_inside_dev(lst(built, unbuilt), u32(2), P(p), n, three, P(p)) == -5
            assert err() == "psm_scene_inside_dev: geometry 1 is not built"
            assert lib.psm_scene_occluded_dev(lst(built), u32(0), P(p), n, P(p)) == -1
            assert lib.psm_scene_occluded_dev((ctypes.c_void_p * 33)(*[built._h] * 33), u32(33), P(p), n, P(p)) == -1
        g = lst(built, built)
        assert lib.psm_scene_intersect_dev(g, u32(2), None, zero, None, None) == 0           # n = 0: no data is touched
        assert lib.psm_scene_intersect_dev(g, u32(2), None, one, P(p), P(p + 64)) == -1
        assert lib.psm_scene_intersect_dev(g, u32(2), P(p), one, None, P(p + 64)) == -1
        assert lib.psm_scene_intersect_dev(g, u32(2), P(p), one, P(p + 32), None) == -1      # geom must not be NULL
        assert err() == "psm_scene_intersect_dev: NULL pointer"
        assert lib.psm_scene_intersect_dev(g, u32(2), P(p), one, P(p + 32), P(p + 66)) == -1
        assert err() == "psm_scene_intersect_dev: geom not 4-byte aligned"
        assert lib.psm_scene_closest_point_dev(g, u32(2), P(p), one, P(p + 36), P(p + 64)) == -1
        assert err() == "psm_scene_closest_point_dev: points or hits not 16-byte aligned"
        assert lib.psm_scene_count_hits_dev(g, u32(2), P(p), one, P(p + 34)) == -1
        assert err() == "psm_scene_count_hits_dev: counts not 4-byte aligned"
        for s in (0, 2, 4, 6):
            assert lib.psm_scene_inside_dev(g, u32(2), P(p), one, u32(s), P(p + 64)) == -1
            assert lib.psm_scene_signed_distance_dev(g, u32(2), P(p), one, u32(s), P(p + 32), P(p + 64)) == -1
        assert err() == "psm_scene_signed_distance_dev: samples must be 1, 3 or 5"
        assert lib.psm_scene_signed_distance_dev(g, u32(2), P(p), one, three, P(p + 32), P(p + 68)) == 0
        ctx.sync()
        ctx.buf_free(h)
        with pytest.raises(psm.PsmError, match="geometry 1 is not built"):
            psm.QueryScene(ctx, [built, unbuilt]).occluded(np.zeros((2, 3), F), np.ones((2, 3), F))
        empty = psm.QueryScene(ctx, [built, built]).intersect(np.zeros((0, 3), F), np.zeros((0, 3), F))
        assert len(empty) == 0 and empty.geom.shape == (0,) and empty.geom.dtype == np.int32
    finally:
        foreign.close()
        other_ctx.close()
        unbuilt.close()
        built.close()


def test_scene_torch_tensors_on_a_non_default_stream(psm, ctx):
    if torch is None:
        pytest.skip("torch is not installed")
    parts, _ = SQ.split(IQ.torus(), (500, 1000))
    rng = np.random.RandomState(6)
    p = rng.uniform([-1.6, -1.6, -0.6], [1.6, 1.6, 0.6], (4099, 3)).astype(F)
    p[-1] = [np.nan, 0, 0]
    o, d = p, rng.normal(size=p.shape).astype(F)
    tmin = rng.uniform(-1, 0.5, p.shape[0]).astype(F)
    r = rng.uniform(0, 0.3, p.shape[0]).astype(F)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        own = psm.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        try:
            for c in (own, ctx):     # a context on torch's (non-default) current stream, and one with a stream of its own
                with _Scene(psm, c, parts) as sc:
                    to, td, tt, tr = (torch.from_numpy(x).to(dev) for x in (o, d, tmin, r))
                    got, ref = sc.scene.intersect(to, td, tt), sc.scene.intersect(o, d, tmin)
                    assert got.buffer.device == dev and got.geom.device == dev and got.geom.dtype == torch.int32
                    _same(got.buffer.cpu().numpy(), ref.buffer, "torch intersect")
                    _same(got.geom.cpu().numpy(), ref.geom, "torch geom")
                    assert (ref.geom >= 0).any()
                    _same(sc.scene.occluded(to, td, tt).cpu().numpy(), sc.scene.occluded(o, d, tmin), "torch occluded")
                    cnt = sc.scene.countHits(to, td, tt)
                    assert cnt.dtype == torch.int32
                    _same(cnt.cpu().numpy().view(np.uint32), sc.scene.countHits(o, d, tmin), "torch countHits")
                    cp, cref = sc.scene.closestPoint(to, tr), sc.scene.closestPoint(p, r)
                    _same(cp.buffer.cpu().numpy(), cref.buffer, "torch closestPoint")
                    _same(cp.geom.cpu().numpy(), cref.geom, "torch closestPoint geom")
                    _same(sc.scene.within(to, tr).cpu().numpy(), sc.scene.within(p, r), "torch within")
                    for s in (1, 3, 5):
                        ins = sc.scene.inside(to, s)
                        assert ins.dtype == torch.bool
                        _same(ins.cpu().numpy(), sc.scene.inside(p, s), "torch inside")
                        sd, sref = sc.scene.signedDistance(to, tr, s), sc.scene.signedDistance(p, r, s)
                        _same(sd.buffer.cpu().numpy(), sref.buffer, "torch signedDistance")
                        _same(sd.geom.cpu().numpy(), sref.geom, "torch signedDistance geom")
        finally:
            own.close()
    torch.cuda.synchronize()


def test_scene_query_captured_into_a_graph_and_replayed(psm, ctx):
    """a scene query captured on the context's stream after a first plain call (which allocates the context's stack area) and
    replayed: a linear graph of the one launch (signed distance: two); the replay answers as the plain call, also for inputs
    rewritten between the replays"""
    hip = psm._hip()
    parts, _ = SQ.split(IQ.icosphere(3), (300, 500))
    rng = np.random.RandomState(31)
    n = 3000
    with _Scene(psm, ctx, parts) as sc:
        lib = psm.lib()
        rays = np.zeros((n, 8), F)
        pts = np.zeros((n, 4), F)
        sizes = (rays.nbytes, pts.nbytes, 16 * n, 4 * n, 16 * n, 4 * n)
        hs = [ctx.buf_alloc(s) for s in sizes]
        ptr = [ctypes.c_void_p(ctx.buf_ptr(h)[0]) for h in hs]
        g = (ctypes.c_void_p * 3)(*[th._h for th in sc.ths])
        cn, three, u3 = ctypes.c_size_t(n), ctypes.c_uint32(3), ctypes.c_uint32(3)

        def launch():
            assert lib.psm_scene_intersect_dev(g, u3, ptr[0], cn, ptr[2], ptr[3]) == 0
            assert lib.psm_scene_signed_distance_dev(g, u3, ptr[1], cn, three, ptr[4], ptr[5]) == 0

        def fill():
            p = rng.uniform(-1.3, 1.3, (n, 3)).astype(F)
            rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = p, 0, rng.normal(size=(n, 3)), np.inf
            pts[:, 0:3], pts[:, 3] = p, np.inf
            ctx.buf_upload(hs[0], rays)
            ctx.buf_upload(hs[1], pts)
            return p

        def results():
            ctx.sync()
            return (ctx.buf_download(hs[2], F, 4 * n).reshape(n, 4), ctx.buf_download(hs[3], np.int32, n),
                    ctx.buf_download(hs[4], F, 4 * n).reshape(n, 4), ctx.buf_download(hs[5], np.int32, n))

        fill()
        launch()                      # the first plain call
        ctx.sync()
        stream = ctypes.c_void_p(ctx.stream)
        graph, exe = ctypes.c_void_p(), ctypes.c_void_p()
        assert hip.hipStreamBeginCapture(stream, ctypes.c_int(1)) == 0        # hipStreamCaptureModeThreadLocal
        try:
            launch()
        finally:
            rc = hip.hipStreamEndCapture(stream, ctypes.byref(graph))
        assert rc == 0 and graph.value
        nodes = ctypes.c_size_t(0)
        assert hip.hipGraphGetNodes(graph, None, ctypes.byref(nodes)) == 0 and nodes.value == 3    # one launch + two
        assert hip.hipGraphInstantiate(ctypes.byref(exe), graph, None, None, ctypes.c_size_t(0)) == 0
        try:
            for _ in range(2):
                p = fill()
                for h, size in zip(hs[2:], sizes[2:]):      # the outputs overwritten: what is read back is the replay's
                    ctx.buf_upload(h, np.full(size // 4, 0x7f, np.int32))
                assert hip.hipGraphLaunch(exe, stream) == 0
                rh, rg, sh, sg = results()
                eh, eg = sc.scene.intersect(p, rays[:, 4:7]), sc.scene.signedDistance(p)
                _same(rh, eh.buffer, "replayed intersect")
                _same(rg, eh.geom, "replayed geom")
                _same(sh, eg.buffer, "replayed signedDistance")
                _same(sg, eg.geom, "replayed signedDistance geom")
                assert (rg >= 0).any() and np.signbit(sh[:, 2]).any()
        finally:
            hip.hipGraphExecDestroy(exe)
            hip.hipGraphDestroy(graph)
            for h in hs:
                ctx.buf_free(h)
