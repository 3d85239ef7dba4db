"""The instanced scene queries on the GPU (psm_instances_*_dev, query.hip; InstancedScene): the seven queries over hierarchies
that each stand at a rigid pose. The yardstick is tests/instance_query_model.py over each hierarchy's own leaves
(PSM_BVH_LEAF_TRI): the canonical move in numpy float32, the single-hierarchy models, the scene's combination rules. Every
comparison with it is exact: floats by their bits, ids, counts and votes as integers."""
import ctypes
import functools

import numpy as np
import pytest

import inside_query_model as IQ
import instance_query_model as NQ
import query_model as Q
import ray_prune_model as RP
import scene_query_model as SQ
from test_gpu_fuzz import fuzz_case
from test_gpu_inside_query import _scene_points
from test_gpu_point_query import ROT_SCALE, SHEAR
from test_gpu_point_query import _hier as _hier_opt
from test_gpu_query import _camera_rays, _hier, _leaves, _nonfinite, _random_rays, _windows
from test_gpu_scene_query import _same, _sizes
from test_instance_query_cpu import BAKED_CASES

try:   # (imported before the library loads its HIP runtime, as tests/test_gpu_query.py)
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32


class _Inst:
    """hierarchies over meshes, an InstancedScene of (hierarchy index, pose) entries, and the model's instances"""

    def __init__(self, psm, ctx, meshes, entries, opts=None):
        self.psm, self.meshes = psm, [np.ascontiguousarray(t, F).reshape(-1, 3, 3) for t in meshes]
        self.ths = [_hier(psm, ctx, t) for t in self.meshes] if opts is None else [_hier_opt(psm, ctx, t, m) for t, m in zip(self.meshes, opts)]
        self.which = [k for k, _ in entries]
        self.scene = psm.InstancedScene(ctx, [(self.ths[k], m) for k, m in entries])

    def insts(self):
        leaves = [_leaves(self.psm, th) for th in self.ths]
        return [(self.meshes[k], leaves[k], m) for k, m in zip(self.which, self.scene.transforms())]

    def close(self):
        for th in self.ths:
            th.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _poses(seed, n, shift):
    """a seeded rotation (even entries) or reflection (odd entries) and a translation per entry"""
    rng = np.random.RandomState(seed)
    return [NQ.random_pose(rng, reflect=bool(k & 1), shift=shift) for k in range(n)]


def _check_rays(sc, o, d, tmin=0.0, tmax=np.inf):
    o = np.ascontiguousarray(o, F).reshape(-1, 3)
    d = np.ascontiguousarray(d, F).reshape(-1, 3)
    n = o.shape[0]
    lo = np.broadcast_to(np.asarray(tmin, F), (n,)).copy()
    hi = np.broadcast_to(np.asarray(tmax, F), (n,)).copy()
    insts = sc.insts()
    got, occ, cnt = sc.scene.intersect(o, d, lo, hi), sc.scene.occluded(o, d, lo, hi), sc.scene.countHits(o, d, lo, hi)
    assert got.geom.dtype == np.int32 and got.geom.shape == (n,) and occ.dtype == np.bool_ and cnt.dtype == np.uint32
    exp, einst, eany = NQ.intersect(insts, o, d, lo, hi)
    _same(got.buffer, exp, "intersect")
    _same(got.geom, einst, "intersect inst")
    _same(occ, eany, "occluded")
    _same(cnt, NQ.count(insts, o, d, lo, hi), "countHits")
    return got


def _check_points(sc, p, rmax=np.inf, samples=(1, 3, 5)):
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    rm = np.broadcast_to(np.asarray(rmax, F), (p.shape[0],)).copy()
    insts = sc.insts()
    got, wi = sc.scene.closestPoint(p, rm), sc.scene.within(p, rm)
    exp, einst, ewi = NQ.closest_point(insts, p, rm)
    _same(got.buffer, exp, "closestPoint")
    _same(got.geom, einst, "closestPoint inst")
    _same(wi, ewi, "within")
    par = NQ.parities(insts, p, max(samples))
    out = {}
    for s in samples:
        ins = sc.scene.inside(p, s)
        assert ins.dtype == np.bool_
        _same(ins, IQ.vote(par, s), "inside %d" % s)
        sd = sc.scene.signedDistance(p, rm, s)
        esd = exp.copy()
        esd.view(U)[(einst >= 0) & ins, 2] |= U(0x80000000)
        _same(sd.buffer, esd, "signedDistance %d" % s)
        _same(sd.geom, einst, "signedDistance inst")
        out[s] = ins
    return got, out


def _all_cases(sc, tris, o, d, seed):
    """the scene suite's cases (tests/test_gpu_scene_query.py _all_cases) on queries aimed at the unposed mesh's box: the poses
    shift the parts by a fraction of it, so the queries meet the posed parts as they met the mesh"""
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


def _cut_and_posed(psm, ctx, tris, parts, seed):
    pieces, _ = SQ.split(tris, _sizes(tris.shape[0], parts))
    assert len(pieces) == parts
    diag = float(np.linalg.norm(tris.reshape(-1, 3).max(0) - tris.reshape(-1, 3).min(0)))
    return _Inst(psm, ctx, pieces, list(enumerate(_poses(seed, parts, 0.05 * diag))))


@pytest.mark.parametrize("parts", [2, 3, 8])
def test_instances_sponza_like(psm, ctx, oracle, scenes, parts):
    sm = scenes.sponza_like(30011)
    tris = sm["tris"].reshape(-1, 3, 3)
    o, d = _camera_rays(oracle, scenes, sm, 32, 18)
    with _cut_and_posed(psm, ctx, tris, parts, 70 + parts) as sc:
        got = _all_cases(sc, tris, o, d, 40 + parts)
        assert len(set(got.geom[got.geom >= 0])) >= 2


@pytest.mark.parametrize("seed,parts", [(0, 2), (1, 3), (2, 8), (3, 3), (4, 2), (5, 8), (6, 3), (7, 2)])
def test_instances_fuzz_soups(psm, ctx, seed, parts):
    tris, o, d, _ = fuzz_case(seed)
    if tris.shape[0] < parts:
        tris = np.concatenate([tris] * parts)
    with _cut_and_posed(psm, ctx, tris, parts, 500 + seed) as sc:
        _all_cases(sc, tris, o[:192], d[:192], 300 + seed)


@pytest.mark.parametrize("opt", [ROT_SCALE, SHEAR], ids=["rotate_scale", "shear"])
def test_a_member_built_with_an_optimisation_matrix(psm, ctx, oracle, scenes, opt):
    """One of three posed members built with a matrix: the file's yardsticks, bit for bit, on the rays that are fully well-posed
    in every member's object space and on the points whose vote rays all are (tests/ray_prune_model.py; the other rays' contract
    is the single hierarchy's, tests/test_gpu_ray_matrix.py); at most 1 % of the rays and of the points are left out"""
    sm = scenes.sponza_like(3001)
    tris = sm["tris"].reshape(-1, 3, 3)
    pieces, _ = SQ.split(tris, _sizes(tris.shape[0], 3))
    diag = float(np.linalg.norm(tris.reshape(-1, 3).max(0) - tris.reshape(-1, 3).min(0)))
    with _Inst(psm, ctx, pieces, list(enumerate(_poses(73, 3, 0.05 * diag))), [None, opt, None]) as sc:
        t = np.array(sc.ths[1].info().transform).reshape(4, 4)[:3, :3]
        assert np.abs(t - np.diag(np.diag(t))).max() > 0.01
        members = [(tr, lv, np.array(sc.ths[k].info().transform, F), m) for k, (tr, lv, m) in zip(sc.which, sc.insts())]
        world = np.concatenate([NQ.posed(tr, m) for tr, _, _, m in members])     # (the grazing rays graze the POSED triangles)
        rng = np.random.RandomState(62)
        oo, od = _camera_rays(oracle, scenes, sm, 32, 16)
        rays = RP.ray_classes(rng, world, oo, od, 512)
        o, d = (np.concatenate([rays[c][k] for c in ("own", "random", "outside", "tilt1e-3", "tilt1e-5")]) for k in (0, 1))
        keep = RP.fully_well_posed(members, o, d)
        assert (~keep).sum() <= 0.01 * keep.size, int((~keep).sum())
        o, d = o[keep], d[keep]
        got = _check_rays(sc, o, d)
        assert (got.geom == 1).sum() > 50 and (got.geom == 2).sum() > 50   # (the member with the matrix is hit, and another)
        _check_rays(sc, o, d, *_windows(rng, got.t.copy(), o.shape[0]))
        p = _scene_points(rng, world, 512)
        sure = RP.vote_rays_well_posed(members, p, IQ.INSIDE_DIRECTIONS)
        assert (~sure).sum() <= 0.01 * sure.size, int((~sure).sum())
        _check_points(sc, p[sure])
        _check_points(sc, p[sure], rng.uniform(0, 2.0, int(sure.sum())).astype(F), samples=(3,))


@functools.lru_cache(maxsize=None)
def _cases():
    return IQ.geometry_cases()


def test_one_torus_at_32_poses_inside_is_analytic(psm, ctx):
    """one hierarchy, 32 instances on a 4 x 4 x 2 lattice wide enough that no two tori touch, each turned or mirrored: a seeded
    point of the torus case mapped through pose k is inside (the analytic answer of the unposed torus) iff the scene says so,
    for 3 and 5 rays -- each ray crosses up to 31 other bodies an even number of times"""
    name, tris, p, truth, clearance, gap = _cases()[1]
    assert name == "torus" and gap < clearance
    ext = float(np.abs(tris).max()) * 2 * 1.8            # (lattice pitch: beyond the diagonal of a torus' box)
    rng = np.random.RandomState(90)
    poses = _poses(91, 32, 0.0)
    for k, m in enumerate(poses):
        m[:, 3] = F([k % 4, (k // 4) % 4, k // 16]) * F(ext)
    with _Inst(psm, ctx, [tris], [(0, m) for m in poses]) as sc:
        assert sc.ths[0].info().leaf_count == tris.shape[0]
        pick = rng.randint(0, 32, 4000)
        q, t = p[:4000], truth[:4000]
        world = np.stack([NQ.to_world(poses[k], q[i:i + 1])[0] for i, k in enumerate(pick)]).astype(F)
        for s in (3, 5):
            ins = sc.scene.inside(world, s)
            bad = np.nonzero(ins != t)[0]
            assert bad.size == 0, (s, bad.size, world[bad[:4]])
        sd = sc.scene.signedDistance(world, samples=3)
        assert (sd.geom >= 0).all() and np.array_equal(np.signbit(sd.t), t)
        near = np.abs(sd.t) < 0.25 * ext
        assert near.mean() > 0.9 and np.array_equal(sd.geom[near], pick[near].astype(np.int32))
        _check_points(sc, world[:600], samples=(3,))
        o, d = _random_rays(rng, NQ.posed(tris, poses[5]), 512)
        _check_rays(sc, o, d)


@pytest.mark.parametrize("level,sizes", [(2, (100,)), (3, (300, 500))], ids=["level2_2parts", "level3_3parts"])
def test_icosphere_cut_into_parts_under_one_pose(psm, ctx, level, sizes):
    """a unit icosphere cut by triangle index, every part placed by ONE pose (a reflection): inside and the sign are the analytic
    answer of the posed sphere away from the surface, and the distance is the analytic one to within the faceting bound.
    The bound: the vertices lie on the unit sphere and a flat triangle sags below it by at most 1 - cos(a), a the angle its
    circumradius spans; after `level` subdivisions the longest edge is at most the icosahedron's 2 sin(0.5536) / 2^level times a
    projection factor (pushing the midpoints out to the sphere lengthens the middle triangles: 1.18, 1.24, 1.25, 1.26 at levels
    1 .. 4, converging; 1.3 is taken and asserted), and the circumradius of a near-equilateral triangle at most
    edge / sqrt 3 * 1.2. The mesh lies between the spheres of radius cos(a) and 1, so
    |dist - | |p - c| - 1 | | <= 1 - cos(a) (+ float32 rounding, 1e-5): 0.028 at level 2, 0.0070 at level 3."""
    tris = IQ.icosphere(level)
    bound = 2 * np.sin(0.5536) / 2 ** level * 1.3
    assert max(float(np.linalg.norm((tris[:, a] - tris[:, b]).astype(np.float64), axis=1).max()) for a, b in ((1, 0), (2, 0), (2, 1))) <= bound
    sag = 1.0 - np.cos(np.arcsin(bound / np.sqrt(3) * 1.2))
    pose = NQ.random_pose(np.random.RandomState(60 + level), reflect=True, shift=3.0)
    pieces, _ = SQ.split(tris, sizes)
    rng = np.random.RandomState(61)
    p = (rng.uniform(-1.6, 1.6, (4000, 3)) + pose[:, 3]).astype(F)
    rad = np.linalg.norm(p.astype(np.float64) - pose[:, 3].astype(np.float64), axis=1)
    with _Inst(psm, ctx, pieces, [(k, pose) for k in range(len(pieces))]) as sc:
        clear = (rad < 1.0 - sag - 1e-4) | (rad > 1.0 + 1e-4)
        assert clear.mean() > 0.9
        for s in (3, 5):
            ins = sc.scene.inside(p, s)
            assert np.array_equal(ins[clear], (rad < 1.0)[clear]), s
            sd = sc.scene.signedDistance(p, samples=s)
            assert (sd.geom >= 0).all() and np.array_equal(np.signbit(sd.t)[clear], (rad < 1.0)[clear])
            err = np.abs(np.abs(sd.t.astype(np.float64)) - np.abs(rad - 1.0))
            assert err.max() <= sag + 1e-5, (err.max(), sag)
        assert len(set(sd.geom.tolist())) == len(pieces)
        _check_points(sc, p[:800], samples=(1, 3, 5))


def test_identity_instances_equal_the_scene_queries(psm, ctx, scenes):
    """(3): identity poses move nothing (x - 0 and 1 * x + 0 * y + 0 * z are exact for inputs without exact zeros, whose sign a
    sum with +0 could change): every answer is QueryScene's on the same hierarchies, bit for bit"""
    tris = scenes.sponza_like(3000)["tris"].reshape(-1, 3, 3)
    n = tris.shape[0]
    pieces, _ = SQ.split(tris, (n // 5, n // 2))
    rng = np.random.RandomState(8)
    o, d = _random_rays(rng, tris, 2048)
    p = _scene_points(rng, tris, 2048)[:-2]
    keep = (o != 0).all(1) & (d != 0).all(1)
    o, d, p = o[keep], d[keep], p[(p != 0).all(1)]
    # (the scene's walls lie in coordinate planes: many of the surface and vertex samples have a zero and are left out)
    assert o.shape[0] > 1024 and p.shape[0] > 1024
    with _Inst(psm, ctx, pieces, [(k, NQ.IDENTITY) for k in range(3)]) as sc:
        ref = psm.QueryScene(ctx, sc.ths)
        tmin, tmax = _windows(rng, ref.intersect(o, d).t.copy(), o.shape[0])
        for lo, hi in ((0.0, np.inf), (tmin, tmax)):
            a, b = sc.scene.intersect(o, d, lo, hi), ref.intersect(o, d, lo, hi)
            _same(a.buffer, b.buffer, "identity intersect")
            _same(a.geom, b.geom, "identity inst")
            _same(sc.scene.occluded(o, d, lo, hi), ref.occluded(o, d, lo, hi), "identity occluded")
            _same(sc.scene.countHits(o, d, lo, hi), ref.countHits(o, d, lo, hi), "identity countHits")
        assert (a.geom >= 0).any()
        diag = float(np.linalg.norm(tris.reshape(-1, 3).max(0) - tris.reshape(-1, 3).min(0)))
        for rm in (np.inf, rng.uniform(0, 0.1 * diag, p.shape[0]).astype(F)):
            a, b = sc.scene.closestPoint(p, rm), ref.closestPoint(p, rm)
            _same(a.buffer, b.buffer, "identity closestPoint")
            _same(a.geom, b.geom, "identity closestPoint inst")
            _same(sc.scene.within(p, rm), ref.within(p, rm), "identity within")
            for s in (1, 3, 5):
                _same(sc.scene.inside(p, s), ref.inside(p, s), "identity inside")
                a, b = sc.scene.signedDistance(p, rm, s), ref.signedDistance(p, rm, s)
                _same(a.buffer, b.buffer, "identity signedDistance")
                _same(a.geom, b.geom, "identity signedDistance inst")


@pytest.mark.parametrize("seed,parts", BAKED_CASES)
def test_instances_against_hierarchies_built_from_the_moved_triangles(psm, ctx, seed, parts):
    """(4): the instanced answers (object space) against a QueryScene over hierarchies built from the pre-moved triangles (world
    space; NQ.posed): the one comparison that does not go through the model's own move(). The two are independent float32
    computations, so flags, counts and (inst, tri) must be identical on every query whose decision margin in the model
    (tests/instance_query_model.py: gap to the runner-up, distance to the window or radius edge, distance of a crossing from its
    triangle's boundary) exceeds 8 x the largest float32 / float64 deviation of the model on these inputs; at most 1 % of the
    queries may be left out (tests/test_instance_query_cpu.py holds the seeds to that without a device). Measured: deviation
    4.4e-6 .. 4.7e-6 for rays and 5.1e-7 .. 5.6e-7 for points, thresholds 3.5e-5 .. 3.7e-5 and 4.1e-6 .. 4.5e-6."""
    pieces, poses, (o, d, tmin, tmax), (p, rmax) = NQ.baked_case(seed, parts)
    with _Inst(psm, ctx, pieces, list(enumerate(poses))) as sc:
        baked = [_hier(psm, ctx, NQ.posed(t, m)) for t, m in zip(pieces, poses)]
        try:
            for th, t in zip(sc.ths + baked, pieces + pieces):      # no build drops a triangle: ids mean the same on both sides
                assert th.info().leaf_count == t.shape[0]
            ref = psm.QueryScene(ctx, baked)
            insts = sc.insts()
            margin, dev = NQ.ray_margin_and_deviation(insts, o, d, tmin, tmax)
            keep = margin > 8 * dev
            print("rays: deviation %.3g, threshold %.3g, left out %.4f" % (dev, 8 * dev, 1 - keep.mean()))
            assert (~keep).mean() <= 0.01
            a, b = sc.scene.intersect(o, d, tmin, tmax), ref.intersect(o, d, tmin, tmax)
            assert (a.geom[keep] >= 0).mean() > 0.1
            _same(a.geom[keep], b.geom[keep], "baked: inst")
            _same(a.tri[keep], b.tri[keep], "baked: tri")
            _same(sc.scene.occluded(o, d, tmin, tmax)[keep], ref.occluded(o, d, tmin, tmax)[keep], "baked: occluded")
            _same(sc.scene.countHits(o, d, tmin, tmax)[keep], ref.countHits(o, d, tmin, tmax)[keep], "baked: countHits")
            margin, dev = NQ.point_margin_and_deviation(insts, p, rmax)
            keep = margin > 8 * dev
            print("points: deviation %.3g, threshold %.3g, left out %.4f" % (dev, 8 * dev, 1 - keep.mean()))
            assert (~keep).mean() <= 0.01
            a, b = sc.scene.closestPoint(p, rmax), ref.closestPoint(p, rmax)
            assert 0.2 < (a.geom[keep] >= 0).mean() < 0.8
            _same(a.geom[keep], b.geom[keep], "baked: closestPoint inst")
            _same(a.tri[keep], b.tri[keep], "baked: closestPoint tri")
            _same(sc.scene.within(p, rmax)[keep], ref.within(p, rmax)[keep], "baked: within")
        finally:
            for th in baked:
                th.close()


def test_a_pose_changed_between_calls_and_refit_rebuild_under_a_live_scene(psm, ctx):
    """(5): setTransform() between two calls: no rebuild, the second call follows the new pose; then one instance's hierarchy
    refitted, then rebuilt with other triangles (a new native handle), the scene object the same throughout"""
    outer, inner = IQ.icosphere(3), IQ.icosphere(2, 0.5)
    rng = np.random.RandomState(21)
    p = rng.uniform(-1.2, 1.2, (2000, 3)).astype(F)
    o, d = p[:1024], rng.normal(size=(1024, 3)).astype(F)
    poses = _poses(22, 2, 0.0)
    with _Inst(psm, ctx, [outer, inner], list(enumerate(poses))) as sc:
        before = _check_rays(sc, o, d)
        rad = np.linalg.norm(p.astype(np.float64), axis=1)
        clear = (np.abs(rad - 1.0) > 0.02) & (np.abs(rad - 0.5) > 0.02)
        ins = _check_points(sc, p, samples=(3,))[1][3]
        assert np.array_equal(ins[clear], ((rad < 1.0) & (rad > 0.5))[clear])
        built = sc.ths[1].info().leaf_count
        away = poses[1].copy()
        away[:, 3] = [0.3, -0.2, 0.1]                     # the inner ball moves inside the outer one
        sc.scene.setTransform(1, away)
        assert np.array_equal(sc.scene.transforms()[1], away) and sc.ths[1].info().leaf_count == built
        after = _check_rays(sc, o, d)
        assert (after.buffer.view(U) != before.buffer.view(U)).any()
        rin = np.linalg.norm(p.astype(np.float64) - away[:, 3].astype(np.float64), axis=1)
        clear = (np.abs(rad - 1.0) > 0.02) & (np.abs(rin - 0.5) > 0.02)
        ins = _check_points(sc, p, samples=(3,))[1][3]
        assert np.array_equal(ins[clear], ((rad < 1.0) & (rin > 0.5))[clear])
        moved = (inner * F(0.8)).astype(F)                # within the build's bounds
        sc.ths[1].clearTribuffer()
        sc.ths[1].loadTriangles(moved.reshape(-1, 9))
        sc.ths[1].refit()
        sc.meshes[1] = moved
        _check_rays(sc, o, d)
        ins = _check_points(sc, p, samples=(3,))[1][3]
        clear = (np.abs(rad - 1.0) > 0.02) & (np.abs(rin - 0.4) > 0.02)
        assert np.array_equal(ins[clear], ((rad < 1.0) & (rin > 0.4))[clear])
        other = (IQ.torus() * F(0.4)).astype(F)
        sc.ths[1].allocate(other.shape[0])
        sc.ths[1].loadTriangles(other.reshape(-1, 9))
        sc.ths[1].build()
        sc.meshes[1] = other
        got = _check_rays(sc, o, d)
        assert (got.geom == 1).any() and (got.geom == 0).any()
        _check_points(sc, p, samples=(3,))


def test_instances_host_checks(psm, ctx, scenes):
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
        eye = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]

        def lst(*entries):
            v = (psm.Instance * len(entries))()
            for k, e in enumerate(entries):
                th, m = e if isinstance(e, tuple) else (e, eye)
                v[k].bvh = th._h.value if th is not None else None
                v[k].world_from_object[:] = m
            return v

        scaled, sheared, nan, mirror = list(eye), list(eye), list(eye), list(eye)
        scaled[0], sheared[1], nan[11], mirror[5] = 1.0001, 1e-4, float("nan"), -1
        for n in (one, zero):   # the list is checked for n = 0 too
            assert lib.psm_instances_intersect_dev(lst(built, None), u32(2), P(p), n, P(p), P(p + 64)) == -1
            assert err() == "psm_instances_intersect_dev: instance 1 is NULL"
            assert lib.psm_instances_count_hits_dev(lst(built, built, foreign), u32(3), P(p), n, P(p)) == -1
            assert err() == "psm_instances_count_hits_dev: instance 2 belongs to another context"
            assert lib.psm_instances_inside_dev(lst(built, unbuilt), u32(2), P(p), n, three, P(p)) == -5
            assert err() == "psm_instances_inside_dev: instance 1 is not built"
            assert lib.psm_instances_within_dev(lst(built, (built, nan)), u32(2), P(p), n, P(p)) == -1
            assert err() == "psm_instances_within_dev: instance 1 has a non-finite transform"
            for bad in (scaled, sheared):
                assert lib.psm_instances_occluded_dev(lst((built, mirror), built, (built, bad)), u32(3), P(p), n, P(p)) == -1
                assert err().startswith("psm_instances_occluded_dev: instance 2 has a transform that is not rigid")
            # the poses are judged before the hierarchies' state: all of it on the host
            assert lib.psm_instances_occluded_dev(lst(unbuilt, (built, scaled)), u32(2), P(p), n, P(p)) == -1
            assert lib.psm_instances_occluded_dev(lst(built), u32(0), P(p), n, P(p)) == -1
            assert lib.psm_instances_occluded_dev(lst(*[built] * 33), u32(33), P(p), n, P(p)) == -1
        g = lst((built, mirror), built)
        assert lib.psm_instances_intersect_dev(g, u32(2), None, zero, None, None) == 0           # n = 0: no data is touched
        assert lib.psm_instances_intersect_dev(g, u32(2), None, one, P(p), P(p + 64)) == -1
        assert lib.psm_instances_intersect_dev(g, u32(2), P(p), one, P(p + 32), None) == -1      # inst must not be NULL
        assert err() == "psm_instances_intersect_dev: NULL pointer"
        assert lib.psm_instances_intersect_dev(g, u32(2), P(p), one, P(p + 32), P(p + 66)) == -1
        assert err() == "psm_instances_intersect_dev: inst not 4-byte aligned"
        assert lib.psm_instances_closest_point_dev(g, u32(2), P(p), one, P(p + 36), P(p + 64)) == -1
        assert err() == "psm_instances_closest_point_dev: points or hits not 16-byte aligned"
        assert lib.psm_instances_count_hits_dev(g, u32(2), P(p), one, P(p + 34)) == -1
        assert err() == "psm_instances_count_hits_dev: counts not 4-byte aligned"
        for s in (0, 2, 4, 6):
            assert lib.psm_instances_inside_dev(g, u32(2), P(p), one, u32(s), P(p + 64)) == -1
            assert lib.psm_instances_signed_distance_dev(g, u32(2), P(p), one, u32(s), P(p + 32), P(p + 64)) == -1
        assert err() == "psm_instances_signed_distance_dev: samples must be 1, 3 or 5"
        assert lib.psm_instances_signed_distance_dev(g, u32(2), P(p), one, three, P(p + 32), P(p + 68)) == 0
        ctx.sync()
        ctx.buf_free(h)
        with pytest.raises(psm.PsmError, match="instance 1 is not built"):
            psm.InstancedScene(ctx, [(built, np.eye(4)), (unbuilt, np.eye(4))]).occluded(np.zeros((2, 3), F), np.ones((2, 3), F))
        empty = psm.InstancedScene(ctx, [(built, np.eye(4))] * 2).intersect(np.zeros((0, 3), F), np.zeros((0, 3), F))
        assert len(empty) == 0 and empty.geom.shape == (0,) and empty.geom.dtype == np.int32
    finally:
        foreign.close()
        other_ctx.close()
        unbuilt.close()
        built.close()
    # the deep fixture (its walk leaves the 16 stack entries kept in LDS) beside a shallow instance, both posed
    deep, o, d = Q.deep_fixture()
    box = (scenes.cornell()["tris"].reshape(-1, 3, 3) * F(0.002) + F([0.006, 0, 0])).astype(F)
    pose = NQ.random_pose(np.random.RandomState(3), shift=0.5)
    wo = NQ.to_world(pose, o).astype(F)
    wd = (NQ.to_world(pose, d) - pose[:, 3].astype(np.float64)).astype(F)
    for order in ((0, 1), (1, 0), (0, 1, 0)):
        with _Inst(psm, ctx, [deep, box], [(k, pose) for k in order]) as sc:
            got = _check_rays(sc, wo, wd)
            assert (got.geom >= 0).all() and len(set(got.geom.tolist())) == 2
            _check_rays(sc, wo, wd, 0.25, 1.0)
            _check_points(sc, (wo[:128] + np.random.RandomState(12).normal(0, 1e-3, (128, 3))).astype(F), samples=(3,))
            assert sc.scene.countHits(wo, wd).max() >= 8


def test_instances_torch_tensors_on_a_non_default_stream(psm, ctx):
    if torch is None:
        pytest.skip("torch is not installed")
    parts, _ = SQ.split(IQ.torus(), (500, 1000))
    rng = np.random.RandomState(6)
    p = rng.uniform([-1.6, -1.6, -0.6], [1.6, 1.6, 0.6], (4099, 3)).astype(F)
    p[-1] = [np.nan, 0, 0]
    o, d = p, rng.normal(size=p.shape).astype(F)
    tmin = rng.uniform(-1, 0.5, p.shape[0]).astype(F)
    r = rng.uniform(0, 0.3, p.shape[0]).astype(F)
    entries = list(enumerate(_poses(66, 3, 0.2)))
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        own = psm.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        try:
            for c in (own, ctx):     # a context on torch's (non-default) current stream, and one with a stream of its own
                with _Inst(psm, c, parts, entries) as sc:
                    to, td, tt, tr = (torch.from_numpy(x).to(dev) for x in (o, d, tmin, r))
                    got, ref = sc.scene.intersect(to, td, tt), sc.scene.intersect(o, d, tmin)
                    assert got.buffer.device == dev and got.geom.device == dev and got.geom.dtype == torch.int32
                    _same(got.buffer.cpu().numpy(), ref.buffer, "torch intersect")
                    _same(got.geom.cpu().numpy(), ref.geom, "torch inst")
                    assert (ref.geom >= 0).any()
                    _same(sc.scene.occluded(to, td, tt).cpu().numpy(), sc.scene.occluded(o, d, tmin), "torch occluded")
                    _same(sc.scene.countHits(to, td, tt).cpu().numpy().view(np.uint32), sc.scene.countHits(o, d, tmin), "torch countHits")
                    cp, cref = sc.scene.closestPoint(to, tr), sc.scene.closestPoint(p, r)
                    _same(cp.buffer.cpu().numpy(), cref.buffer, "torch closestPoint")
                    _same(cp.geom.cpu().numpy(), cref.geom, "torch closestPoint inst")
                    _same(sc.scene.within(to, tr).cpu().numpy(), sc.scene.within(p, r), "torch within")
                    for s in (1, 3, 5):
                        _same(sc.scene.inside(to, s).cpu().numpy(), sc.scene.inside(p, s), "torch inside")
                        sd, sref = sc.scene.signedDistance(to, tr, s), sc.scene.signedDistance(p, r, s)
                        _same(sd.buffer.cpu().numpy(), sref.buffer, "torch signedDistance")
                        _same(sd.geom.cpu().numpy(), sref.geom, "torch signedDistance inst")
                    _check_rays(sc, o[:512], d[:512], tmin[:512])
        finally:
            own.close()
    torch.cuda.synchronize()


def test_a_captured_graph_replays_the_poses_it_was_captured_with(psm, ctx):
    """(8): an instanced query captured into a linear graph after a first plain call; the pose is then changed on the host: the
    replay answers with the capture-time pose (the transforms travelled in the kernel arguments), a fresh call with the new one"""
    hip = psm._hip()
    parts, _ = SQ.split(IQ.icosphere(3), (300, 500))
    rng = np.random.RandomState(31)
    n = 3000
    old = _poses(32, 3, 0.1)
    new = _poses(33, 3, 0.3)
    with _Inst(psm, ctx, parts, list(enumerate(old))) as sc:
        lib = psm.lib()
        p = rng.uniform(-1.3, 1.3, (n, 3)).astype(F)
        rays, pts = np.zeros((n, 8), F), np.zeros((n, 4), F)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = p, 0, rng.normal(size=(n, 3)), np.inf
        pts[:, 0:3], pts[:, 3] = p, np.inf
        sizes = (rays.nbytes, pts.nbytes, 16 * n, 4 * n, 16 * n, 4 * n)
        hs = [ctx.buf_alloc(s) for s in sizes]
        ptr = [ctypes.c_void_p(ctx.buf_ptr(h)[0]) for h in hs]
        ctx.buf_upload(hs[0], rays)
        ctx.buf_upload(hs[1], pts)
        cn, three, u3 = ctypes.c_size_t(n), ctypes.c_uint32(3), ctypes.c_uint32(3)

        def launch(poses):
            v = (psm.Instance * 3)()
            for k in range(3):
                v[k].bvh = sc.ths[k]._h.value
                v[k].world_from_object[:] = poses[k].reshape(12).tolist()
            assert lib.psm_instances_intersect_dev(v, u3, ptr[0], cn, ptr[2], ptr[3]) == 0
            assert lib.psm_instances_signed_distance_dev(v, u3, ptr[1], cn, three, ptr[4], ptr[5]) == 0
            return v

        def results():
            ctx.sync()
            return (ctx.buf_download(hs[2], F, 4 * n).reshape(n, 4), ctx.buf_download(hs[3], np.int32, n),
                    ctx.buf_download(hs[4], F, 4 * n).reshape(n, 4), ctx.buf_download(hs[5], np.int32, n))

        def wipe():
            for h, size in zip(hs[2:], sizes[2:]):
                ctx.buf_upload(h, np.full(size // 4, 0x7f, np.int32))

        launch(old)                      # the first plain call (it allocates the context's stack area)
        first = results()
        eh, es = sc.scene.intersect(p, rays[:, 4:7]), sc.scene.signedDistance(p)
        for got, exp in zip(first, (eh.buffer, eh.geom, es.buffer, es.geom)):
            _same(got, exp, "plain call")
        stream = ctypes.c_void_p(ctx.stream)
        graph, exe = ctypes.c_void_p(), ctypes.c_void_p()
        assert hip.hipStreamBeginCapture(stream, ctypes.c_int(1)) == 0        # hipStreamCaptureModeThreadLocal
        try:
            held = launch(old)
        finally:
            rc = hip.hipStreamEndCapture(stream, ctypes.byref(graph))
        assert rc == 0 and graph.value
        nodes = ctypes.c_size_t(0)
        assert hip.hipGraphGetNodes(graph, None, ctypes.byref(nodes)) == 0 and nodes.value == 3    # one launch + two: linear
        assert hip.hipGraphInstantiate(ctypes.byref(exe), graph, None, None, ctypes.c_size_t(0)) == 0
        try:
            for k in range(3):           # the pose changes on the host: in the scene, and in the very list that was captured from
                sc.scene.setTransform(k, new[k])
                held[k].world_from_object[:] = new[k].reshape(12).tolist()
            wipe()
            assert hip.hipGraphLaunch(exe, stream) == 0
            for got, exp in zip(results(), first):
                _same(got, exp, "the replay answers with the capture-time poses")
            wipe()
            launch(new)
            fresh = results()
            nh, ns = sc.scene.intersect(p, rays[:, 4:7]), sc.scene.signedDistance(p)
            for got, exp in zip(fresh, (nh.buffer, nh.geom, ns.buffer, ns.geom)):
                _same(got, exp, "a fresh call answers with the new poses")
            assert (fresh[0].view(U) != first[0].view(U)).any() and (fresh[2].view(U) != first[2].view(U)).any()
            _check_rays(sc, p[:512], rays[:512, 4:7])
        finally:
            hip.hipGraphExecDestroy(exe)
            hip.hipGraphDestroy(graph)
            for h in hs:
                ctx.buf_free(h)
