"""GPU tests of the instance worlds (psm_world_*, world.hip; InstanceWorld): every kind bit for bit against the
flat answer of world_query_model part (a), at sizes on both sides of the instanced queries' limit; behaviour and refusals."""
import ctypes
import functools

import numpy as np
import pytest

import inside_query_model as IQ
import instance_query_model as NQ
import query_model as Q
import ray_prune_model as RP
import world_query_model as WQ
from test_gpu_point_query import ROT_SCALE, SHEAR
from test_gpu_point_query import _hier as _hier_opt
from test_gpu_query import _hier, _leaves
from test_world_query_cpu import _same, _shift, soup_case, soup_entries, unit_box

try:   # (imported before the library loads its HIP runtime, as tests/test_gpu_query.py)
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32


class _World:
    """hierarchies over meshes, an InstanceWorld of (mesh index, pose) entries, and the model's instances"""

    def __init__(self, psm, ctx, meshes, entries, opts=None):
        self.psm, self.ctx = psm, ctx
        self.meshes = [np.ascontiguousarray(t, F).reshape(-1, 3, 3) for t in meshes]
        self.ths = [_hier(psm, ctx, t) for t in self.meshes] if opts is None else [_hier_opt(psm, ctx, t, m) for t, m in zip(self.meshes, opts)]
        self.which = [k for k, _ in entries]
        self.world = psm.InstanceWorld(ctx, [(self.ths[k], m) for k, m in entries])

    def insts(self):
        leaves = [_leaves(self.psm, th) for th in self.ths]
        return [(self.meshes[k], leaves[k], m) for k, m in zip(self.which, self.world.transforms())]

    def members(self):
        """the instances as tests/ray_prune_model.py judges rays against them: (tris, leaves, the hierarchy's transform, pose)"""
        ms = [np.array(th.info().transform, F) for th in self.ths]
        return [(tr, lv, ms[k], m) for k, (tr, lv, m) in zip(self.which, self.insts())]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.world.close()
        for th in self.ths:
            th.close()


def _check(sc, rays, points, samples=(1, 3, 5), insts=None):
    """all seven kinds against (a)"""
    insts = sc.insts() if insts is None else insts
    w = sc.world
    o, d, tmin, tmax = rays
    n = o.shape[0]
    lo, hi = np.broadcast_to(np.asarray(tmin, F), (n,)).copy(), np.broadcast_to(np.asarray(tmax, F), (n,)).copy()
    eh, ei, ea, ec = WQ.flat_rays(WQ.per_instance_rays(insts, o, d, lo, hi))
    got = w.intersect(o, d, lo, hi)
    _same(got.buffer, eh, "intersect")
    _same(got.geom, ei, "intersect inst")
    _same(w.occluded(o, d, lo, hi), ea, "occluded")
    _same(w.countHits(o, d, lo, hi), ec, "countHits")
    p, rmax = points
    rm = np.broadcast_to(np.asarray(rmax, F), (p.shape[0],)).copy()
    ph, pi, pw = WQ.flat_points(WQ.per_instance_points(insts, p, rm))
    gp = w.closestPoint(p, rm)
    _same(gp.buffer, ph, "closestPoint")
    _same(gp.geom, pi, "closestPoint inst")
    _same(w.within(p, rm), pw, "within")
    par = WQ.flat_parities(WQ.per_instance_parities(insts, p, max(samples)))
    for s in samples:
        ins = IQ.vote(par[:s] if s < par.shape[0] else par, s)
        _same(w.inside(p, s), ins, "inside %d" % s)
        sd = w.signedDistance(p, rm, s)
        _same(sd.buffer, WQ.signed(ph, pi, ins), "signedDistance %d" % s)
        _same(sd.geom, pi, "signedDistance inst")
    return got, gp


def _posed_entries(n, seed):
    """n entries over two meshes (0: the icosphere, 1: the torus): random rotations and reflections, translations that leave some
    bodies overlapping, and every fifth exactly where its predecessor is (touching everywhere: ties)"""
    rng = np.random.RandomState(seed)
    spread = max(1.0, n ** (1.0 / 3.0))
    out = []
    for k in range(n):
        m = NQ.random_pose(rng, reflect=bool(k & 1), shift=spread)
        if k % 5 == 4:
            m = out[-1][1].copy()
        out.append((k % 2, m))
    return out, spread


def _queries(rng, spread, n=2000):
    o = rng.uniform(-spread - 1.5, spread + 1.5, (n, 3)).astype(F)
    d = (rng.uniform(-spread, spread, (n, 3)) - o).astype(F)
    tmin = rng.uniform(-0.5, 1.0, n).astype(F)
    tmax = (tmin + rng.uniform(0.0, 3.0 * spread, n)).astype(F)
    tmax[:8] = np.inf
    p = rng.uniform(-spread - 1.2, spread + 1.2, (n, 3)).astype(F)
    rmax = rng.uniform(0.0, 1.0, n).astype(F)
    rmax[:8] = [np.inf, 0, -0.0, -1, np.nan, np.inf, 0, -1]
    return (o, d, tmin, tmax), (p, rmax)


@functools.lru_cache(maxsize=None)
def _meshes():
    return IQ.icosphere(0, 0.6), IQ.torus(8, 4, 0.7, 0.25)


@pytest.mark.parametrize("n", [1, 2, 33, 257])
def test_world_parity_with_the_flat_list(psm, ctx, n):
    """the named test: 33 instances is a list the project could not express"""
    ico, tor = _meshes()
    assert ico.shape[0] == 20 and tor.shape[0] == 64
    entries, spread = _posed_entries(n, 100 + n)
    with _World(psm, ctx, [ico, tor], entries) as sc:
        assert len(sc.world) == n
        rays, points = _queries(np.random.RandomState(n), spread)
        got, gp = _check(sc, rays, points, samples=(3, 5))
        assert (got.geom >= 0).sum() > 50 and (gp.geom >= 0).sum() > 50


def matrix_world_queries(sc, seed, n=1024):
    """rays and points for a world one of whose members was built with a matrix: the files' random queries plus rays that graze
    the posed triangles, cut down to the rays that are fully well-posed in every instance and the points whose vote rays all are
    (tests/ray_prune_model.py); at most 1 % of either is left out. Returns (o, d, tmin, tmax), (p, rmax)."""
    members = sc.members()
    rng = np.random.RandomState(seed)
    (o, d, tmin, tmax), (p, rmax) = _queries(rng, 2.0, n)
    posed = np.concatenate([NQ.posed(tr, m) for tr, _, _, m in members])
    graze = [RP.grazing_rays(rng, posed, n // 4, tilt) for tilt in (1e-3, 1e-5)]
    o, d = np.concatenate([o] + [g[0] for g in graze]), np.concatenate([d] + [g[1] for g in graze])
    tmin, tmax = np.concatenate([tmin, np.zeros(n // 2, F)]), np.concatenate([tmax, np.full(n // 2, np.inf, F)])
    keep = RP.fully_well_posed(members, o, d)
    sure = RP.vote_rays_well_posed(members, p, IQ.INSIDE_DIRECTIONS)
    assert (~keep).sum() <= 0.01 * keep.size and (~sure).sum() <= 0.01 * sure.size, (int((~keep).sum()), int((~sure).sum()))
    return (o[keep], d[keep], tmin[keep], tmax[keep]), (p[sure], rmax[sure])


@pytest.mark.parametrize("opt", [ROT_SCALE, SHEAR], ids=["rotate_scale", "shear"])
def test_a_member_built_with_an_optimisation_matrix(psm, ctx, opt):
    """the torus of a two-mesh world built with a matrix: the seven kinds bit for bit against the flat answer on the fully
    well-posed rays and points (the other rays' contract is the single hierarchy's, tests/test_gpu_ray_matrix.py)"""
    ico, tor = _meshes()
    entries, _ = _posed_entries(7, 107)
    with _World(psm, ctx, [ico, tor], entries, [None, opt]) as sc:
        t = np.array(sc.ths[1].info().transform).reshape(4, 4)[:3, :3]
        assert np.abs(t - np.diag(np.diag(t))).max() > 0.01
        rays, points = matrix_world_queries(sc, 63)
        got, gp = _check(sc, rays, points)
        assert (got.geom >= 0).sum() > 50 and (got.geom[got.geom >= 0] % 2 == 1).any() and (gp.geom >= 0).sum() > 50


def test_world_adversarial_soup(psm, ctx, scenes):
    box, _, rays, points = soup_case()
    with _World(psm, ctx, [unit_box(scenes)], soup_entries()) as sc:
        o, d, tmin, tmax = rays
        _check(sc, (o, d, np.zeros_like(tmin), np.full_like(tmax, np.inf)), (points[0], np.full_like(points[1], np.inf)), samples=(3,))
        _check(sc, rays, points, samples=(3,))


def test_identity_world_equals_the_instanced_scene(psm, ctx):
    ico, tor = _meshes()
    rng = np.random.RandomState(9)
    rays, points = _queries(rng, 1.0, 1000)
    for n in (1, 7, 32):
        with _World(psm, ctx, [ico, tor], [(k % 2, NQ.IDENTITY) for k in range(n)]) as sc:
            flat = psm.InstancedScene(ctx, [(sc.ths[k % 2], NQ.IDENTITY) for k in range(n)])
            a, b = sc.world.intersect(*rays), flat.intersect(*rays)
            _same(a.buffer, b.buffer, "intersect")
            _same(a.geom, b.geom, "inst")
            _same(sc.world.occluded(*rays), flat.occluded(*rays), "occluded")
            _same(sc.world.countHits(*rays), flat.countHits(*rays), "count")
            a, b = sc.world.closestPoint(*points), flat.closestPoint(*points)
            _same(a.buffer, b.buffer, "closestPoint")
            _same(a.geom, b.geom, "closestPoint inst")
            _same(sc.world.within(*points), flat.within(*points), "within")
            _same(sc.world.inside(points[0], 3), flat.inside(points[0], 3), "inside")
            _same(sc.world.signedDistance(*points, 5).buffer, flat.signedDistance(*points, 5).buffer, "signedDistance")


def test_a_cut_icosphere_at_forty_poses_is_inside_analytically(psm, ctx):
    """an icosphere cut into 3 hierarchies x 40 poses: a ray's parity is summed over the parts of a body"""
    ico = IQ.icosphere(2, 0.5)
    third = ico.shape[0] // 3
    parts = [ico[:third], ico[third:2 * third], ico[2 * third:]]
    rng = np.random.RandomState(4)
    poses = []
    for k in range(40):
        m = NQ.random_pose(rng, reflect=bool(k & 1), shift=0.0)
        m[:, 3] = (1.5 * (k % 7), 1.5 * (k // 7), 0.4 * (k % 3))
        poses.append(m)
    entries = [(j, m) for m in poses for j in range(3)]
    with _World(psm, ctx, parts, entries) as sc:
        c = np.asarray([m[:, 3] for m in poses], F)
        u = rng.normal(size=(40, 8, 3))
        u /= np.linalg.norm(u, axis=2, keepdims=True)
        r = np.concatenate([rng.uniform(0.0, 0.42, (40, 4, 1)), rng.uniform(0.56, 0.7, (40, 4, 1))], axis=1)
        p = (c[:, None, :] + u * r).astype(F).reshape(-1, 3)
        inside = (r < 0.5).reshape(-1)
        for s in (3, 5):
            _same(sc.world.inside(p, s), inside, "inside %d" % s)
            sd = sc.world.signedDistance(p, np.inf, s)
            assert (sd.geom >= 0).all() and np.array_equal(np.signbit(sd.t), inside)


def test_set_transform_moves_the_answer_without_a_rebuild(psm, ctx):
    ico, tor = _meshes()
    with _World(psm, ctx, [ico, tor], [(0, _shift(0, 0, 0)), (0, _shift(5, 0, 0)), (1, _shift(0, 5, 0))]) as sc:
        nodes = [th.download(psm.BVH_NODE32, np.uint32, 8 * max(th.info().leaf_count - 1, 1)).copy() for th in sc.ths]
        o, d = np.asarray([[-3, 0.1, 0.05]], F), np.asarray([[1, 0, 0]], F)
        assert sc.world.intersect(o, d).geom[0] == 0
        sc.world.setTransform(0, _shift(0, -9, 0))
        assert sc.world.intersect(o, d).geom[0] == 1
        sc.world.setTransforms(1, [_shift(0, 9, 0), _shift(2, 0, 0)])
        assert sc.world.intersect(o, d).geom[0] == 2
        rays, points = _queries(np.random.RandomState(2), 5.0, 500)
        _check(sc, rays, points, samples=(3,))
        for th, before in zip(sc.ths, nodes):
            assert np.array_equal(th.download(psm.BVH_NODE32, np.uint32, before.size), before)


def test_a_rebuilt_member_is_stale_and_a_refit_needs_a_refresh(psm, ctx):
    ico, tor = _meshes()
    shifts = [_shift(0, 0, 0), _shift(3, 0, 0), _shift(0, 3, 0)]
    with _World(psm, ctx, [ico, tor], [(0, shifts[0]), (1, shifts[1]), (0, shifts[2])]) as sc:
        rays, points = _queries(np.random.RandomState(3), 3.0, 500)
        _check(sc, rays, points, samples=(3,))
        h = sc.ths[1]
        h.markDirty()
        h.build()
        with pytest.raises(psm.PsmError, match="instance 1's hierarchy was rebuilt"):
            sc.world.intersect(rays[0], rays[1])
        with pytest.raises(psm.PsmError, match="instance 1's hierarchy was rebuilt"):
            sc.world.setTransform(0, shifts[0])
        sc.world.setInstances([(sc.ths[k], m) for k, m in zip(sc.which, shifts)])
        _check(sc, rays, points, samples=(3,))
        # a refit: the torus moves out of its boxes; between the reload and the refit the world refuses, after refresh() it is exact
        moved = (tor + F(1.25)).astype(F)
        h.clearTribuffer()
        h.loadTriangles(moved)
        with pytest.raises(psm.PsmError, match="instance 1's hierarchy"):
            sc.world.within(*points)
        h.refit()
        sc.world.refresh()
        sc.meshes[1] = moved
        _check(sc, rays, points, samples=(3,))


def test_depth_refusal_and_the_empty_world(psm, ctx):
    """a chain-shaped tree over the instances (centres at single-bit Morton cells) is ~45 deep: with the 20-triangle icosphere it
    fits the stack and walks its spill area; with the deep fixture's bound it is refused and the world left empty"""
    ico, _ = _meshes()
    deep, _, _ = Q.deep_fixture()
    shifts = [(0.0, 0.0, 0.0)] + [tuple(100.0 * 2.0 ** -k * np.eye(3)[a]) for a in range(3) for k in range(16)]
    rng = np.random.RandomState(6)
    rays, points = _queries(rng, 1.0, 500)
    rays = ((rays[0] * F(30) + F(40)).astype(F), rays[1], rays[2], (rays[3] * F(60)).astype(F))
    points = ((points[0] * F(30) + F(40)).astype(F), (points[1] * F(40)).astype(F))
    with _World(psm, ctx, [ico, deep], [(0, _shift(*s)) for s in shifts]) as sc:
        _check(sc, rays, points, samples=(3,))
        with pytest.raises(psm.PsmError, match="deeper than the query stack"):
            sc.world.setInstances([(sc.ths[1], _shift(*s)) for s in shifts])
        assert len(sc.world) == 0
        o, d, tmin, tmax = rays
        got = sc.world.intersect(o, d, tmin, tmax)
        assert (got.geom == -1).all() and (got.tri == -1).all() and np.isinf(got.t).all()
        assert not sc.world.occluded(o, d, tmin, tmax).any() and not sc.world.countHits(o, d, tmin, tmax).any()
        gp = sc.world.signedDistance(points[0], np.inf, 3)
        assert (gp.geom == -1).all() and not sc.world.inside(points[0], 3).any() and not sc.world.within(*points).any()
        sc.world.setInstances([(sc.ths[1], _shift(0, 0, 0)), (sc.ths[0], _shift(0.5, 0, 0))])   # the deep fixture in a shallow world
        assert len(sc.world) == 2


@pytest.mark.skipif(torch is None, reason="torch is not installed")
def test_world_torch_tensors_on_a_non_default_stream(psm, ctx):
    ico, tor = _meshes()
    entries, spread = _posed_entries(40, 77)
    with _World(psm, ctx, [ico, tor], entries) as sc:
        (o, d, tmin, tmax), (p, rmax) = _queries(np.random.RandomState(8), spread, 1000)
        ref = sc.world.intersect(o, d, tmin, tmax)
        refp = sc.world.closestPoint(p, rmax)
        dev = torch.device("cuda", 0)
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            t = [torch.from_numpy(a).to(dev, non_blocking=True) for a in (o, d, tmin, tmax, p, rmax)]
            got = sc.world.intersect(t[0], t[1], t[2], t[3])
            gp = sc.world.closestPoint(t[4], t[5])
            ins = sc.world.inside(t[4], 3)
        s.synchronize()
        _same(got.buffer.cpu().numpy(), ref.buffer, "torch intersect")
        _same(got.geom.cpu().numpy(), ref.geom, "torch inst")
        _same(gp.buffer.cpu().numpy(), refp.buffer, "torch closestPoint")
        _same(ins.cpu().numpy(), sc.world.inside(p, 3), "torch inside")


def test_65536_poses_of_one_icosphere(psm, ctx):
    """a 256 x 256 grid of one hierarchy; 256 local queries, each checked against (a) over the instances within its reach
    (chosen in float64, with a margin of one pitch)"""
    ico, _ = _meshes()
    side, pitch = 256, 2.0
    rng = np.random.RandomState(12)
    poses = np.repeat(NQ.IDENTITY[None], side * side, axis=0).copy()
    k = np.arange(side * side)
    poses[:, 0, 3], poses[:, 1, 3] = pitch * (k % side), pitch * (k // side)
    turn = NQ.random_pose(rng)
    poses[1::2, :, :3] = turn[:, :3]
    th = _hier(psm, ctx, ico)
    world = psm.InstanceWorld(ctx, [(th, m) for m in poses])
    try:
        assert len(world) == side * side
        cand = _leaves(psm, th)
        n = 256
        at = rng.randint(0, side * side, n)
        c = poses[at, :, 3]
        o = (c + rng.uniform(-1.5, 1.5, (n, 3))).astype(F)
        d = (c + rng.uniform(-0.5, 0.5, (n, 3)) - o).astype(F)
        tmin, tmax = np.zeros(n, F), rng.uniform(0.5, 2.0, n).astype(F)
        p = (c + rng.uniform(-1.2, 1.2, (n, 3))).astype(F)
        rmax = rng.uniform(0.2, 1.0, n).astype(F)
        got, occ, cnt = world.intersect(o, d, tmin, tmax), world.occluded(o, d, tmin, tmax), world.countHits(o, d, tmin, tmax)
        gp, wi = world.closestPoint(p, rmax), world.within(p, rmax)
        centres = poses[:, :, 3].astype(np.float64)
        for i in range(n):
            reach = float(tmax[i]) + 0.6 + pitch
            near = np.nonzero(np.linalg.norm(centres - o[i].astype(np.float64), axis=1) <= reach)[0]
            insts = [(ico, cand, poses[j]) for j in near]
            eh, ei, ea, ec = WQ.flat_rays(WQ.per_instance_rays(insts, o[i:i + 1], d[i:i + 1], tmin[i:i + 1], tmax[i:i + 1]))
            _same(got.buffer[i:i + 1], eh, "intersect %d" % i)
            assert got.geom[i] == (near[ei[0]] if ei[0] >= 0 else -1) and occ[i] == ea[0] and cnt[i] == ec[0], i
            near = np.nonzero(np.linalg.norm(centres - p[i].astype(np.float64), axis=1) <= float(rmax[i]) + 0.6 + pitch)[0]
            insts = [(ico, cand, poses[j]) for j in near]
            ph, pi, pw = WQ.flat_points(WQ.per_instance_points(insts, p[i:i + 1], rmax[i:i + 1]))
            _same(gp.buffer[i:i + 1], ph, "closestPoint %d" % i)
            assert gp.geom[i] == (near[pi[0]] if pi[0] >= 0 else -1) and wi[i] == pw[0], i
        assert (got.geom >= 0).sum() > 30 and (gp.geom >= 0).sum() > 30
    finally:
        world.close()
        th.close()


def test_world_host_checks_by_their_exact_messages(psm, ctx):
    """every refusal of a world query's data and of psm_world_set_instances' list, by return code and text: all of them are
    made on the host before any launch, and a refused list leaves the world as it was"""
    two = np.asarray([[0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1, 1, 0, 1, 0, 1, 1]], F)
    a, b = _hier(psm, ctx, two), _hier(psm, ctx, two + F(2))
    unbuilt = psm.TriangleHierarchy(ctx)
    unbuilt.allocate(4)
    unbuilt.loadTriangles(two)
    other_ctx = psm.Context(0)
    foreign = _hier(psm, other_ctx, two)
    world = psm.InstanceWorld(ctx, [(a, NQ.IDENTITY), (b, NQ.IDENTITY)], capacity=4)
    try:
        lib = psm.lib()
        h = ctx.buf_alloc(256)
        p = ctx.buf_ptr(h)[0]
        P, one, three, u32, w = ctypes.c_void_p, ctypes.c_size_t(1), ctypes.c_uint32(3), ctypes.c_uint32, world._w
        err = lambda: lib.psm_last_error(ctx._h).decode()
        assert lib.psm_world_intersect_dev(w, None, one, P(p + 32), P(p + 64)) == -1
        assert err() == "psm_world_intersect_dev: NULL pointer"
        assert lib.psm_world_closest_point_dev(w, P(p), one, P(p + 32), None) == -1      # inst must not be NULL
        assert err() == "psm_world_closest_point_dev: NULL pointer"
        assert lib.psm_world_within_dev(w, P(p), one, None) == -1
        assert err() == "psm_world_within_dev: NULL pointer"
        assert lib.psm_world_intersect_dev(w, P(p), one, P(p + 36), P(p + 64)) == -1
        assert err() == "psm_world_intersect_dev: rays or hits not 16-byte aligned"
        assert lib.psm_world_closest_point_dev(w, P(p + 8), one, P(p + 32), P(p + 64)) == -1
        assert err() == "psm_world_closest_point_dev: points or hits not 16-byte aligned"
        assert lib.psm_world_occluded_dev(w, P(p + 4), one, P(p + 64)) == -1
        assert err() == "psm_world_occluded_dev: rays not 16-byte aligned"
        assert lib.psm_world_count_hits_dev(w, P(p), one, P(p + 34)) == -1
        assert err() == "psm_world_count_hits_dev: counts not 4-byte aligned"
        assert lib.psm_world_intersect_dev(w, P(p), one, P(p + 32), P(p + 66)) == -1
        assert err() == "psm_world_intersect_dev: inst not 4-byte aligned"
        for s in (0, 2, 4, 6):
            assert lib.psm_world_inside_dev(w, P(p), one, u32(s), P(p + 64)) == -1
            assert err() == "psm_world_inside_dev: samples must be 1, 3 or 5"
            assert lib.psm_world_signed_distance_dev(w, P(p), one, u32(s), P(p + 32), P(p + 64)) == -1
            assert err() == "psm_world_signed_distance_dev: samples must be 1, 3 or 5"
        # the data is judged before the samples, and a NULL before an alignment
        assert lib.psm_world_signed_distance_dev(w, P(p), one, u32(2), P(p + 32), P(p + 66)) == -1
        assert err() == "psm_world_signed_distance_dev: inst not 4-byte aligned"
        assert lib.psm_world_intersect_dev(w, P(p + 4), one, P(p + 32), None) == -1
        assert err() == "psm_world_intersect_dev: NULL pointer"

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
        name = "psm_world_set_instances"
        assert lib.psm_world_set_instances(w, None, u32(2)) == -1
        assert err() == name + ": NULL list"
        assert lib.psm_world_set_instances(w, lst(a, b, a, b, a), u32(5)) == -4
        assert err() == name + ": 5 instances exceed the world's capacity of 4"
        assert lib.psm_world_set_instances(w, lst(a, None), u32(2)) == -1
        assert err() == name + ": instance 1 is NULL"
        assert lib.psm_world_set_instances(w, lst(a, b, foreign), u32(3)) == -1
        assert err() == name + ": instance 2 belongs to another context"
        assert lib.psm_world_set_instances(w, lst(a, (b, nan)), u32(2)) == -1
        assert err() == name + ": instance 1 has a non-finite transform"
        for bad in (scaled, sheared):
            assert lib.psm_world_set_instances(w, lst((a, mirror), b, (b, bad)), u32(3)) == -1
            assert err().startswith(name + ": instance 2 has a transform that is not rigid")
        assert lib.psm_world_set_instances(w, lst(a, unbuilt), u32(2)) == -5
        assert err() == name + ": instance 1 is not built"
        # in the list's order of checks: every handle, then every pose, then every hierarchy's state
        assert lib.psm_world_set_instances(w, lst(unbuilt, (b, scaled), None), u32(3)) == -1
        assert err() == name + ": instance 2 is NULL"
        assert lib.psm_world_set_instances(w, lst(unbuilt, (b, scaled)), u32(2)) == -1
        assert err().startswith(name + ": instance 1 has a transform that is not rigid")
        assert lib.psm_world_count(w) == 2
        ctx.buf_free(h)
    finally:
        world.close()
        foreign.close()
        other_ctx.close()
        unbuilt.close()
        b.close()
        a.close()
