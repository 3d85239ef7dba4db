"""The sphere sweeps of an instance world on the GPU (psm_world_sweep_sphere_dev / psm_world_sweep_occluded_dev, world_sweep.hip;
InstanceWorld.sphereCast / sphereCastOccluded). The yardstick is tests/world_sweep_query_model.py part (a):
sweep_tri in numpy float32 over the downloaded leaves of every instance, the sweep moved as a world ray is. Every comparison is
exact on every sweep -- t, u, v bit for bit, tri and geom -- and in every case the queries are also held against one another:
sphereCastOccluded == isfinite(t), and t == 0 wherever the world's within(origin, radius) counts a pair (and nowhere else, in
the cases whose starts are not built onto dist == radius)."""
import ctypes

import numpy as np
import pytest

import inside_query_model as IQ
import instance_query_model as NQ
import query_model as Q
import world_sweep_query_model as WS
from test_gpu_box_query import GRID_CAP, ROT_SCALE, SHEAR
from test_gpu_world_box import _World
from test_world_box_cpu import _pose, _rotation, cube, lattice_world

try:   # (imported before the library loads its HIP runtime, as tests/test_gpu_query.py)
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
U = np.uint32


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, "%s: %d differ, first %d: %s against %s" % (what, bad.size, bad[0], a[bad[0]], b[bad[0]])


def check_sweeps(sc, o, d, r, tmax=np.inf, insts=None, converse=True):
    """both queries against (a) and against one another and the world's within query; returns (a): hits [n, 4], inst [n]"""
    w = sc.world
    o, d = np.ascontiguousarray(o, F).reshape(-1, 3), np.ascontiguousarray(d, F).reshape(-1, 3)
    n = o.shape[0]
    r, tm = (np.broadcast_to(np.asarray(x, F), (n,)).astype(F) for x in (r, tmax))
    want, winst, occluded = WS.flat(sc.insts() if insts is None else insts, o, d, r, tm)
    got, flag = w.sphereCast(o, d, r, tm), w.sphereCastOccluded(o, d, r, tm)
    assert got.buffer.shape == (n, 4) and got.buffer.dtype == F and got.tri.dtype == np.int32
    assert got.geom.shape == (n,) and got.geom.dtype == np.int32 and flag.shape == (n,) and flag.dtype == np.bool_
    _same(got.buffer.view(U), want.view(U), "sphereCast (u, v, t, tri as bits)")
    _same(got.geom, winst, "sphereCast geom")
    _same(flag, occluded, "sphereCastOccluded")
    assert np.array_equal(flag, np.isfinite(got.t)) and np.array_equal(flag, got.tri >= 0) and np.array_equal(flag, got.geom >= 0)
    valid = WS.world_valid(o, d, r, tm)
    with np.errstate(invalid="ignore"):
        rq = np.where(r >= 0, r, F(-1))                      # (a NaN radius: within misses on a negative one as well)
    near = w.within(np.where(np.isfinite(o), o, F(0)), rq) & valid & np.isfinite(o).all(axis=1)
    assert (got.t[near] == 0).all(), "within(origin, radius) without t == 0"
    if converse:
        _same(got.t == 0, near, "t == 0 against within")
    return want, winst


def check_closed(sc, o, d, r, tmax, want, winst, insts=None):
    """every hit again with tmax = t (the same record) and with the float before t (a miss; a t = 0 hit unchanged)"""
    n = want.shape[0]
    r, tm = (np.broadcast_to(np.asarray(x, F), (n,)).astype(F) for x in (r, tmax))
    t, hit = want[:, 2], np.isfinite(want[:, 2])
    at = sc.world.sphereCast(o, d, r, np.where(hit, t, tm))
    _same(at.buffer.view(U), want.view(U), "tmax = t")
    _same(at.geom, winst, "tmax = t: geom")
    before = sc.world.sphereCast(o, d, r, np.where(hit & (t > 0), np.nextafter(t, F(0)), np.where(hit, t, tm)))
    gone = hit & (t > 0)
    assert gone.sum() > 0 and np.isinf(before.t[gone]).all() and (before.tri[gone] == -1).all() and (before.geom[gone] == -1).all()
    _same(before.buffer[~gone].view(U), want[~gone].view(U), "tmax = the float before t, t = 0 hits and misses")
    _same(before.geom[~gone], winst[~gone], "tmax = the float before t: geom")


def check_from_contact(sc, o, d, r, want, insts, most=384):
    """hits with t > 0 issued again from where they ended, fl(origin + t dn), along the same direction: the sphere rests on a
    triangle within rounding of its radius and moves into it, so it touches at once or a rounding later, and equals the model
    bit for bit as everything else (these starts ARE built onto dist == radius: the converse of within is not asserted)"""
    n = want.shape[0]
    r = np.broadcast_to(np.asarray(r, F), (n,)).astype(F)
    k = np.nonzero(np.isfinite(want[:, 2]) & (want[:, 2] > 0) & (r > 0))[0][:most]
    dn = Q.normalize3(np.ascontiguousarray(d, F)[k])
    o2 = (np.ascontiguousarray(o, F)[k] + want[k, 2:3] * dn).astype(F)
    again, _ = check_sweeps(sc, o2, dn, r[k], np.inf, insts, converse=False)
    assert k.size > 30 and np.isfinite(again[:, 2]).mean() > 0.9 and (again[:, 2] == 0).sum() > k.size // 4


def _soup(seed, n, spread=1.0, size=0.15):
    rng = np.random.RandomState(seed)
    c = rng.uniform(-spread, spread, (n, 1, 3))
    return (c + rng.uniform(-size, size, (n, 3, 3))).astype(F)


def _sweeps(rng, n, spread, rmax):
    """sweeps through a world of half-width `spread`: origins in and around it, directions of any length towards points of it,
    radii over 1e-3 .. rmax, half of them with a finite tmax; the first ten invalid"""
    o = rng.uniform(-spread - 1.5, spread + 1.5, (n, 3))
    d = (rng.uniform(-spread, spread, (n, 3)) - o) * 10.0 ** rng.uniform(-2, 2, (n, 1))
    r = 10.0 ** rng.uniform(-3, np.log10(rmax), n)
    tm = np.where(rng.uniform(size=n) < 0.5, np.inf, rng.uniform(0, 2 * spread + 2, n))
    o, d, r, tm = o.astype(F), d.astype(F), r.astype(F), tm.astype(F)
    o[0, 0], d[1, 1], o[2, 2], d[3, 0], d[4] = np.nan, np.nan, np.inf, -np.inf, 0
    r[5], r[6], r[7], tm[8], tm[9] = np.nan, -0.5, np.inf, np.nan, -1.0
    return o, d, r, tm


def test_identity_world_of_one_equals_the_hierarchy(psm, ctx):
    """the root < 0 path: no tree, the instance is entered by every sweep; the identity moves nothing"""
    tris = _soup(61, 600, 1.0, 0.1)
    o, d, r, tm = _sweeps(np.random.RandomState(62), 2048, 1.0, 0.3)
    with _World(psm, ctx, [tris], [(0, NQ.IDENTITY)]) as sc:
        th, w = sc.ths[0], sc.world
        a, b = w.sphereCast(o, d, r, tm), th.sweepSphere(o, d, r, tm)
        _same(a.buffer.view(U), b.buffer.view(U), "sphereCast against sweepSphere")
        assert np.array_equal(a.geom, np.where(b.tri >= 0, 0, -1))
        _same(w.sphereCastOccluded(o, d, r, tm), th.sweepOccluded(o, d, r, tm), "occluded")
        want, _ = check_sweeps(sc, o, d, r, tm)
        assert np.isinf(want[:10, 2]).all() and np.isfinite(want[:, 2]).sum() > 500 and np.isinf(want[:, 2]).sum() > 200


def test_lattice_world(psm, ctx):
    """cubes at the 48 signed axis permutations and integer translations, three of them twice: all arithmetic exact, contacts tie
    across touching and coincident cubes; the lowest (instance, triangle) has them"""
    model = lattice_world()
    rng = np.random.RandomState(63)
    n = 1536
    o = (rng.randint(-6, 9, (n, 3)) / 2.0).astype(F)
    dirs = np.concatenate([np.eye(3), -np.eye(3), [[1, 1, 0], [0, -1, 1], [1, 0, -1], [1, 1, 1], [-1, 1, -1], [0, 2, 0]]]).astype(F)
    d = dirs[rng.randint(0, dirs.shape[0], n)]
    r = (rng.randint(0, 9, n) / 8.0).astype(F)
    tm = rng.choice(np.array([np.inf, np.inf, 0.5, 1.0, 4.0], F), n)
    with _World(psm, ctx, [cube()], [(0, m[2]) for m in model]) as sc:
        assert sc.ths[0].info().leaf_count == 12
        insts = sc.insts()
        want, winst = check_sweeps(sc, o, d, r, tm, insts)
        t = want[:, 2]
        assert np.isfinite(t).sum() > 500 and np.isinf(t).sum() > 50 and (t == 0).sum() > 50 and (np.isfinite(t) & (t > 0)).sum() > 100
        assert np.isin(winst, (0, 1, 2)).any() and not np.isin(winst, (48, 49, 50)).any()        # coincident: the lowest instance
        check_closed(sc, o, d, r, tm, want, winst, insts)


def _members():
    deep, _, _ = Q.deep_fixture()
    return [IQ.icosphere(0, 0.6), _soup(64, 24, 0.8, 0.3), deep]


def _rigid_entries(n, seed):
    """n random rigid poses, every second a reflection, of the small members; the deep member (1 344 leaves: the spill path)
    stands first in the worlds of 2 and 33"""
    rng = np.random.RandomState(seed)
    spread = max(1.0, n ** (1.0 / 3.0))
    return [(2 if k == 0 and n < 100 else k % 2, NQ.random_pose(rng, reflect=bool(k & 1), shift=spread)) for k in range(n)], spread


@pytest.mark.parametrize("n", [2, 33, 257])
def test_world_sweep_parity_with_the_flat_answer(psm, ctx, n):
    entries, spread = _rigid_entries(n, 400 + n)
    rng = np.random.RandomState(n)
    count = 512 if n < 100 else 256                                     # (the yardstick pays for every pair)
    o, d, r, tm = _sweeps(rng, count, spread, spread)                   # radii up to half the world
    r[10:26] = 0
    tm[26:42] = 0
    with _World(psm, ctx, _members(), entries) as sc:
        insts = sc.insts()
        for j, (tris, leaves, pose) in enumerate(insts[:8]):            # origins on posed vertices: t = 0
            v = NQ.to_world(pose, tris[np.sort(leaves)[:4], 0]).astype(F)
            o[42 + 4 * j:46 + 4 * j] = v
            r[42 + 4 * j:46 + 4 * j] = np.maximum(r[42 + 4 * j:46 + 4 * j], F(1e-2))
            tm[42 + 4 * j:46 + 4 * j] = np.inf
        o[80], r[80], tm[80] = 0, 4 * spread + 8, np.inf                 # one sweep whose radius reaches every instance
        want, winst = check_sweeps(sc, o, d, r, tm, insts)
        t = want[:, 2]
        assert np.isinf(t[:10]).all() and (winst[:10] == -1).all()
        assert (t[42:42 + 4 * min(n, 8)] == 0).all() and (winst[42:42 + 4 * min(n, 8)] >= 0).all()
        assert t[80] == 0 and winst[80] == 0 and want.view(np.int32)[80, 3] == np.sort(insts[0][1])[0]   # all tie at 0: the lowest pair
        assert (t[26:42][np.isfinite(t[26:42])] == 0).all()
        assert np.isfinite(t[81:]).sum() > 60 and np.isinf(t[81:]).sum() > 20 and (np.isfinite(t[81:]) & (t[81:] > 0)).sum() > 30
        assert len(np.unique(winst)) > min(n, 24) // 2
        if n < 100:
            assert sc.ths[2].info().leaf_count > 900
        check_closed(sc, o, d, r, tm, want, winst, insts)
        check_from_contact(sc, o, d, r, want, insts, 256 if n < 100 else 128)


def test_two_coincident_instances_tie_to_the_lowest(psm, ctx):
    rng = np.random.RandomState(65)
    pose = NQ.random_pose(rng, reflect=True, shift=1.0)
    o, d, r, tm = _sweeps(rng, 1024, 1.5, 0.5)
    with _World(psm, ctx, [_soup(66, 120, 1.0, 0.2)], [(0, NQ.random_pose(rng, shift=4.0)), (0, pose), (0, pose.copy())]) as sc:
        want, winst = check_sweeps(sc, o, d, r, tm)
        assert (winst == 1).sum() > 200 and not (winst == 2).any()
        sc.world.setInstances([(sc.ths[0], pose)])                         # and a world of the one pose gives the same records
        sc.which = [0]
        alone, ainst = check_sweeps(sc, o, d, r, tm)
        k = winst == 1
        _same(alone[k].view(U), want[k].view(U), "the coincident pose alone")
        assert (ainst[k] == 0).all()


def test_a_member_far_from_its_origin(psm, ctx):
    """object coordinates at +1000, the pose brings the body back; beside it the same body at -1000 taken out to +2000"""
    rng = np.random.RandomState(67)
    near = _soup(68, 100, 1.0, 0.15)
    far = (near + F(1000)).astype(F)
    r0, r1 = _rotation(rng), _rotation(rng, True)
    entries = [(0, _pose(r0, -r0 @ np.full(3, 1000.0))), (1, _pose(r1, r1 @ np.full(3, 1000.0) + 2000.0)), (1, NQ.IDENTITY)]
    with _World(psm, ctx, [far, (near - F(1000)).astype(F)], entries) as sc:
        insts = sc.insts()
        o, d, r = [], [], []
        for tris, leaves, pose in insts:
            v = NQ.to_world(pose, tris[np.sort(leaves)].reshape(-1, 3))
            c = v.mean(0)
            start = c + rng.normal(size=(300, 3)) * 2.0
            o.append(start)
            d.append(v[rng.randint(0, v.shape[0], 300)] + rng.normal(size=(300, 3)) * 0.1 - start)
            r.append(10.0 ** rng.uniform(-3, -0.5, 300))
        o, d, r = np.concatenate(o).astype(F), np.concatenate(d).astype(F), np.concatenate(r).astype(F)
        want, winst = check_sweeps(sc, o, d, r, np.inf, insts)
        for j in range(3):
            part = slice(300 * j, 300 * (j + 1))
            assert (winst[part] == j).sum() > 100 and (np.isfinite(want[part, 2]) & (want[part, 2] > 0)).sum() > 80
        check_closed(sc, o, d, r, np.inf, want, winst, insts)


def test_an_instance_in_which_the_moved_sweep_overflows_is_skipped(psm, ctx):
    """origin - T overflows in the first instance and is small in the second: the second alone answers"""
    rng = np.random.RandomState(69)
    big = F(2e38)
    n = 256
    o = np.tile(np.array([[big, 0, 0]], F), (n, 1))
    d = rng.normal(size=(n, 3)).astype(F)
    r = (10.0 ** rng.uniform(-2, 0, n)).astype(F)
    with _World(psm, ctx, [_soup(70, 50, 1.0, 0.3)], [(0, _pose(np.eye(3), (-big, 0, 0))), (0, _pose(np.eye(3), (big, 0, 0)))]) as sc:
        with np.errstate(all="ignore"):
            want, winst = check_sweeps(sc, o, d, r, np.inf)
        assert (winst == 1).sum() > 30 and not (winst == 0).any()


def test_tiny_members_and_the_empty_world(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    degenerate = np.repeat(tri[:, :1], 3, axis=1)                    # three equal vertices: the build keeps no leaf
    meshes = [np.concatenate([degenerate] * 4), np.concatenate([degenerate, tri, degenerate]),
              np.concatenate([tri, degenerate, tri + F([0.5, 0, 0])])]
    rng = np.random.RandomState(71)
    entries = [(k % 3, NQ.random_pose(rng, reflect=bool(k & 2), shift=1.5)) for k in range(12)]
    o, d, r, tm = _sweeps(rng, 600, 2.0, 1.0)
    with _World(psm, ctx, meshes, entries) as sc:
        assert [th.info().leaf_count for th in sc.ths] == [0, 1, 2]
        want, winst = check_sweeps(sc, o, d, r, tm)
        assert np.isfinite(want[:, 2]).sum() > 100 and np.isinf(want[:, 2]).sum() > 100 and not np.isin(winst, (0, 3, 6, 9)).any()
        for one in range(3):                                          # worlds of one: no tree, the instance is entered by every sweep
            sc.world.setInstances([(sc.ths[one], entries[one][1])])
            sc.which = [one]
            w1, _ = check_sweeps(sc, o, d, r, tm)
            assert np.isfinite(w1[:, 2]).any() == (one > 0)
        sc.world.setInstances([])                                     # the empty world answers without a tree
        sc.which = []
        assert len(sc.world) == 0
        got = sc.world.sphereCast(o, d, r, tm)
        assert np.isinf(got.t).all() and (got.tri == -1).all() and (got.geom == -1).all() and not got.u.any() and not got.v.any()
        assert not sc.world.sphereCastOccluded(o, d, r, tm).any()


@pytest.mark.parametrize("n", [1, 63, 65, GRID_CAP * 64 + 65])
def test_world_sweep_batch_sizes(psm, ctx, n):
    """the last size takes a second trip of the grid-stride loop: the best record must start at tmax and no instance again"""
    rng = np.random.RandomState(72)
    c = rng.uniform(-1, 1, (3, 1, 3))                                 # (few triangles: the yardstick is n x 2 x 3 pairs)
    tris = (c + rng.uniform(-0.5, 0.5, (3, 3, 3))).astype(F)
    entries = [(0, NQ.random_pose(rng, reflect=bool(k & 1), shift=1.0)) for k in range(2)]
    rng = np.random.RandomState(n % 1000)
    o = rng.uniform(-2.5, 2.5, (n, 3)).astype(F)
    d = (rng.uniform(-1.2, 1.2, (n, 3)) - o).astype(F)
    r = rng.uniform(0.0, 0.3, n).astype(F)
    tm = np.where(rng.uniform(size=n) < 0.5, rng.uniform(0, 3, n), np.inf).astype(F)
    with _World(psm, ctx, [tris], entries) as sc:
        want, winst = check_sweeps(sc, o, d, r, tm)
        if n > 1000:
            assert len(np.unique(winst)) == 3 and len(np.unique(winst[-65:])) == 3 and len(np.unique(want.view(np.int32)[-65:, 3])) > 2


@pytest.mark.parametrize("opt", [ROT_SCALE, SHEAR], ids=["rotate_scale", "shear"])
def test_a_member_built_with_an_optimisation_matrix(psm, ctx, opt):
    rng = np.random.RandomState(73)
    c = rng.uniform(-1, 1, (500, 1, 3)) * [1.0, 0.3, 2.0]
    tris = (c + rng.uniform(-0.08, 0.08, (500, 3, 3))).astype(F)
    entries = [(0, NQ.random_pose(rng, reflect=bool(k & 1), shift=2.0)) for k in range(4)]
    with _World(psm, ctx, [tris], entries, [opt]) as sc:
        t = np.array(sc.ths[0].info().transform).reshape(4, 4)[:3, :3]
        assert np.abs(t - np.diag(np.diag(t))).max() > 0.01
        insts = sc.insts()
        o, d, r, tm = _sweeps(rng, 1024, 3.0, 0.3)
        # the tightest case for the prune: sweeps that pass a posed vertex at the radius, give or take a few ulps
        for j, (tr, leaves, pose) in enumerate(insts):
            part = slice(16 + 64 * j, 16 + 64 * (j + 1))
            v = NQ.to_world(pose, tr[np.sort(leaves)].reshape(-1, 3))
            q = v[rng.randint(0, v.shape[0], 64)]
            dd = rng.normal(size=(64, 3))
            dd /= np.linalg.norm(dd, axis=1, keepdims=True)
            perp = np.cross(dd, rng.normal(size=(64, 3)))
            perp /= np.linalg.norm(perp, axis=1, keepdims=True)
            o[part] = (q + perp * r[part, None] - dd * rng.uniform(0.2, 1.5, (64, 1))).astype(F)
            d[part] = dd.astype(F)
            r[part] = (r[part] + rng.randint(-8, 9, 64) * np.spacing(r[part])).astype(F)
            tm[part] = np.inf
        want, winst = check_sweeps(sc, o, d, r, tm, insts)
        assert np.isfinite(want[:, 2]).sum() > 300 and np.isinf(want[:, 2]).sum() > 100 and len(np.unique(winst)) == 5


def test_set_transform_refit_and_refresh(psm, ctx):
    rng = np.random.RandomState(74)
    a, b = _soup(75, 80, 1.0, 0.2), _soup(76, 60, 1.0, 0.2)
    entries = [(k % 2, NQ.random_pose(rng, reflect=bool(k & 1), shift=2.0)) for k in range(9)]
    o, d, r, tm = _sweeps(rng, 1024, 3.0, 0.5)
    with _World(psm, ctx, [a, b], entries) as sc:
        before, _ = check_sweeps(sc, o, d, r, tm)
        sc.world.setTransform(3, NQ.random_pose(rng, shift=2.0))
        sc.world.setTransforms(5, [NQ.random_pose(rng, reflect=True, shift=2.0), NQ.random_pose(rng, shift=2.0)])
        after, _ = check_sweeps(sc, o, d, r, tm)
        assert (before.view(U) != after.view(U)).any()
        # a rebuilt member is stale: refused by message
        h = sc.ths[1]
        h.markDirty()
        h.build()
        with pytest.raises(psm.PsmError, match="psm_world_sweep_sphere_dev: instance 1's hierarchy was rebuilt"):
            sc.world.sphereCast(o, d, r, tm)
        with pytest.raises(psm.PsmError, match="psm_world_sweep_occluded_dev: instance 1's hierarchy was rebuilt"):
            sc.world.sphereCastOccluded(o, d, r, tm)
        sc.world.setInstances([(sc.ths[k], m) for k, m in zip(sc.which, sc.world.transforms())])
        # a refit: the triangles move within the build's bounds; after refresh() the answers are exact again
        blo, bhi = b.reshape(-1, 3).min(0), b.reshape(-1, 3).max(0)
        moved = b.copy()
        k = rng.choice(b.shape[0], 10, replace=False)
        cc = moved[k].mean(axis=1, keepdims=True)
        moved[k] = np.clip(cc + (moved[k] - cc) * F(0.5) + rng.uniform(-0.3, 0.3, (10, 1, 3)).astype(F), blo, bhi).astype(F)
        h.clearTribuffer()
        h.loadTriangles(moved.reshape(-1, 9))
        h.refit()
        sc.world.refresh()
        sc.meshes[1] = moved
        refit, _ = check_sweeps(sc, o, d, r, tm)
        assert (refit.view(U) != after.view(U)).any()


def test_world_sweep_refusals_launch_nothing(psm, ctx):
    """a stale world, NULL and misaligned pointers and mismatched arguments are refused on the host by their messages: the outputs
    keep what they held"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    n = 4
    with _World(psm, ctx, [tri, tri + F(1)], [(0, NQ.IDENTITY), (1, NQ.IDENTITY)]) as sc:
        w = sc.world._w
        hin, hout, hinst, hbyte = ctx.buf_alloc(32 * n + 32), ctx.buf_alloc(16 * n + 32), ctx.buf_alloc(4 * n + 16), ctx.buf_alloc(16)
        try:
            sweeps = np.zeros((n, 8), F)
            sweeps[:, 0:4], sweeps[:, 4:8] = [-1, 0, 0, 0.25], [1, 0, 0, np.inf]
            ctx.buf_upload(hin, np.concatenate([sweeps.reshape(-1), np.zeros(8, F)]))
            ctx.buf_upload(hout, np.full(4 * n + 8, 7, np.int32))
            ctx.buf_upload(hinst, np.full(n + 4, 9, np.int32))
            ctx.buf_upload(hbyte, np.full(16, 77, np.uint8))
            pin, pout, pinst, pbyte = (ctypes.c_void_p(ctx.buf_ptr(h)[0]) for h in (hin, hout, hinst, hbyte))
            size = ctypes.c_size_t(n)

            def cast(p_in=pin, p_out=pout, p_inst=pinst, count=size):
                return lib.psm_world_sweep_sphere_dev(w, p_in, count, p_out, p_inst)

            def occluded(p_in=pin, p_out=pbyte, count=size):
                return lib.psm_world_sweep_occluded_dev(w, p_in, count, p_out)
            assert cast(p_in=None) == -1 and cast(p_out=None) == -1
            assert cast(p_inst=None) == -1 and b"psm_world_sweep_sphere_dev: NULL pointer" in lib.psm_last_error(ctx._h)
            assert cast(p_in=ctypes.c_void_p(pin.value + 4)) == -1 and b"sweeps or hits not 16-byte aligned" in lib.psm_last_error(ctx._h)
            assert cast(p_out=ctypes.c_void_p(pout.value + 8)) == -1 and b"sweeps or hits not 16-byte aligned" in lib.psm_last_error(ctx._h)
            assert cast(p_inst=ctypes.c_void_p(pinst.value + 2)) == -1 and b"inst not 4-byte aligned" in lib.psm_last_error(ctx._h)
            assert occluded(p_in=None) == -1 and occluded(p_out=None) == -1
            assert occluded(p_in=ctypes.c_void_p(pin.value + 8)) == -1 and b"psm_world_sweep_occluded_dev: sweeps not 16-byte aligned" in lib.psm_last_error(ctx._h)
            assert cast(count=ctypes.c_size_t(0)) == 0 and occluded(count=ctypes.c_size_t(0)) == 0
            o = np.zeros((3, 3), F)
            for call in (sc.world.sphereCast, sc.world.sphereCastOccluded):
                with pytest.raises(ValueError, match="3 against 2"):
                    call(o, o[:2], 0.5)
                with pytest.raises(ValueError):
                    call(o, o, np.zeros(2, F))
            sc.ths[1].markDirty()
            sc.ths[1].build()                                          # stale: PSM_ERR_STATE
            assert cast() == -5 and b"psm_world_sweep_sphere_dev: instance 1's hierarchy was rebuilt" in lib.psm_last_error(ctx._h)
            assert occluded() == -5 and b"psm_world_sweep_occluded_dev: instance 1's hierarchy was rebuilt" in lib.psm_last_error(ctx._h)
            ctx.sync()
            assert (ctx.buf_download(hout, np.int32, 4 * n + 8) == 7).all() and (ctx.buf_download(hinst, np.int32, n + 4) == 9).all()
            assert (ctx.buf_download(hbyte, np.uint8, 16) == 77).all()
            sc.world.setInstances([(sc.ths[0], NQ.IDENTITY), (sc.ths[1], NQ.IDENTITY)])
            w = sc.world._w
            assert cast() == 0 and occluded() == 0                     # and the same buffers are fine
            ctx.sync()
            rec = ctx.buf_download(hout, np.int32, 4 * n + 8)
            assert (rec[:4 * n].reshape(n, 4)[:, 3] == 0).all() and (rec[:4 * n].view(F).reshape(n, 4)[:, 2] == 1.75).all() and (rec[4 * n:] == 7).all()
            inst = ctx.buf_download(hinst, np.int32, n + 4)
            assert (inst[:n] == 0).all() and (inst[n:] == 9).all()
            byte = ctx.buf_download(hbyte, np.uint8, 16)
            assert (byte[:n] == 1).all() and (byte[n:] == 77).all()
        finally:
            for h in (hin, hout, hinst, hbyte):
                ctx.buf_free(h)


def test_world_sweep_torch_tensors_on_a_side_stream(psm, ctx):
    if torch is None:
        pytest.skip("torch is not installed")
    rng = np.random.RandomState(77)
    entries = [(k % 2, NQ.random_pose(rng, reflect=bool(k & 1), shift=3.0)) for k in range(40)]
    n = 4099
    o, d, r, tm = _sweeps(rng, n, 3.0, 0.5)
    with _World(psm, ctx, [IQ.icosphere(1, 0.6), _soup(78, 150, 0.8, 0.2)], entries) as sc:
        w = sc.world
        hits, flag, scalar = w.sphereCast(o, d, r, tm), w.sphereCastOccluded(o, d, r, tm), w.sphereCast(o, d, 0.05, 2.5)
        assert flag.any() and not flag.all()
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            to, td, tr, tt = (torch.from_numpy(x).to(dev, non_blocking=True) for x in (o, d, r, tm))
            ghits, gflag, gscalar = w.sphereCast(to, td, tr, tt), w.sphereCastOccluded(to, td, tr, tt), w.sphereCast(to, td, 0.05, 2.5)
            bufs = [x.cpu() for x in (ghits.buffer, ghits.geom, gflag, gscalar.buffer, gscalar.geom)]   # (on the side stream: in order)
        assert ghits.buffer.device == dev and ghits.buffer.shape == (n, 4) and ghits.tri.dtype == torch.int32
        assert ghits.geom.shape == (n,) and ghits.geom.dtype == torch.int32 and gflag.device == dev and gflag.dtype == torch.bool
        _same(bufs[0].numpy().view(U), hits.buffer.view(U), "torch sphereCast")
        _same(bufs[1].numpy(), hits.geom, "torch sphereCast geom")
        _same(bufs[2].numpy(), flag, "torch sphereCastOccluded")
        _same(bufs[3].numpy().view(U), scalar.buffer.view(U), "torch sphereCast, scalar radius and tmax")
        _same(bufs[4].numpy(), scalar.geom, "torch sphereCast geom, scalar radius and tmax")
