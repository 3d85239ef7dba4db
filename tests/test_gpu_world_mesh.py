"""The mesh queries of an instance world on the GPU (psm_world_mesh_overlaps_dev / psm_world_mesh_count_dev /
psm_world_mesh_triangles_dev, world_mesh.hip; InstanceWorld.overlapsMesh / countOnMesh / trianglesOnMesh). The
yardsticks are tests/world_mesh_query_model.py -- the other hierarchy's stored leaves posed in numpy float32, then tri_tri by brute
force over the forward-posed downloaded leaves of every instance -- and the contract's own statement: countOnTriangle /
trianglesOnTriangle of the same host-posed triangles on the same world. Every comparison is exact on every (pose, triangle), and
in every case the three queries are also held against one another: flag == any(count > 0), the rows' count == min(k, count), the
live slots are the non-negative ones in both arrays, the rows are prefixes."""
import ctypes
import os

import numpy as np
import pytest

import instance_query_model as NQ
import mesh_query_model as MQ
import world_mesh_query_model as WM
from test_gpu_box_query import GRID_CAP, ROT_SCALE, SHEAR
from test_gpu_world_box import KS, _World, _hier, _same, _soup
from test_world_box_cpu import _pose, cube, lattice_world, signed_permutations

try:   # (imported before the library loads its HIP runtime, as tests/test_gpu_query.py)
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
U = np.uint32
POINT = np.repeat(F([[[0.25, 0.25, 0.25]]]), 3, axis=1)   # three equal vertices: the build keeps no leaf


def _leaves(psm, th):
    return np.sort(th.download(psm.BVH_LEAF_TRI, np.int32, th.info().leaf_count))


def check_mesh(sc, other, otris, poses, ks=KS, skip=None, insts=None, model=True):
    """the three queries against the model (computed once at the largest k: its rows are prefixes, test_world_mesh_cpu) -- or, where
    `model` is False, against countOnTriangle / trianglesOnTriangle of the same float32-posed triangles on the same world -- and
    against one another; returns the flag, the full count, the triangle rows and the instance rows at the largest k"""
    w, psm = sc.world, sc.psm
    otris = np.ascontiguousarray(otris, F).reshape(-1, 3, 3)
    p, t, kmax = MQ.poses12(poses).shape[0], otris.shape[0], max(ks)
    oleaves = _leaves(psm, other)
    if model:
        flag, count, trows, irows, _ = WM.query(sc.insts() if insts is None else insts, otris, oleaves, poses, kmax, skip)
    else:
        assert skip is None
        q = MQ.posed(otris, poses)
        count, trows, irows = np.zeros((p, t), U), np.full((p, t, kmax), -1, np.int32), np.full((p, t, kmax), -1, np.int32)
        if oleaves.size:
            packed = q[:, oleaves].reshape(-1, 3, 3)
            count[:, oleaves] = w.countOnTriangle(packed).reshape(p, -1)
            lists = w.trianglesOnTriangle(packed, kmax)
            trows[:, oleaves], irows[:, oleaves] = lists.tri.reshape(p, -1, kmax), lists.geom.reshape(p, -1, kmax)
        flag = (count > 0).any(axis=1)
    got_flag, got_count = w.overlapsMesh(other, poses, skip=skip), w.countOnMesh(other, poses, skip=skip)
    assert got_flag.shape == (p,) and got_flag.dtype == np.bool_ and got_count.shape == (p, t) and got_count.dtype == U
    _same(got_flag, flag, "overlapsMesh")
    _same(got_count, count, "countOnMesh")
    assert np.array_equal(got_flag, (got_count > 0).any(axis=1))
    widest = None
    for k in sorted(ks, reverse=True):
        got = w.trianglesOnMesh(other, poses, k, skip=skip)
        assert got.tri.shape == (p, t, k) and got.tri.dtype == np.int32 and got.geom.shape == (p, t, k) and got.geom.dtype == np.int32
        assert got.count.shape == (p, t) and got.count.dtype == U
        _same(got.tri, trows[:, :, :k], "trianglesOnMesh tri, k = %d" % k)
        _same(got.geom, irows[:, :, :k], "trianglesOnMesh inst, k = %d" % k)
        _same(got.count, np.minimum(got_count, U(k)), "trianglesOnMesh count against countOnMesh, k = %d" % k)
        live = np.arange(k)[None, None] < got.count[:, :, None]
        assert np.array_equal(got.tri >= 0, live) and np.array_equal(got.geom >= 0, live)
        if widest is None:
            widest = got
        _same(got.tri, widest.tri[:, :, :k], "trianglesOnMesh k = %d is a prefix" % k)
        _same(got.geom, widest.geom[:, :, :k], "trianglesOnMesh inst k = %d is a prefix" % k)
    return flag, count, trows, irows


def rotations(rng, n):
    """n random rotations and reflections (alternating), float64, from unit quaternions"""
    q = rng.normal(size=(n, 4))
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    r = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)
    r[1::2, :, 0] = -r[1::2, :, 0]
    return r


def general_poses(rng, p, lo=-3.0, hi=1.0):
    """p rigid poses, rotations and reflections alternating, translations of length 10^lo .. 10^hi"""
    shift = rng.normal(size=(p, 3))
    shift *= (10.0 ** np.linspace(lo, hi, p) / np.linalg.norm(shift, axis=1))[:, None]
    return [_pose(r, t) for r, t in zip(rotations(rng, p), shift)]


# ---- 1: an identity world of one is the member's own mesh query --------------------------------------------------------------------

def test_identity_world_of_one_answers_as_the_mesh_queries(psm, ctx):
    rng = np.random.RandomState(91)
    tris = _soup(92, 300, 1.0, 0.25)
    otris = np.concatenate([_soup(93, 40, 0.7, 0.3), POINT, _soup(94, 40, 0.7, 0.3)])
    poses = general_poses(rng, 5, -3.0, 0.5)
    with _World(psm, ctx, [tris], [(0, NQ.IDENTITY)]) as sc:
        other = _hier(psm, ctx, otris)
        try:
            th, w = sc.ths[0], sc.world
            flag, count = th.meshOverlaps(other, poses), th.meshCount(other, poses)
            assert flag.any() and (count > 0).sum() > 50 and (count[:, 40] == 0).all()
            _same(w.overlapsMesh(other, poses), flag, "overlaps")
            _same(w.countOnMesh(other, poses), count, "count")
            for k in (1, 4, 16):
                a, b = w.trianglesOnMesh(other, poses, k), th.meshTriangles(other, poses, k)
                _same(a.tri, b.tri, "rows k = %d" % k)
                _same(a.count, b.count, "rows' count k = %d" % k)
                assert np.array_equal(a.geom, np.where(b.tri >= 0, 0, -1))
            # and the member against its own world at the identity: every leaf meets at least itself
            own = w.trianglesOnMesh(th, NQ.IDENTITY, 16)
            _same(own.tri, th.meshTriangles(th, NQ.IDENTITY, 16).tri, "the member itself")
            assert (own.count[0, _leaves(psm, th)] >= 1).all()
        finally:
            other.close()


# ---- 2: the lattice, every operation exact -----------------------------------------------------------------------------------------

def test_lattice_world_and_a_lattice_mesh(psm, ctx):
    """cubes at the 48 signed axis permutations and integer translations, three of them twice; an integer-vertex mesh at signed
    permutations with integer translations: all arithmetic exact. Against the model and against the world's triangle queries of
    the host-posed triangles; coincident instances are listed lowest instance first"""
    rng = np.random.RandomState(95)
    model = lattice_world()
    otris = np.concatenate([rng.randint(-1, 3, (40, 1, 3)) + rng.randint(-1, 2, (40, 3, 3)), np.ones((1, 3, 3)), rng.randint(0, 2, (20, 3, 3))]).astype(F)
    perms = signed_permutations()
    poses = [_pose(perms[j], t) for j, t in zip((0, 7, 18, 29, 40, 47), ([0, 0, 0], [1, 0, -1], [0, 2, 1], [-1, -1, 0], [2, 2, 2], [40, 0, 0]))]
    with _World(psm, ctx, [cube()], [(0, m[2]) for m in model]) as sc:
        other = _hier(psm, ctx, otris)
        try:
            assert sc.ths[0].info().leaf_count == 12 and 40 not in _leaves(psm, other)
            flag, count, trows, irows = check_mesh(sc, other, otris, poses)
            assert flag[:5].all() and not flag[5] and (count > 16).any() and ((count > 0) & (count < 16)).any()
            assert (count[:, 40] == 0).all() and (trows[:, 40] == -1).all() and (irows[:, 40] == -1).all()
            f2, c2, t2, i2 = check_mesh(sc, other, otris, poses, (3, 16), model=False)
            assert np.array_equal(c2, count) and np.array_equal(t2, trows) and np.array_equal(i2, irows)
            # coincident instances, in a world small enough for whole rows: a cube, another, and the first again
            sc.world.setInstances([(sc.ths[0], model[j][2]) for j in (0, 5, 0)])
            sc.which = [0, 0, 0]
            _, count, trows, irows = check_mesh(sc, other, otris, poses, (16,))
            both = np.argwhere((irows == 0).any(axis=2) & (count <= 16))
            assert both.shape[0] > 5
            for q, t in both[:20]:
                assert list(trows[q, t][irows[q, t] == 0]) == list(trows[q, t][irows[q, t] == 2])
                live = irows[q, t][irows[q, t] >= 0]
                assert list(live) == sorted(live)
        finally:
            other.close()


# ---- 3: general poses, worlds of 2, 33 and 257 ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 33, 257])
def test_world_mesh_parity_with_the_flat_answer(psm, ctx, n):
    """n rigid poses (every second a reflection) of a 130-triangle mesh, the last standing exactly where the first stands; a
    60-triangle mesh at 3 poses, rotations and reflections, translated by 1e-3 .. 10"""
    rng = np.random.RandomState(300 + n)
    member = _soup(96, 130, 0.8, 0.25)
    spread = max(1.0, n ** (1.0 / 3.0))
    entries = [(0, NQ.random_pose(rng, reflect=bool(k & 1), shift=spread)) for k in range(n)]
    entries[-1] = (0, entries[0][1].copy())                                 # coincident instances
    otris = (_soup(97, 60, 0.7, 0.3) * F(1.0 if n == 2 else 2.0)).astype(F)
    otris[59] = [[-20, -20, 0.1], [20, -20, -0.1], [0, 20, 0.05]]           # the last one cuts through whatever stands near its pose
    poses = general_poses(rng, 3)
    poses[0][:, 3] += entries[0][1][:, 3]                                   # pose 0 sits on instance 0 (and n - 1)
    with _World(psm, ctx, [member], entries) as sc:
        other = _hier(psm, ctx, otris)
        try:
            assert 120 <= sc.ths[0].info().leaf_count <= 130 and other.info().leaf_count >= 55
            insts = sc.insts()
            flag, count, trows, irows = check_mesh(sc, other, otris, poses, KS, None, insts)
            assert flag[0] and (count > 16).any() and ((count > 0) & (count <= 16)).sum() > 10 and (count == 0).any()
            pairs = np.argwhere((irows == 0).any(axis=2) & (count <= 16))
            assert pairs.shape[0] > 0
            for q, t in pairs:                                              # the coincident pair: the same triangles, the lowest first
                assert list(trows[q, t][irows[q, t] == 0]) == list(trows[q, t][irows[q, t] == n - 1])
            c2 = check_mesh(sc, other, otris, poses, (16,), model=False)[1]
            assert np.array_equal(c2, count)
        finally:
            other.close()


# ---- 4: the other mesh's leaf counts ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("leaves", [1, 63, 64, 65])
@pytest.mark.parametrize("p", [1, 3])
def test_world_mesh_other_sizes(psm, ctx, leaves, p):
    rng = np.random.RandomState(100 * leaves + p)
    entries = [(0, NQ.random_pose(rng, reflect=bool(k & 1), shift=0.6)) for k in range(5)]
    otris = np.concatenate([POINT, _soup(1000 + leaves, leaves, 0.8, 0.3)])            # a dropped triangle first
    poses = [_pose(r, t) for r, t in zip(rotations(rng, p), rng.uniform(-0.3, 0.3, (p, 3)))]
    with _World(psm, ctx, [_soup(98, 100, 0.8, 0.25)], entries) as sc:
        other = _hier(psm, ctx, otris)
        try:
            assert other.info().leaf_count == leaves
            flag, count, trows, _ = check_mesh(sc, other, otris, poses, (2, 16))
            assert (count[:, 0] == 0).all() and (trows[:, 0] == -1).all() and (leaves == 1 or (flag.all() and (count == 0).any()))
        finally:
            other.close()


def test_world_mesh_dropped_triangles_and_a_mesh_without_leaves(psm, ctx):
    rng = np.random.RandomState(99)
    entries = [(0, NQ.random_pose(rng, reflect=bool(k & 1), shift=0.5)) for k in range(4)]
    soup = _soup(101, 9, 0.6, 0.5)
    otris = np.concatenate([POINT, soup[:3], POINT, POINT, soup[3:], POINT])
    poses = general_poses(rng, 2, -2.0, -0.5)
    with _World(psm, ctx, [_soup(102, 100, 0.8, 0.25)], entries) as sc:
        other, empty = _hier(psm, ctx, otris), _hier(psm, ctx, np.concatenate([POINT] * 3))
        try:
            assert list(_leaves(psm, other)) == [1, 2, 3, 6, 7, 8, 9, 10, 11] and empty.info().leaf_count == 0
            flag, count, trows, irows = check_mesh(sc, other, otris, poses, (1, 16))
            assert flag.all() and not count[:, [0, 4, 5, 12]].any() and (trows[:, [0, 4, 5, 12]] == -1).all() and (irows[:, [0, 4, 5, 12]] == -1).all()
            f0, c0, t0, i0 = check_mesh(sc, empty, np.concatenate([POINT] * 3), poses, (4,))
            assert not f0.any() and not c0.any() and (t0 == -1).all() and (i0 == -1).all()
        finally:
            other.close()
            empty.close()


# ---- 5: the grid-stride loop and the flag kernel's skip ------------------------------------------------------------------------------------

def test_world_mesh_grid_stride_second_trip(psm, ctx):
    """p x L just above PSM_QUERY_GRID_CAP x 64 + 65 against a world of two tiny members: the last queries take a second trip of the
    grid-stride loop, where the count and the list must start empty again, and the flag kernel's skip is on by itself; held against
    countOnTriangle / trianglesOnTriangle of the host-posed triangles"""
    rng = np.random.RandomState(103)
    otris = np.concatenate([_soup(104, 30, 0.6, 0.5), POINT, _soup(105, 35, 0.6, 0.5)])
    leaves = 65
    p = -(-(GRID_CAP * 64 + 65) // leaves)
    assert GRID_CAP * 64 + 65 <= p * leaves < GRID_CAP * 64 + 65 + leaves
    poses = np.concatenate([rotations(rng, p), rng.uniform(-1.5, 1.5, (p, 3, 1))], axis=2)
    entries = [(0, NQ.random_pose(rng, shift=0.5)), (1, NQ.random_pose(rng, reflect=True, shift=0.5))]
    with _World(psm, ctx, [_soup(106, 8, 0.5, 0.5), _soup(107, 7, 0.5, 0.5)], entries) as sc:
        other = _hier(psm, ctx, otris)
        try:
            assert other.info().leaf_count == leaves
            flag, count, _, irows = check_mesh(sc, other, otris, poses, (2,), model=False)
            assert flag.any() and not flag.all() and (irows == 0).any() and (irows == 1).any()
            tail = count[-2:, _leaves(psm, other)]
            assert len(np.unique(count)) > 2 and len(np.unique(tail)) > 2 and (count[:, 30] == 0).all()
        finally:
            other.close()


def test_world_mesh_flag_per_pose_and_the_study_knob(psm, ctx):
    """257 poses of a small lattice mesh, most far away, a handful cutting the world: the flag is per pose; with PSM_MESH_SKIP
    forced on (a launch this small leaves it off) twice the same answer, and the same with it forced off"""
    rng = np.random.RandomState(108)
    model = lattice_world()[:12]
    otris = np.concatenate([(rng.randint(-1, 2, (40, 1, 3)) + rng.randint(-1, 2, (40, 3, 3)) * 0.5), np.ones((1, 3, 3))]).astype(F)
    perms = signed_permutations()
    poses = [_pose(np.eye(3), [-40.0 - q, 0.5 * (q % 5), 0]) for q in range(257)]
    meeting = {3: (0, [0, 0, 0]), 64: (9, [1, 0, 1]), 65: (20, [0, 1, 0]), 200: (33, [1, 1, 0]), 256: (46, [0, 0, 1])}
    for q, (r, t) in meeting.items():
        poses[q] = _pose(perms[r], t)
    with _World(psm, ctx, [cube()], [(0, m[2]) for m in model]) as sc:
        other = _hier(psm, ctx, otris)
        try:
            flag, count, _, _ = check_mesh(sc, other, otris, poses, (16,))
            assert list(np.nonzero(flag)[0]) == sorted(meeting)
            for knob in ("1", "1", "0"):
                os.environ["PSM_MESH_SKIP"] = knob
                try:
                    assert np.array_equal(sc.world.overlapsMesh(other, poses), flag), knob
                    assert np.array_equal(sc.world.overlapsMesh(other, poses, skip=2), (sc.world.countOnMesh(other, poses, skip=2) > 0).any(axis=1)), knob
                finally:
                    del os.environ["PSM_MESH_SKIP"]
        finally:
            other.close()


# ---- 6: skip ------------------------------------------------------------------------------------------------------------------------------

def test_skip_leaves_one_instance_out(psm, ctx):
    """other is a member of the world at its own pose: with no skip every leaf meets at least itself in that instance; with skip =
    its index the answer is the model's without it, the other indices kept ("body i against all the others")"""
    rng = np.random.RandomState(109)
    a, b = _soup(110, 90, 0.7, 0.15), _soup(111, 60, 0.7, 0.15)
    entries = [(k % 2, NQ.random_pose(rng, reflect=bool(k & 1), shift=0.8)) for k in range(7)]
    with _World(psm, ctx, [a, b], entries) as sc:
        insts = sc.insts()
        for s in (0, 3, 6):
            body, mesh, pose = sc.ths[entries[s][0]], sc.meshes[entries[s][0]], entries[s][1]
            moved = NQ.random_pose(rng, shift=0.8)
            _, full, _, irows = check_mesh(sc, body, mesh, [pose, moved], (16,), None, insts)
            leaves = _leaves(psm, body)
            assert (full[0, leaves] >= 1).all()
            few = leaves[full[0, leaves] <= 16]
            assert few.size > 10 and (irows[0, few] == s).any(axis=1).all()
            _, without, _, irows = check_mesh(sc, body, mesh, [pose, moved], (3, 16), s, insts)
            assert not (irows == s).any() and (without[0] < full[0])[leaves].all() and without.any()
            assert (irows > s).any() or s == 6                              # the indices are kept, not renumbered


def test_skip_in_a_world_of_one_and_of_a_single_leaf_member(psm, ctx):
    rng = np.random.RandomState(112)
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    soup = _soup(113, 50, 0.8, 0.4)
    otris = np.concatenate([_soup(114, 20, 0.8, 0.5), F([[[-4, -0.5, -0.25], [4, -0.5, -0.25], [4, 0.5, 0.5]]])])   # the last: through all
    poses = [NQ.IDENTITY, NQ.random_pose(rng, shift=0.1)]
    among = [(0, NQ.IDENTITY), (1, NQ.IDENTITY), (1, _pose(np.eye(3), [0.25, 0, 0])), (0, poses[1])]
    with _World(psm, ctx, [soup, tri], among) as sc:
        other = _hier(psm, ctx, otris)
        try:
            # a single-leaf member (the lone leaf is tested where the instance is entered), among others and alone
            for entries in (among, [(1, NQ.IDENTITY)]):
                sc.world.setInstances([(sc.ths[k], m) for k, m in entries])
                sc.which = [k for k, _ in entries]
                insts = sc.insts()
                lone = sc.which.index(1)
                _, c_all, _, i_all = check_mesh(sc, other, otris, poses, (16,), None, insts)
                assert c_all[0, 20] >= 1 and (i_all[0, 20] == lone).any()
                _, c_skip, _, i_skip = check_mesh(sc, other, otris, poses, (16,), lone, insts)
                assert c_skip[0, 20] == c_all[0, 20] - 1 and not (i_skip == lone).any()
            sc.world.setInstances([(sc.ths[0], NQ.IDENTITY)])                             # a world of one: no tree
            sc.which = [0]
            flag, count, _, _ = check_mesh(sc, other, otris, poses, (4,))
            assert flag.all() and count[0, 20] >= 4
            f, c, t, i = check_mesh(sc, other, otris, poses, (4,), 0)
            assert not f.any() and not c.any() and (t == -1).all() and (i == -1).all()
        finally:
            other.close()


# ---- 7: tiny and empty worlds ---------------------------------------------------------------------------------------------------------------

def test_tiny_members_and_the_empty_world(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    degenerate = np.repeat(tri[:, :1], 3, axis=1)
    meshes = [np.concatenate([degenerate] * 4), np.concatenate([degenerate, tri, degenerate]),
              np.concatenate([tri, degenerate, tri + F([0.5, 0, 0])]), np.concatenate([tri, tri + F([0.25, 0, 0]), degenerate, tri + F([0.5, 0, 0])])]
    rng = np.random.RandomState(115)
    entries = [(k % 4, NQ.random_pose(rng, reflect=bool(k & 2), shift=1.5)) for k in range(12)]
    otris = np.concatenate([_soup(116, 40, 2.0, 1.0), POINT])
    poses = general_poses(rng, 3, -2.0, 0.0)
    with _World(psm, ctx, meshes, entries) as sc:
        other = _hier(psm, ctx, otris)
        try:
            assert [th.info().leaf_count for th in sc.ths] == [0, 1, 2, 3]
            flag, count, _, irows = check_mesh(sc, other, otris, poses, (1, 16))
            assert flag.any() and count.min() == 0 and not (irows % 4 == 0)[irows >= 0].any()
            check_mesh(sc, other, otris, poses, (16,), 5)
            for one in range(4):                                          # worlds of one: no tree, the instance is entered by every query
                sc.world.setInstances([(sc.ths[one], entries[one][1])])
                sc.which = [one]
                _, c1, _, _ = check_mesh(sc, other, otris, poses, (2,))
                assert c1.max() <= one
            sc.world.setInstances([])                                     # the empty world answers without a kernel
            sc.which = []
            assert len(sc.world) == 0
            assert not sc.world.overlapsMesh(other, poses).any() and not sc.world.countOnMesh(other, poses).any()
            got = sc.world.trianglesOnMesh(other, poses, 5)
            assert (got.tri == -1).all() and (got.geom == -1).all() and not got.count.any() and got.tri.shape == (3, 41, 5)
            with pytest.raises(psm.PsmError, match="skip must be None"):
                sc.world.countOnMesh(other, poses, skip=0)
        finally:
            other.close()


# ---- 8: transforms, refits and other trees ------------------------------------------------------------------------------------------------

def test_set_transform_refit_and_refresh(psm, ctx):
    rng = np.random.RandomState(117)
    a, b = _soup(118, 120, 1.0, 0.25), _soup(119, 90, 1.0, 0.25)
    entries = [(k % 2, NQ.random_pose(rng, reflect=bool(k & 1), shift=1.5)) for k in range(9)]
    otris = _soup(120, 60, 1.5, 0.5)
    poses = general_poses(rng, 3, -2.0, 0.3)
    with _World(psm, ctx, [a, b], entries) as sc:
        other = _hier(psm, ctx, otris)
        try:
            _, before, _, _ = check_mesh(sc, other, otris, poses, (4,))
            sc.world.setTransform(3, NQ.random_pose(rng, shift=1.5))       # no hierarchy is rebuilt
            sc.world.setTransforms(5, [NQ.random_pose(rng, reflect=True, shift=1.5), NQ.random_pose(rng, shift=1.5)])
            _, after, _, _ = check_mesh(sc, other, otris, poses, (4, 16))
            assert (before != after).any()
            h = sc.ths[1]
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
            _, refit, _, _ = check_mesh(sc, other, otris, poses, (4, 16))
            assert (refit != after).any()
            # other refitted too: the query triangles are its stored records as they now are
            shrunk = (otris * F(0.75)).astype(F)
            other.clearTribuffer()
            other.loadTriangles(shrunk.reshape(-1, 9))
            other.refit()
            check_mesh(sc, other, shrunk, poses, (16,))
        finally:
            other.close()


def test_answers_do_not_depend_on_the_trees(psm, ctx):
    """the members and other built under a rotating and under a shearing optimisation matrix: other trees, the same answers"""
    rng = np.random.RandomState(121)
    a, b = _soup(122, 150, 1.0, 0.2), _soup(123, 100, 1.0, 0.2)
    entries = [(k % 2, NQ.random_pose(rng, reflect=bool(k & 1), shift=1.0)) for k in range(6)]
    otris = _soup(124, 80, 1.2, 0.4)
    poses = general_poses(rng, 3, -2.0, 0.0)
    with _World(psm, ctx, [a, b], entries) as plain:
        other = _hier(psm, ctx, otris)
        try:
            flag, count, trows, irows = check_mesh(plain, other, otris, poses, (16,))
            assert flag.any() and (count > 0).sum() > 50
            for opt in (ROT_SCALE, SHEAR):
                with _World(psm, ctx, [a, b], entries, [opt, opt]) as sc:
                    t = np.array(sc.ths[0].info().transform).reshape(4, 4)[:3, :3]
                    assert np.abs(t - np.diag(np.diag(t))).max() > 0.01
                    other2 = _hier(psm, ctx, otris, opt)
                    try:
                        for o in (other, other2):
                            got = sc.world.trianglesOnMesh(o, poses, 16, skip=None)
                            _same(sc.world.overlapsMesh(o, poses), flag, "flag under an optimisation matrix")
                            _same(sc.world.countOnMesh(o, poses), count, "count under an optimisation matrix")
                            _same(got.tri, trows, "tri rows under an optimisation matrix")
                            _same(got.geom, irows, "inst rows under an optimisation matrix")
                        _same(sc.world.countOnMesh(other2, poses, skip=1), plain.world.countOnMesh(other, poses, skip=1), "skip under an optimisation matrix")
                    finally:
                        other2.close()
        finally:
            other.close()


# ---- 9: torch ------------------------------------------------------------------------------------------------------------------------------

def test_world_mesh_torch_tensors_on_a_side_stream(psm, ctx):
    if torch is None:
        pytest.skip("torch is not installed")
    rng = np.random.RandomState(125)
    entries = [(k % 2, NQ.random_pose(rng, reflect=bool(k & 1), shift=2.0)) for k in range(20)]
    otris = _soup(126, 150, 1.5, 0.4)
    poses = general_poses(rng, 8, -2.0, 1.0)
    with _World(psm, ctx, [_soup(127, 150, 0.8, 0.2), _soup(128, 100, 0.8, 0.2)], entries) as sc:
        other = _hier(psm, ctx, otris)
        try:
            w = sc.world
            flag, count, lists = w.overlapsMesh(other, poses, skip=4), w.countOnMesh(other, poses, skip=4), w.trianglesOnMesh(other, poses, 5, skip=4)
            assert flag.any() and not flag.all()
            dev = torch.device("cuda", 0)
            side = torch.cuda.Stream(dev)
            with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
                gflag, gcount = w.overlapsMesh(other, poses, skip=4, as_torch=True), w.countOnMesh(other, poses, skip=4, as_torch=True)
                glists = w.trianglesOnMesh(other, poses, 5, skip=4, as_torch=True)
                total = gcount.sum()                                                  # (torch work on the side stream: in order)
                bufs = [x.cpu() for x in (gflag, gcount, glists.tri, glists.geom, glists.count, total)]
            assert gflag.device == dev and gflag.dtype == torch.bool and gflag.shape == (8,)
            assert gcount.dtype == torch.int32 and gcount.shape == (8, 150)
            assert glists.tri.shape == (8, 150, 5) and glists.geom.shape == (8, 150, 5) and glists.geom.dtype == torch.int32
            _same(bufs[0].numpy(), flag, "torch overlapsMesh")
            _same(bufs[1].numpy().view(U), count, "torch countOnMesh")
            _same(bufs[2].numpy(), lists.tri, "torch trianglesOnMesh tri")
            _same(bufs[3].numpy(), lists.geom, "torch trianglesOnMesh inst")
            _same(bufs[4].numpy().view(U), lists.count, "torch trianglesOnMesh count")
            assert int(bufs[5]) == int(count.sum())
        finally:
            other.close()


# ---- 10: refusals ---------------------------------------------------------------------------------------------------------------------------

def test_world_mesh_refusals_launch_nothing(psm, ctx):
    """NULL other, poses and outputs, misaligned outputs, k = 0, 17 and 2^31, other not built, other of another context, a stale
    world, a bad pose named by its index, skip out of range and p x T = 2^32 are refused on the host: the outputs keep what they
    held; then the same buffers succeed at k = 16. The 2^32 bound is reached with 65 536 poses of a 65 536-triangle mesh, through
    the overlaps entry alone, whose whole output (a byte per pose) is allocated"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    through = F([[[0, 0, -2], [2, 0, 2], [2, 1, 2]], [[0, 0.25, -2], [2, 0.25, 2], [2, 1.25, 2]]])
    p, t = 3, 2
    ctx2 = psm.Context(0)
    foreign = big = unbuilt = None
    with _World(psm, ctx, [tri, tri + F([0.125, 0, 0])], [(0, NQ.IDENTITY), (1, NQ.IDENTITY)]) as sc:
        other = _hier(psm, ctx, through)
        hout, hinst, hcnt = ctx.buf_alloc(4 * 17 * p * t), ctx.buf_alloc(4 * 17 * p * t), ctx.buf_alloc(4 * p * t + 16)
        hbig = ctx.buf_alloc(65536 + 16)
        try:
            w = sc.world._w
            ctx.buf_upload(hout, np.full(17 * p * t, 7, np.int32))
            ctx.buf_upload(hinst, np.full(17 * p * t, 9, np.int32))
            ctx.buf_upload(hcnt, np.full(p * t + 4, 77, U))
            ctx.buf_upload(hbig, np.full(65536 + 16, 5, np.uint8))
            pout, pinst, pcnt, pbig = (ctypes.c_void_p(ctx.buf_ptr(h)[0]) for h in (hout, hinst, hcnt, hbig))
            good = np.ascontiguousarray(np.tile(np.eye(3, 4, dtype=F).reshape(1, 12), (p, 1)))
            size, none = ctypes.c_size_t(p), ctypes.c_int32(-1)
            err = lambda: lib.psm_last_error(ctx._h)

            def ptr(a):
                return a.ctypes.data_as(ctypes.c_void_p)

            def tris_call(k, o=other, m=good, skip=none, p_out=pout, p_inst=pinst, p_cnt=pcnt, count=size):
                return lib.psm_world_mesh_triangles_dev(w, None if o is None else o._h, None if m is None else ptr(m), count, skip,
                                                        ctypes.c_uint32(k), p_out, p_inst, p_cnt)

            def flat_call(fn, o=other, m=good, skip=none, p_out=pcnt, count=size):
                return fn(w, None if o is None else o._h, None if m is None else ptr(m), count, skip, p_out)
            flat = (lib.psm_world_mesh_overlaps_dev, lib.psm_world_mesh_count_dev)
            for k in (0, 17, 1 << 31):
                assert tris_call(k) == -1 and b"psm_world_mesh_triangles_dev: k must be 1 .. 16" in err()
            assert tris_call(4, o=None) == -1 and tris_call(4, m=None) == -1 and tris_call(4, p_out=None) == -1
            assert tris_call(4, p_inst=None) == -1 and tris_call(4, p_cnt=None) == -1 and b"psm_world_mesh_triangles_dev: NULL pointer" in err()
            assert tris_call(4, p_out=ctypes.c_void_p(pout.value + 2)) == -1 and b"tris not 4-byte aligned" in err()
            assert tris_call(4, p_inst=ctypes.c_void_p(pinst.value + 2)) == -1 and b"inst not 4-byte aligned" in err()
            assert tris_call(4, p_cnt=ctypes.c_void_p(pcnt.value + 2)) == -1 and b"counts not 4-byte aligned" in err()
            for fn in flat:
                assert flat_call(fn, o=None) == -1 and flat_call(fn, m=None) == -1 and flat_call(fn, p_out=None) == -1 and b"NULL pointer" in err()
                assert flat_call(fn, count=ctypes.c_size_t(0)) == 0                   # p = 0 is answered first
                assert fn(None, other._h, ptr(good), size, none, pcnt) == lib.psm_world_tri_count_dev(None, pcnt, size, pcnt) != 0
            assert flat_call(lib.psm_world_mesh_count_dev, p_out=ctypes.c_void_p(pcnt.value + 2)) == -1 and b"counts not 4-byte aligned" in err()
            unbuilt = psm.TriangleHierarchy(ctx)                                      # other not built: PSM_ERR_STATE
            unbuilt.allocate(4)
            unbuilt.loadTriangles(through.reshape(2, 9))
            foreign = _hier(psm, ctx2, through)                                       # a built hierarchy of another context
            ctx2.sync()
            scaled, nan = good.copy(), good.copy()
            scaled[1, [0, 5, 10]] = 1.01                                              # pose 1 scaled by 1.01
            nan[2, 7] = np.nan
            for call in (lambda **kw: tris_call(4, **kw), lambda **kw: flat_call(flat[0], **kw), lambda **kw: flat_call(flat[1], **kw)):
                assert call(o=unbuilt) == -5 and b"mesh query before build" in err()
                assert call(o=foreign) == -1 and b"different contexts" in err()
                assert call(m=scaled) == -1 and b"pose 1 has a transform that is not rigid" in err()
                assert call(m=nan) == -1 and b"pose 2 has a non-finite transform" in err()
                for s in (2, 3, -2, 1 << 30):
                    assert call(skip=ctypes.c_int32(s)) == -1 and b"skip %d of a world of 2" % s in err()
            # p x T = 2^32: PSM_ERR_CAPACITY (-4), before any upload
            big = psm.TriangleHierarchy(ctx)
            big.allocate(65536)
            big.loadTriangles(np.tile(through.reshape(2, 9), (32768, 1)))
            big.build()
            many = np.ascontiguousarray(np.tile(np.eye(3, 4, dtype=F).reshape(1, 12), (65536, 1)))
            assert flat_call(flat[0], o=big, m=many, p_out=pbig, count=ctypes.c_size_t(65536)) == -4 and b"more than 2^32 answers" in err()
            sc.ths[1].markDirty()
            sc.ths[1].build()                                                         # stale: PSM_ERR_STATE, every world query's message
            assert tris_call(4) == -5 and b"psm_world_mesh_triangles_dev: instance 1's hierarchy was rebuilt" in err()
            for fn in flat:
                assert flat_call(fn) == -5 and b"instance 1's hierarchy was rebuilt, or reloaded and not refitted, after psm_world_set_instances" in err()
            ctx.sync()
            assert (ctx.buf_download(hout, np.int32, 17 * p * t) == 7).all() and (ctx.buf_download(hinst, np.int32, 17 * p * t) == 9).all()
            assert (ctx.buf_download(hcnt, U, p * t + 4) == 77).all() and (ctx.buf_download(hbig, np.uint8, 65536 + 16) == 5).all()
            poses = good.reshape(p, 3, 4)
            with pytest.raises(psm.PsmError, match="instance 1's hierarchy was rebuilt"):
                sc.world.countOnMesh(other, poses)
            sc.world.setInstances([(sc.ths[0], NQ.IDENTITY), (sc.ths[1], NQ.IDENTITY)])
            w = sc.world._w
            for k in (0, 17):
                with pytest.raises(psm.PsmError, match="k must be 1 .. 16"):
                    sc.world.trianglesOnMesh(other, poses, k)
            with pytest.raises(psm.PsmError, match="skip must be None"):
                sc.world.overlapsMesh(other, poses, skip=2)
            with pytest.raises(ValueError):
                sc.world.countOnMesh(other, scaled.reshape(p, 3, 4))
            with pytest.raises(psm.PsmError, match="different contexts"):
                sc.world.countOnMesh(foreign, poses)
            with pytest.raises(psm.PsmError, match="mesh query before build"):
                sc.world.countOnMesh(unbuilt, poses)
            assert tris_call(16) == 0                                                 # and the same buffers are fine at k = 16
            ctx.sync()
            assert (ctx.buf_download(hcnt, U, p * t + 4) == [2] * (p * t) + [77] * 4).all()
            rows, irows = ctx.buf_download(hout, np.int32, 17 * p * t), ctx.buf_download(hinst, np.int32, 17 * p * t)
            assert (rows[:16 * p * t].reshape(p * t, 16) == [0, 0] + [-1] * 14).all() and (rows[16 * p * t:] == 7).all()
            assert (irows[:16 * p * t].reshape(p * t, 16) == [0, 1] + [-1] * 14).all() and (irows[16 * p * t:] == 9).all()
            assert tris_call(16, skip=ctypes.c_int32(0)) == 0                         # ... and with instance 0 left out
            ctx.sync()
            assert (ctx.buf_download(hcnt, U, p * t) == 1).all()
            assert (ctx.buf_download(hinst, np.int32, 16 * p * t).reshape(p * t, 16) == [1] + [-1] * 15).all()
        finally:
            for h in (hout, hinst, hcnt, hbig):
                ctx.buf_free(h)
            for th in (other, foreign, big, unbuilt):
                if th is not None:
                    th.close()
            ctx2.close()
