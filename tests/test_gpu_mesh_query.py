"""The mesh queries on the GPU (psm_bvh_mesh_overlaps_dev / psm_bvh_mesh_count_dev / psm_bvh_mesh_triangles_dev, mesh.hip;
TriangleHierarchy.meshOverlaps / meshCount / meshTriangles). The yardsticks are tests/mesh_query_model.py -- the
other hierarchy's stored leaves posed in numpy float32, then tri_tri by brute force over the queried hierarchy's leaves -- and the
contract's own statement: triCount / triTriangles of the same posed triangles. Every comparison is exact on every (pose,
triangle), and in every case the three queries are also held against one another: flag == any(count > 0), triangles.count ==
min(k, count), rows are prefixes."""
import ctypes
import os
import re

import numpy as np
import pytest

import mesh_query_model as MQ
from util import ROOT

try:   # (imported before the library loads its HIP runtime: see test_gpu_query.py)
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
U = np.uint32
GRID_CAP = int(re.search(r"#define PSM_QUERY_GRID_CAP (\d+)",
                         open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "psm_query_dev.h")).read()).group(1))
KS = (1, 2, 3, 8, 16)
POINT = np.repeat(F([[[0.25, 0.25, 0.25]]]), 3, axis=1)   # three equal vertices: the build keeps no leaf


def _hier(psm, ctx, tris, opt=None):
    tris = np.ascontiguousarray(tris, F).reshape(-1, 9)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(max(tris.shape[0], 1))
    th.loadTriangles(tris)
    th.build(opt)
    return th


def _leaves(psm, th):
    return th.download(psm.BVH_LEAF_TRI, np.int32, th.info().leaf_count)


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.size == 0:
        return
    bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, "%s: %d poses differ, first %d" % (what, bad.size, bad[0])


def check_mesh(psm, th, tris, other, otris, poses, ks=KS, model=True):
    """the three queries against the model (computed once at the largest k: its rows are prefixes, test_mesh_query_cpu), against
    triCount / triTriangles of the same float32-posed triangles where `model` is False, and against one another; returns the
    flag, the full count and the rows at the largest k"""
    p, t = MQ.poses12(poses).shape[0], np.asarray(otris).reshape(-1, 9).shape[0]
    oleaves = np.sort(_leaves(psm, other))
    if model:
        flag, count, rows, _ = MQ.query(tris, _leaves(psm, th), otris, oleaves, poses, max(ks))
    else:
        q = MQ.posed(otris, poses)
        count, rows = np.zeros((p, t), U), np.full((p, t, max(ks)), -1, np.int32)
        if oleaves.size:
            count[:, oleaves] = th.triCount(q[:, oleaves].reshape(-1, 3, 3)).reshape(p, -1)
            rows[:, oleaves] = th.triTriangles(q[:, oleaves].reshape(-1, 3, 3), max(ks)).tri.reshape(p, -1, max(ks))
        flag = (count > 0).any(axis=1)
    got_flag, got_count = th.meshOverlaps(other, poses), th.meshCount(other, poses)
    assert got_flag.shape == (p,) and got_flag.dtype == np.bool_ and got_count.shape == (p, t) and got_count.dtype == U
    _same(got_flag, flag, "meshOverlaps")
    _same(got_count, count, "meshCount")
    assert np.array_equal(got_flag, (got_count > 0).any(axis=1))
    widest = None
    for k in sorted(ks, reverse=True):
        got = th.meshTriangles(other, poses, k)
        assert got.tri.shape == (p, t, k) and got.tri.dtype == np.int32 and got.count.shape == (p, t) and got.count.dtype == U
        _same(got.tri, rows[:, :, :k], "meshTriangles k = %d" % k)
        _same(got.count, np.minimum(got_count, U(k)), "meshTriangles count against meshCount, k = %d" % k)
        assert np.array_equal(got.tri >= 0, np.arange(k)[None, None] < got.count[:, :, None])
        if widest is None:
            widest = got.tri
        _same(got.tri, widest[:, :, :k], "meshTriangles k = %d is a prefix of k = %d" % (k, max(ks)))
    return flag, count, rows


def lattice_soup(seed, count):
    """triangles with vertices on the 1/8 lattice of [-1, 1]^3, each vertex within a step of one lattice point
    (tests/test_gpu_tri_query.py's)"""
    rng = np.random.RandomState(seed)
    a = rng.randint(-8, 9, (count, 1, 3))
    a[count // 2:] = rng.randint(0, 5, (count - count // 2, 1, 3))   # half of them crowd one octant: queries that meet more than 16
    return (np.clip(a + rng.randint(-1, 2, (count, 3, 3)), -8, 8) / 8.0).astype(F)


def _pose(r, t):
    return np.concatenate([np.asarray(r, D), np.asarray(t, D).reshape(3, 1)], axis=1)


def rotations(rng, n):
    """n random rotations and reflections (alternating), float64, from unit quaternions"""
    q = rng.normal(size=(n, 4))
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    r = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)
    r[1::2, :, 0] = -r[1::2, :, 0]
    return r


SIGNED_PERMUTATIONS = [np.eye(3), np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]]), np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]]),
                       np.array([[-1, 0, 0], [0, 1, 0], [0, 0, 1]]), np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]]),
                       np.array([[0, 0, -1], [0, -1, 0], [-1, 0, 0]])]
LATTICE_SHIFTS = ([0, 0, 0], [0.125, 0, -0.25], [3, 3, 3], [0, 0.5, 0], [-3.375, 0, 0.125], [0.25, 0.25, 0])


def lattice_case():
    """(tris, otris, poses): all arithmetic exact. The other mesh is a 130-triangle lattice soup and one triangle with three
    equal vertices; the poses are the identity and five signed permutation matrices (reflections among them) with translations
    on the 1/8 lattice, two of them out of reach"""
    otris = np.concatenate([lattice_soup(51, 130), POINT])
    return lattice_soup(41, 500), otris, [_pose(r, t) for r, t in zip(SIGNED_PERMUTATIONS, LATTICE_SHIFTS)]


def test_mesh_lattice_soup(psm, ctx):
    tris, otris, poses = lattice_case()
    assert sum(np.linalg.det(m[:, :3]) < 0 for m in poses) >= 2
    th, other = _hier(psm, ctx, tris), _hier(psm, ctx, otris)
    try:
        leaf_count = other.info().leaf_count
        assert leaf_count % 64 != 0 and leaf_count < otris.shape[0] == 131 and leaf_count > 64
        flag, count, rows = check_mesh(psm, th, tris, other, otris, poses)
        assert flag.sum() >= 3 and (~flag).sum() >= 2 and (count > 16).any()
        assert (count[:, 130] == 0).all() and (rows[:, 130] == -1).all()      # the dropped triangle, at every pose
        assert ((count > 0) & (count < 16)).sum() > 50 and (count[flag] == 0).sum() > 50
    finally:
        th.close()
        other.close()


def general_case():
    rng = np.random.RandomState(71)
    tris = (rng.uniform(-1, 1, (2000, 1, 3)) + rng.uniform(-0.1, 0.1, (2000, 3, 3))).astype(F)
    otris = (rng.uniform(-0.6, 0.6, (300, 1, 3)) + rng.uniform(-0.15, 0.15, (300, 3, 3))).astype(F)
    shift = rng.normal(size=(8, 3))
    shift *= (10.0 ** np.linspace(-3, 1, 8) / np.linalg.norm(shift, axis=1))[:, None]      # translations over 1e-3 .. 10
    return tris, otris, [_pose(r, t) for r, t in zip(rotations(rng, 8), shift)]


def test_mesh_general_poses(psm, ctx):
    tris, otris, poses = general_case()
    th, other = _hier(psm, ctx, tris), _hier(psm, ctx, otris)
    try:
        flag, count, rows = check_mesh(psm, th, tris, other, otris, poses)
        assert flag.sum() >= 5 and (~flag).sum() >= 1 and (count > 0).sum() > 500 and (count == 0).sum() > 500
        # the contract's own statement: triCount / triTriangles of the same float32-posed triangles
        f2, c2, r2 = check_mesh(psm, th, tris, other, otris, poses, (3, 16), model=False)
        assert np.array_equal(c2, count) and np.array_equal(r2, rows)
        # a 4 x 4 matrix, and one pose alone: its row of the batch
        m44 = np.concatenate([poses[2], [[0, 0, 0, 1]]])
        _same(th.meshCount(other, m44), count[2:3], "one 4 x 4 pose")
        _same(th.meshCount(other, np.stack([np.concatenate([m, [[0, 0, 0, 1]]]) for m in poses])), count, "[p, 4, 4] poses")
    finally:
        th.close()
        other.close()


def test_mesh_self_query(psm, ctx):
    """other == bvh at the identity: every leaf meets at least itself (the query is the stored triangle: A = 0)"""
    rng = np.random.RandomState(72)
    tris = np.concatenate([lattice_soup(7, 200), POINT, (rng.uniform(-1, 1, (600, 1, 3)) + rng.uniform(-0.08, 0.08, (600, 3, 3))).astype(F),
                           (rng.uniform(-1e3, 1e3, (50, 1, 3)) + rng.uniform(-1e-2, 1e-2, (50, 3, 3))).astype(F)])
    th = _hier(psm, ctx, tris)
    try:
        leaves = np.sort(_leaves(psm, th))
        assert 200 not in leaves and 800 < leaves.size < tris.shape[0]      # (some of the 1e-2 triangles at 1e3 are too small for the build)
        flag, count, rows = check_mesh(psm, th, tris, th, tris, np.eye(3, 4), (16,))
        assert flag[0] and (count[0, leaves] >= 1).all() and not count[0, np.setdiff1d(np.arange(tris.shape[0]), leaves)].any()
        few = leaves[count[0, leaves] <= 16]
        assert few.size > 300 and (rows[0, few] == few[:, None]).any(axis=1).all()
    finally:
        th.close()


def _soup(rng, n, spread=0.5):
    return (rng.uniform(-1, 1, (n, 1, 3)) + rng.uniform(-spread, spread, (n, 3, 3))).astype(F)


@pytest.mark.parametrize("leaves", [1, 63, 64, 65])
@pytest.mark.parametrize("p", [1, 3])
def test_mesh_other_sizes(psm, ctx, leaves, p):
    rng = np.random.RandomState(100 * leaves + p)
    tris = _soup(np.random.RandomState(73), 200, 0.2)
    otris = np.concatenate([POINT, _soup(rng, leaves, 0.2)])
    poses = [_pose(r, t) for r, t in zip(rotations(rng, p), rng.uniform(-0.3, 0.3, (p, 3)))]
    th, other = _hier(psm, ctx, tris), _hier(psm, ctx, otris)
    try:
        assert other.info().leaf_count == leaves
        flag, count, _ = check_mesh(psm, th, tris, other, otris, poses, (2, 16))
        assert (count[:, 0] == 0).all() and (leaves == 1 or (flag.all() and (count == 0).any()))
    finally:
        th.close()
        other.close()


def test_mesh_hierarchies_without_leaves_and_tiny_ones(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    degenerate = np.repeat(tri[:, :1], 3, axis=1)
    rng = np.random.RandomState(74)
    otris = np.concatenate([_soup(rng, 70, 0.8) + F([0.7, 0, 0]), F([[[-4, -0.5, -0.25], [4, -0.5, -0.25], [4, 0.5, 0.5]]])])   # the last: through all
    poses = [np.eye(3, 4), _pose(rotations(rng, 1)[0], [0.1, 0, 0])]
    other = _hier(psm, ctx, otris)
    empty = _hier(psm, ctx, np.concatenate([degenerate] * 4))
    try:
        assert empty.info().leaf_count == 0
        for tris, leaves in ((np.concatenate([degenerate] * 4), 0), (np.concatenate([degenerate, tri, degenerate]), 1),
                             (np.concatenate([tri, degenerate, tri + F([0.5, 0, 0])]), 2),
                             (np.concatenate([tri, tri + F([0.25, 0, 0]), degenerate, tri + F([0.5, 0, 0])]), 3)):
            th = _hier(psm, ctx, tris)
            try:
                assert th.info().leaf_count == leaves
                flag, count, rows = check_mesh(psm, th, tris, other, otris, poses, (1, 16))
                assert count.max() == leaves == count[0, 70] and (leaves == 0) == (not flag.any())
                # and the other way round: a mesh without leaves meets nothing, whatever is queried
                f0, c0, r0 = check_mesh(psm, th, tris, empty, np.concatenate([degenerate] * 4), poses, (4,))
                assert not f0.any() and not c0.any() and (r0 == -1).all()
            finally:
                th.close()
    finally:
        other.close()
        empty.close()


def test_mesh_grid_stride_second_trip(psm, ctx):
    """p x L just above PSM_QUERY_GRID_CAP x 64 + 65: the last queries take a second trip of the grid-stride loop, where the count
    and the list must start empty again; held against triCount / triTriangles of the host-posed triangles"""
    rng = np.random.RandomState(75)
    tris = _soup(np.random.RandomState(76), 16, 0.6)
    otris = np.concatenate([_soup(rng, 30, 0.5), POINT, _soup(rng, 35, 0.5)])
    leaves = 65
    p = -(-(GRID_CAP * 64 + 65) // leaves)
    assert GRID_CAP * 64 + 65 <= p * leaves < GRID_CAP * 64 + 65 + leaves
    poses = np.concatenate([rotations(rng, p), rng.uniform(-0.8, 0.8, (p, 3, 1))], axis=2)
    th, other = _hier(psm, ctx, tris), _hier(psm, ctx, otris)
    try:
        assert other.info().leaf_count == leaves
        flag, count, _ = check_mesh(psm, th, tris, other, otris, poses, (2,), model=False)   # (the flag kernel skips here by itself)
        assert flag.any() and not flag.all()
        tail = count[-2:, np.sort(_leaves(psm, other))]
        assert len(np.unique(count)) > 2 and len(np.unique(tail)) > 2 and (count[:, 30] == 0).all()
    finally:
        th.close()
        other.close()


def flag_case():
    """(tris, otris, poses, touching): 257 poses of a small mesh, most far away, a few cutting, and one (`touching`) at which a
    single vertex of the other mesh lies on a single vertex of the queried one and nothing else meets -- all on a lattice"""
    far = F([[[4, 4, 4], [4.5, 4, 4], [4, 4.5, 4]]])
    tris = np.concatenate([lattice_soup(41, 500), far])
    finger = F([[[-1, -1, -1], [-1.5, -1, -1], [-1, -1.5, -1]]])
    otris = np.concatenate([(lattice_soup(52, 40) * F(0.25)).astype(F), POINT, finger])
    poses = [_pose(np.eye(3), [-20.0 - q, 0.25 * (q % 5), 0]) for q in range(257)]
    for q, (r, t) in {3: (0, [0, 0, 0]), 64: (1, [0.25, 0.125, 0.25]), 65: (3, [0.5, 0.25, 0.125]), 200: (5, [0.375, 0.375, 0.25]),
                      256: (2, [0.25, 0.5, 0.5])}.items():
        poses[q] = _pose(SIGNED_PERMUTATIONS[r], t)
    touching = 131
    poses[touching] = _pose(np.eye(3), [5, 5, 5])
    return tris, otris, poses, touching


def test_mesh_flag_per_pose(psm, ctx):
    tris, otris, poses, touching = flag_case()
    th, other = _hier(psm, ctx, tris), _hier(psm, ctx, otris)
    try:
        flag, count, _ = check_mesh(psm, th, tris, other, otris, poses, (16,))
        assert list(np.nonzero(flag)[0]) == [3, 64, 65, touching, 200, 256]
        assert count[touching].sum() == 1 and count[touching, 41] == 1          # the finger alone, on the far triangle alone
        assert np.array_equal(flag, (th.meshCount(other, poses) > 0).any(axis=1))
        # the early-out skip depends on timing, the answer does not: with the skip forced on (a launch this small leaves it off)
        # twice the same, and the same with it forced off
        for skip in ("1", "1", "0"):
            os.environ["PSM_MESH_SKIP"] = skip
            try:
                assert np.array_equal(th.meshOverlaps(other, poses), flag), skip
            finally:
                del os.environ["PSM_MESH_SKIP"]
    finally:
        th.close()
        other.close()


# the optimisation matrices of test_gpu_tri_query.py: the fit transform's 3 x 3 part is full
ROT_SCALE = np.array([[np.cos(0.3), 0, np.sin(0.3), 0.5], [0, 1.3, 0, -1.0], [-np.sin(0.3), 0, np.cos(0.3), 2.0], [0, 0, 0, 1]])
SHEAR = np.array([[1, 0.6, 0, 0.2], [0, 1, -0.4, 0], [0.3, 0, 1, -1], [0, 0, 0, 1]])


def test_mesh_answers_do_not_depend_on_the_trees(psm, ctx):
    """other built under a rotating and under a shearing optimisation matrix (another tree; the lane mapping goes by triangle id), the
    queried hierarchy under one too, and both refitted: the same answers"""
    tris, otris, poses = general_case()
    tris, otris, poses = tris[:800], otris[:150], poses[:4]
    th = _hier(psm, ctx, tris)
    plain = _hier(psm, ctx, otris)
    try:
        flag, count, rows = check_mesh(psm, th, tris, plain, otris, poses, (16,))
        assert flag.any() and (count > 0).sum() > 100
        for opt in (ROT_SCALE, SHEAR):
            other = _hier(psm, ctx, otris, opt)
            try:
                _same(th.meshOverlaps(other, poses), flag, "flag under an optimisation matrix of other")
                _same(th.meshCount(other, poses), count, "count under an optimisation matrix of other")
                _same(th.meshTriangles(other, poses, 16).tri, rows, "rows under an optimisation matrix of other")
                other.clearTribuffer()
                other.loadTriangles(otris.reshape(-1, 9))
                other.refit()
                _same(th.meshCount(other, poses), count, "count after refit() of other")
                _same(th.meshTriangles(other, poses, 16).tri, rows, "rows after refit() of other")
            finally:
                other.close()
        for opt in (ROT_SCALE, SHEAR):
            th2 = _hier(psm, ctx, tris, opt)
            try:
                _same(th2.meshCount(plain, poses), count, "count under an optimisation matrix of the queried hierarchy")
                th2.clearTribuffer()
                th2.loadTriangles(tris.reshape(-1, 9))
                th2.refit()
                _same(th2.meshOverlaps(plain, poses), flag, "flag after refit()")
                _same(th2.meshCount(plain, poses), count, "count after refit()")
                _same(th2.meshTriangles(plain, poses, 16).tri, rows, "rows after refit()")
            finally:
                th2.close()
    finally:
        th.close()
        plain.close()


def test_mesh_torch_tensors_on_a_side_stream(psm, ctx):
    if torch is None:
        pytest.skip("torch is not installed")
    tris, otris, poses = general_case()
    th, other = _hier(psm, ctx, tris), _hier(psm, ctx, otris)
    try:
        flag, count, lists = th.meshOverlaps(other, poses), th.meshCount(other, poses), th.meshTriangles(other, poses, 5)
        assert flag.any() and not flag.all()
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            gflag, gcount = th.meshOverlaps(other, poses, as_torch=True), th.meshCount(other, poses, as_torch=True)
            glists = th.meshTriangles(other, poses, 5, as_torch=True)
            total = gcount.sum()                                                  # (torch work on the side stream: in order)
            bufs = [x.cpu() for x in (gflag, gcount, glists.tri, glists.count, total)]
        assert gflag.device == dev and gflag.dtype == torch.bool and gflag.shape == (8,)
        assert gcount.dtype == torch.int32 and gcount.shape == (8, 300)
        assert glists.tri.shape == (8, 300, 5) and glists.tri.dtype == torch.int32 and glists.count.dtype == torch.int32
        _same(bufs[0].numpy(), flag, "torch meshOverlaps")
        _same(bufs[1].numpy().view(U), count, "torch meshCount")
        _same(bufs[2].numpy(), lists.tri, "torch meshTriangles")
        _same(bufs[3].numpy().view(U), lists.count, "torch meshTriangles count")
        assert int(bufs[4]) == int(count.sum())
    finally:
        th.close()
        other.close()


def test_mesh_refusals_launch_nothing(psm, ctx):
    """a call before either build, k = 0, k = 17, NULL and misaligned pointers, poses that are not finite or not rigid and
    hierarchies of two contexts are refused on the host: the outputs keep what they held. (A single hierarchy deeper than the
    query stack cannot be made: 2^27 triangles bound it at 90 entries.)"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    through = F([[[0, 0, -2], [2, 0, 2], [2, 1, 2]], [[0, 0.25, -2], [2, 0.25, 2], [2, 1.25, 2]]])
    th, other = psm.TriangleHierarchy(ctx), psm.TriangleHierarchy(ctx)
    th.allocate(4)
    th.loadTriangles(tri.reshape(1, 9))
    other.allocate(4)
    other.loadTriangles(through.reshape(2, 9))
    ctx2 = psm.Context(0)
    foreign = None
    p, t = 3, 2
    hout, hcnt = ctx.buf_alloc(4 * 17 * p * t), ctx.buf_alloc(4 * p * t + 16)
    try:
        ctx.buf_upload(hout, np.full(17 * p * t, 7, np.int32))
        ctx.buf_upload(hcnt, np.full(p * t + 4, 77, U))
        pout, pcnt = (ctypes.c_void_p(ctx.buf_ptr(h)[0]) for h in (hout, hcnt))
        good = np.ascontiguousarray(np.tile(np.eye(3, 4, dtype=F).reshape(1, 12), (p, 1)))
        size = ctypes.c_size_t(p)
        err = lambda: lib.psm_last_error(ctx._h)

        def ptr(a):
            return a.ctypes.data_as(ctypes.c_void_p)

        def tris_call(k, a=th, b=other, m=good, p_out=pout, p_cnt=pcnt, count=size):
            return lib.psm_bvh_mesh_triangles_dev(a._h, b._h, None if m is None else ptr(m), count, ctypes.c_uint32(k), p_out, p_cnt)

        def flat_call(fn, a=th, b=other, m=good, p_out=pcnt, count=size):
            return fn(a._h, b._h, None if m is None else ptr(m), count, p_out)
        flat = (lib.psm_bvh_mesh_overlaps_dev, lib.psm_bvh_mesh_count_dev)
        for fn in flat:
            assert flat_call(fn) == -5 and b"mesh query before build" in err()   # neither is built: PSM_ERR_STATE
            assert flat_call(fn, count=ctypes.c_size_t(0)) == 0                   # p = 0 is answered first
        assert tris_call(4) == -5 and b"mesh query before build" in err()
        th.build()
        for fn in flat:
            assert flat_call(fn) == -5 and b"mesh query before build" in err()   # other is not built
        other.build()
        th_unbuilt = psm.TriangleHierarchy(ctx)
        th_unbuilt.allocate(4)
        th_unbuilt.loadTriangles(tri.reshape(1, 9))
        try:
            assert tris_call(4, a=th_unbuilt) == -5 and b"mesh query before build" in err()   # the queried one is not built
        finally:
            th_unbuilt.close()
        for k in (0, 17, 1 << 31):
            assert tris_call(k) == -1 and b"k must be 1 .. 16" in err()
        assert tris_call(4, p_out=None) == -1 and tris_call(4, p_cnt=None) == -1 and tris_call(4, m=None) == -1
        assert b"NULL pointer" in err()
        assert tris_call(4, p_out=ctypes.c_void_p(pout.value + 2)) == -1 and b"tris not 4-byte aligned" in err()
        assert tris_call(4, p_cnt=ctypes.c_void_p(pcnt.value + 2)) == -1 and b"counts not 4-byte aligned" in err()
        for fn in flat:
            assert flat_call(fn, m=None) == -1 and flat_call(fn, p_out=None) == -1
            assert fn(None, other._h, ptr(good), size, pcnt) == -1 and fn(th._h, None, ptr(good), size, pcnt) == -1
        assert flat_call(lib.psm_bvh_mesh_count_dev, p_out=ctypes.c_void_p(pcnt.value + 2)) == -1 and b"counts not 4-byte aligned" in err()
        scaled, nan = good.copy(), good.copy()
        scaled[1, [0, 5, 10]] = 1.01                                              # pose 1 scaled by 1.01
        nan[2, 7] = np.nan
        for fn in flat:
            assert flat_call(fn, m=scaled) == -1 and b"pose 1 has a transform that is not rigid" in err()
            assert flat_call(fn, m=nan) == -1 and b"pose 2 has a non-finite transform" in err()
        assert tris_call(4, m=scaled) == -1 and b"pose 1 " in err()
        foreign = psm.TriangleHierarchy(ctx2)                                     # a built hierarchy of another context
        foreign.allocate(4)
        foreign.loadTriangles(through.reshape(2, 9))
        foreign.build()
        ctx2.sync()
        for fn in flat:
            assert flat_call(fn, b=foreign) == -1 and b"different contexts" in err()
        assert tris_call(4, b=foreign) == -1 and b"different contexts" in err()
        ctx.sync()
        assert (ctx.buf_download(hout, np.int32, 17 * p * t) == 7).all() and (ctx.buf_download(hcnt, U, p * t + 4) == 77).all()
        for k in (0, 17):
            with pytest.raises(psm.PsmError):
                th.meshTriangles(other, good.reshape(p, 3, 4), k)
        with pytest.raises(ValueError):
            th.meshCount(other, scaled.reshape(p, 3, 4))
        with pytest.raises(psm.PsmError, match="different contexts"):
            th.meshCount(foreign, good.reshape(p, 3, 4))
        assert tris_call(16) == 0                                                  # and the same buffers are fine at k = 16
        ctx.sync()
        assert (ctx.buf_download(hcnt, U, p * t + 4) == [1] * (p * t) + [77] * 4).all()
        rows = ctx.buf_download(hout, np.int32, 17 * p * t)
        assert (rows[:16 * p * t].reshape(p * t, 16) == [0] + [-1] * 15).all() and (rows[16 * p * t:] == 7).all()
    finally:
        for h in (hout, hcnt):
            ctx.buf_free(h)
        th.close()
        other.close()
        if foreign is not None:
            foreign.close()
        ctx2.close()
