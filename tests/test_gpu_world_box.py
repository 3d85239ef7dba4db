"""The box queries of an instance world on the GPU (psm_world_box_overlaps_dev / psm_world_box_count_dev /
psm_world_box_triangles_dev, world_box.hip; InstanceWorld.overlapsBox / countInBox / trianglesInBox). The yardstick
is tests/world_box_query_model.py part (a): box_tri in numpy float32 over the forward-posed downloaded leaves of every instance.
Every comparison is exact on every box, and in every case the three queries are also held against one another: overlaps ==
(count > 0), the rows' count == min(k, count), the rows are prefixes."""
import ctypes

import numpy as np
import pytest

import inside_query_model as IQ
import instance_query_model as NQ
import query_model as Q
import world_box_query_model as WB
from test_gpu_box_query import GRID_CAP, ROT_SCALE, SHEAR
from test_world_box_cpu import _pose, _rotation, cube, grid_cells, lattice_world

try:   # (imported before the library loads its HIP runtime, as tests/test_gpu_query.py)
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
U = np.uint32
KS = (1, 2, 3, 8, 16)


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, "%s: %d differ, first %d: %s against %s" % (what, bad.size, bad[0], a[bad[0]], b[bad[0]])


def _hier(psm, ctx, tris, opt=None):
    tris = np.ascontiguousarray(tris, F).reshape(-1, 9)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(max(tris.shape[0], 1))
    th.loadTriangles(tris)
    th.build(opt)
    return th


class _World:
    """hierarchies over meshes (opts: an optimisation matrix per mesh, or None), an InstanceWorld of (mesh index, pose) entries,
    and the model's instances (mesh, downloaded leaves, pose)"""

    def __init__(self, psm, ctx, meshes, entries, opts=None):
        self.psm, self.ctx = psm, ctx
        self.meshes = [np.ascontiguousarray(t, F).reshape(-1, 3, 3) for t in meshes]
        self.ths = [_hier(psm, ctx, t, None if opts is None else opts[k]) for k, t in enumerate(self.meshes)]
        self.which = [k for k, _ in entries]
        self.world = psm.InstanceWorld(ctx, [(self.ths[k], m) for k, m in entries])

    def insts(self):
        leaves = [th.download(self.psm.BVH_LEAF_TRI, np.int32, th.info().leaf_count) for th in self.ths]
        return [(self.meshes[k], leaves[k], m) for k, m in zip(self.which, self.world.transforms())]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.world.close()
        for th in self.ths:
            th.close()


def check_boxes(sc, lo, hi, ks=KS, insts=None):
    """the three queries against (a) (computed once at the largest k: its rows are prefixes, test_world_box_cpu) and against one
    another; returns (a) at the largest k: flag, count, tri rows, inst rows"""
    w = sc.world
    lo, hi = np.ascontiguousarray(lo, F).reshape(-1, 3), np.ascontiguousarray(hi, F).reshape(-1, 3)
    n = lo.shape[0]
    flag, count, trows, irows, _ = WB.flat(sc.insts() if insts is None else insts, lo, hi, max(ks))
    got_flag, got_count = w.overlapsBox(lo, hi), w.countInBox(lo, hi)
    assert got_flag.shape == (n,) and got_flag.dtype == np.bool_ and got_count.shape == (n,) and got_count.dtype == U
    _same(got_flag, flag, "overlapsBox")
    _same(got_count, count, "countInBox")
    assert np.array_equal(got_flag, got_count > 0)
    widest = None
    for k in sorted(ks, reverse=True):
        got = w.trianglesInBox(lo, hi, k)
        assert got.tri.shape == (n, k) and got.tri.dtype == np.int32 and got.geom.shape == (n, k) and got.geom.dtype == np.int32
        assert got.count.shape == (n,) and got.count.dtype == U
        _same(got.tri, trows[:, :k], "trianglesInBox tri, k = %d" % k)
        _same(got.geom, irows[:, :k], "trianglesInBox inst, k = %d" % k)
        _same(got.count, np.minimum(got_count, U(k)), "trianglesInBox count against countInBox, k = %d" % k)
        live = np.arange(k)[None] < got.count[:, None]
        assert np.array_equal(got.tri >= 0, live) and np.array_equal(got.geom >= 0, live)
        if widest is None:
            widest = got
        _same(got.tri, widest.tri[:, :k], "trianglesInBox k = %d is a prefix" % k)
        _same(got.geom, widest.geom[:, :k], "trianglesInBox inst k = %d is a prefix" % k)
    return flag, count, trows, irows


def _soup(seed, n, spread=1.0, size=0.15):
    rng = np.random.RandomState(seed)
    c = rng.uniform(-spread, spread, (n, 1, 3))
    return (c + rng.uniform(-size, size, (n, 3, 3))).astype(F)


def test_identity_world_of_one_equals_the_hierarchy(psm, ctx):
    tris = _soup(41, 600, 1.0, 0.1)
    rng = np.random.RandomState(42)
    centre = rng.uniform(-1.1, 1.1, (2048, 3))
    half = 10.0 ** rng.uniform(-3, -0.3, (2048, 1)) * rng.uniform(0.3, 1.0, (2048, 3))
    lo, hi = (centre - half).astype(F), (centre + half).astype(F)
    lo[0, 0], hi[1, 1], lo[2], hi[2] = np.nan, np.inf, 0.5, 0.25
    lo[3:40] = hi[3:40] = tris[rng.choice(600, 37), 0]
    with _World(psm, ctx, [tris], [(0, NQ.IDENTITY)]) as sc:
        th, w = sc.ths[0], sc.world
        _same(w.overlapsBox(lo, hi), th.boxOverlaps(lo, hi), "overlaps")
        _same(w.countInBox(lo, hi), th.boxCount(lo, hi), "count")
        for k in (1, 4, 16):
            a, b = w.trianglesInBox(lo, hi, k), th.boxTriangles(lo, hi, k)
            _same(a.tri, b.tri, "rows k = %d" % k)
            _same(a.count, b.count, "rows' count k = %d" % k)
            assert np.array_equal(a.geom, np.where(b.tri >= 0, 0, -1))
        _, count, _, _ = check_boxes(sc, lo, hi, (16,))
        assert (count[:3] == 0).all() and (count[3:40] >= 1).all() and (count > 16).any()


def test_lattice_world_and_its_cells(psm, ctx):
    """cubes at the 48 signed axis permutations and integer translations, three of them twice: all arithmetic exact; grid cells,
    cells shifted by half a cell on one, two and three axes, point boxes. Coincident instances are listed lowest instance first."""
    model = lattice_world()
    lo, hi = grid_cells((-2, -2, -2), (4, 4, 4), 6, ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)))
    pts = np.array([(x, y, z) for x in (-1.0, 0.0, 0.5, 1.0, 2.0) for y in (-1.0, 0.0, 0.5, 1.0, 2.0) for z in (-1.0, 0.0, 0.5, 1.0, 2.0)], F)
    lo, hi = np.concatenate([lo, pts]), np.concatenate([hi, pts])
    with _World(psm, ctx, [cube()], [(0, m[2]) for m in model]) as sc:
        assert sc.ths[0].info().leaf_count == 12
        flag, count, trows, irows = check_boxes(sc, lo, hi)
        assert (count > 16).any() and ((count > 0) & (count < 16)).any() and (count == 0).any()
        both = np.nonzero((irows == 0).any(axis=1) & (irows == 48).any(axis=1) & (count <= 16))[0]
        assert both.size > 0
        for i in both[:20]:
            assert list(trows[i][irows[i] == 0]) == list(trows[i][irows[i] == 48])
            live = irows[i][irows[i] >= 0]
            assert list(live) == sorted(live)


def _members():
    deep, _, _ = Q.deep_fixture()
    return [IQ.icosphere(1, 0.6), _soup(43, 200, 0.8, 0.2), deep]


def _rigid_entries(n, seed):
    """n random rigid poses, every second a reflection, of the three members; the deep member stands at every third place of the
    first 33 and at every 32nd after that (the brute force pays for each of its 1 344 leaves)"""
    rng = np.random.RandomState(seed)
    spread = max(1.0, n ** (1.0 / 3.0))
    out = []
    for k in range(n):
        which = k % 3 if k < 33 else (2 if k % 32 == 0 else k % 2)
        out.append((which, NQ.random_pose(rng, reflect=bool(k & 1), shift=spread)))
    return out, spread


@pytest.mark.parametrize("n", [2, 33, 257])
def test_world_box_parity_with_the_flat_answer(psm, ctx, n):
    members = _members()
    assert members[0].shape[0] == 80 and members[1].shape[0] == 200
    entries, spread = _rigid_entries(n, 200 + n)
    rng = np.random.RandomState(n)
    with _World(psm, ctx, members, entries) as sc:
        insts = sc.insts()
        B = 1024
        centre = rng.uniform(-spread - 1.2, spread + 1.2, (B, 3))
        half = 10.0 ** rng.uniform(-3, 0, (B, 1)) * rng.uniform(0.3, 1.0, (B, 3)) * spread      # sizes over three decades
        lo, hi = (centre - half).astype(F), (centre + half).astype(F)
        lo[0, 0], hi[1, 1], lo[2, 2], hi[3, 0] = np.nan, np.nan, np.inf, np.inf
        lo[4, 1], hi[5, 2] = -np.inf, -np.inf
        lo[6, 0], hi[6, 0] = 0.5, 0.25                                                          # lo > hi on one axis
        lo[7], hi[7] = -np.inf, np.inf
        at = 8
        for tris, leaves, pose in insts[:8]:                                                    # point boxes on posed vertices
            v0 = WB.posed_leaves(tris[np.sort(leaves)[:8]], pose)[0]
            lo[at:at + v0.shape[0]] = hi[at:at + v0.shape[0]] = v0
            at += 8
        lo[72], hi[72] = -spread - 4, spread + 4                                                # one box around everything
        flag, count, trows, irows = check_boxes(sc, lo, hi, KS, insts)
        assert (count[:8] == 0).all() and (count[8:8 + 8 * min(n, 8)] >= 1).all()
        total = sum(len(i[1]) for i in insts)
        assert count[72] == total and sc.ths[2].info().leaf_count > 900                        # (through the deep member: the spill path)
        first = sorted(insts[0][1])[:16]
        assert list(zip(irows[72], trows[72])) == [(0, t) for t in first]
        some, many = ((count[73:] > 0) & (count[73:] <= 16)).sum(), (count[73:] > 16).sum()      # so that the case cannot pass emptily
        assert (count[73:] == 0).sum() > 20 and some > (50 if n > 2 else 20) and many > (20 if n > 2 else 4)


def test_a_member_far_from_its_origin(psm, ctx):
    """object coordinates at +1000, the pose brings the body back; beside it the same body at -1000 taken out to +2000"""
    rng = np.random.RandomState(44)
    near = _soup(45, 150, 1.0, 0.15)
    far = (near + F(1000)).astype(F)
    r0, r1 = _rotation(rng), _rotation(rng, True)
    entries = [(0, _pose(r0, -r0 @ np.full(3, 1000.0))), (1, _pose(r1, r1 @ np.full(3, 1000.0) + 2000.0)), (1, NQ.IDENTITY)]
    with _World(psm, ctx, [far, (near - F(1000)).astype(F)], entries) as sc:
        insts = sc.insts()
        lo, hi = [], []
        for tris, leaves, pose in insts:
            v0 = WB.posed_leaves(tris[np.sort(leaves)], pose)[0].astype(D)
            c = v0[rng.randint(0, v0.shape[0], 300)] + rng.normal(size=(300, 3)) * 0.05
            h = 10.0 ** rng.uniform(-3, -0.3, (300, 3))
            lo.append(c - h)
            hi.append(c + h)
        _, count, _, irows = check_boxes(sc, np.concatenate(lo), np.concatenate(hi), (4, 16), insts)
        for j in range(3):
            assert (count[300 * j:300 * (j + 1)] > 0).mean() > 0.2 and (irows[300 * j:300 * (j + 1), 0] == j).any()


def test_tiny_members_and_the_empty_world(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    degenerate = np.repeat(tri[:, :1], 3, axis=1)                    # three equal vertices: the build keeps no leaf
    meshes = [np.concatenate([degenerate] * 4), np.concatenate([degenerate, tri, degenerate]),
              np.concatenate([tri, degenerate, tri + F([0.5, 0, 0])]), np.concatenate([tri, tri + F([0.25, 0, 0]), degenerate, tri + F([0.5, 0, 0])])]
    rng = np.random.RandomState(46)
    entries = [(k % 4, NQ.random_pose(rng, reflect=bool(k & 2), shift=1.5)) for k in range(12)]
    centre = rng.uniform(-3, 3, (600, 3))
    half = rng.uniform(0.0, 1.5, (600, 3))
    lo, hi = (centre - half).astype(F), (centre + half).astype(F)
    lo[0], hi[0] = -9, 9
    with _World(psm, ctx, meshes, entries) as sc:
        assert [th.info().leaf_count for th in sc.ths] == [0, 1, 2, 3]
        _, count, _, _ = check_boxes(sc, lo, hi, (1, 16))
        assert count[0] == 18 and count.min() == 0
        for one in range(4):                                          # worlds of one: no tree, the instance is entered by every query
            sc.world.setInstances([(sc.ths[one], entries[one][1])])
            sc.which = [one]
            _, c1, _, _ = check_boxes(sc, lo, hi, (2,))
            assert c1[0] == one
        sc.world.setInstances([])                                     # the empty world answers without a tree
        sc.which = []
        assert len(sc.world) == 0
        assert not sc.world.overlapsBox(lo, hi).any() and not sc.world.countInBox(lo, hi).any()
        got = sc.world.trianglesInBox(lo, hi, 5)
        assert (got.tri == -1).all() and (got.geom == -1).all() and not got.count.any() and got.tri.shape == (600, 5)


@pytest.mark.parametrize("n", [1, 63, 65, GRID_CAP * 64 + 65])
def test_world_box_batch_sizes(psm, ctx, n):
    """the last size takes a second trip of the grid-stride loop: the count and the list must start empty again"""
    rng = np.random.RandomState(47)
    entries = [(0, NQ.random_pose(rng, reflect=bool(k & 1), shift=1.0)) for k in range(3)]
    rng = np.random.RandomState(n % 1000)
    centre = rng.uniform(-2.2, 2.2, (n, 3)).astype(F)
    half = rng.uniform(0.0, 0.5, (n, 3)).astype(F)
    with _World(psm, ctx, [_soup(48, 24, 1.0, 0.3)], entries) as sc:
        _, count, _, _ = check_boxes(sc, centre - half, centre + half, (2,))
        if n > 64:
            assert len(np.unique(count)) > 2 and len(np.unique(count[-65:])) > 2


def test_4096_poses_of_the_cube_against_4096_cells(psm, ctx):
    rng = np.random.RandomState(49)
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), axis=-1).reshape(-1, 3)
    entries = [(0, _pose(_rotation(rng, bool(k & 1)), 2.0 * g[k] + rng.uniform(-0.4, 0.4, 3))) for k in range(4096)]
    lo, hi = grid_cells((-1, -1, -1), (32, 32, 32), 16)
    lo, hi = (lo + (hi - lo) * F(0.25)).astype(F), (hi - (hi - lo) * F(0.25)).astype(F)      # the middle half of every cell
    with _World(psm, ctx, [cube()], entries) as sc:
        assert len(sc.world) == 4096
        _, count, _, irows = check_boxes(sc, lo, hi, (4, 16))
        assert (count > 0).sum() > 2000 and (count == 0).sum() > 50 and len(np.unique(irows[irows >= 0])) > 3000


@pytest.mark.parametrize("opt", [ROT_SCALE, SHEAR], ids=["rotate_scale", "shear"])
def test_a_member_built_with_an_optimisation_matrix(psm, ctx, opt):
    rng = np.random.RandomState(50)
    c = rng.uniform(-1, 1, (800, 1, 3)) * [1.0, 0.3, 2.0]
    tris = (c + rng.uniform(-0.08, 0.08, (800, 3, 3))).astype(F)
    entries = [(0, NQ.random_pose(rng, reflect=bool(k & 1), shift=2.0)) for k in range(6)]
    with _World(psm, ctx, [tris], entries, [opt]) as sc:
        t = np.array(sc.ths[0].info().transform).reshape(4, 4)[:3, :3]
        assert np.abs(t - np.diag(np.diag(t))).max() > 0.01
        insts = sc.insts()
        lo, hi = [], []
        for tr, leaves, pose in insts:
            v0 = WB.posed_leaves(tr[np.sort(leaves)], pose)[0]
            pick = v0[rng.randint(0, v0.shape[0], 64)]
            lo.append(pick)                                           # point boxes on posed v0 (they count): the tightest case
            hi.append(pick)
            cc = pick.astype(D) + rng.normal(size=(64, 3)) * 0.05
            h = 10.0 ** rng.uniform(-3, -0.3, (64, 3))
            lo.append(cc - h)
            hi.append(cc + h)
        lo, hi = np.concatenate(lo).astype(F), np.concatenate(hi).astype(F)
        _, count, _, _ = check_boxes(sc, lo, hi, (3, 16), insts)
        assert all((count[128 * j:128 * j + 64] >= 1).all() for j in range(6)) and (count > 16).any()


def test_set_transform_refit_and_refresh(psm, ctx):
    rng = np.random.RandomState(51)
    a, b = _soup(52, 120, 1.0, 0.2), _soup(53, 90, 1.0, 0.2)
    entries = [(k % 2, NQ.random_pose(rng, reflect=bool(k & 1), shift=2.0)) for k in range(9)]
    centre = rng.uniform(-3.5, 3.5, (1500, 3))
    half = 10.0 ** rng.uniform(-2, 0, (1500, 3))
    lo, hi = (centre - half).astype(F), (centre + half).astype(F)
    with _World(psm, ctx, [a, b], entries) as sc:
        _, before, _, _ = check_boxes(sc, lo, hi, (4,))
        sc.world.setTransform(3, NQ.random_pose(rng, shift=2.0))
        sc.world.setTransforms(5, [NQ.random_pose(rng, reflect=True, shift=2.0), NQ.random_pose(rng, shift=2.0)])
        _, after, _, _ = check_boxes(sc, lo, hi, (4, 16))
        assert (before != after).any()
        # a rebuilt member is stale: refused by message, the outputs untouched
        h = sc.ths[1]
        h.markDirty()
        h.build()
        with pytest.raises(psm.PsmError, match="psm_world_box_count_dev: instance 1's hierarchy was rebuilt"):
            sc.world.countInBox(lo, hi)
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
        _, refit, _, _ = check_boxes(sc, lo, hi, (4, 16))
        assert (refit != after).any()


def test_world_box_refusals_launch_nothing(psm, ctx):
    """a stale world, k = 0, k = 17, NULL and misaligned pointers are refused on the host by their messages: the outputs keep
    what they held"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    n = 4
    with _World(psm, ctx, [tri, tri + F(1)], [(0, NQ.IDENTITY), (1, NQ.IDENTITY)]) as sc:
        w = sc.world._w
        hin, hout, hinst, hcnt = ctx.buf_alloc(32 * n), ctx.buf_alloc(4 * 17 * n), ctx.buf_alloc(4 * 17 * n), ctx.buf_alloc(4 * n + 16)
        try:
            boxes = np.zeros((n, 8), F)
            boxes[:, 0:3], boxes[:, 4:7] = -3.0, 3.0
            ctx.buf_upload(hin, boxes)
            ctx.buf_upload(hout, np.full(17 * n, 7, np.int32))
            ctx.buf_upload(hinst, np.full(17 * n, 9, np.int32))
            ctx.buf_upload(hcnt, np.full(n + 4, 77, U))
            pin, pout, pinst, pcnt = (ctypes.c_void_p(ctx.buf_ptr(h)[0]) for h in (hin, hout, hinst, hcnt))
            size = ctypes.c_size_t(n)

            def tris_call(k, p_in=pin, p_out=pout, p_inst=pinst, p_cnt=pcnt, count=size):
                return lib.psm_world_box_triangles_dev(w, p_in, count, ctypes.c_uint32(k), p_out, p_inst, p_cnt)

            def flat_call(fn, p_in=pin, p_out=pcnt, count=size):
                return fn(w, p_in, count, p_out)
            for k in (0, 17, 1 << 31):
                assert tris_call(k) == -1
                assert b"psm_world_box_triangles_dev: k must be 1 .. 16" in lib.psm_last_error(ctx._h)
            assert tris_call(4, p_out=None) == -1 and tris_call(4, p_cnt=None) == -1 and tris_call(4, p_in=None) == -1
            assert tris_call(4, p_inst=None) == -1 and b"NULL pointer" in lib.psm_last_error(ctx._h)
            assert tris_call(4, p_in=ctypes.c_void_p(pin.value + 4)) == -1 and b"boxes not 16-byte aligned" in lib.psm_last_error(ctx._h)
            assert tris_call(4, p_out=ctypes.c_void_p(pout.value + 2)) == -1 and b"tris not 4-byte aligned" in lib.psm_last_error(ctx._h)
            assert tris_call(4, p_inst=ctypes.c_void_p(pinst.value + 2)) == -1 and b"inst not 4-byte aligned" in lib.psm_last_error(ctx._h)
            assert tris_call(4, p_cnt=ctypes.c_void_p(pcnt.value + 2)) == -1 and b"counts not 4-byte aligned" in lib.psm_last_error(ctx._h)
            for fn in (lib.psm_world_box_overlaps_dev, lib.psm_world_box_count_dev):
                assert flat_call(fn, p_in=None) == -1 and flat_call(fn, p_out=None) == -1
                assert flat_call(fn, p_in=ctypes.c_void_p(pin.value + 8)) == -1
                assert flat_call(fn, count=ctypes.c_size_t(0)) == 0
            assert flat_call(lib.psm_world_box_count_dev, p_out=ctypes.c_void_p(pcnt.value + 2)) == -1
            for k in (0, 17):
                with pytest.raises(psm.PsmError, match="k must be 1 .. 16"):
                    sc.world.trianglesInBox(boxes[:, 0:3], boxes[:, 4:7], k)
            sc.ths[1].markDirty()
            sc.ths[1].build()                                          # stale: PSM_ERR_STATE
            assert tris_call(4) == -5 and b"psm_world_box_triangles_dev: instance 1's hierarchy was rebuilt" in lib.psm_last_error(ctx._h)
            for fn in (lib.psm_world_box_overlaps_dev, lib.psm_world_box_count_dev):
                assert flat_call(fn) == -5 and b"instance 1's hierarchy was rebuilt" in lib.psm_last_error(ctx._h)
            ctx.sync()
            assert (ctx.buf_download(hout, np.int32, 17 * n) == 7).all() and (ctx.buf_download(hinst, np.int32, 17 * n) == 9).all()
            assert (ctx.buf_download(hcnt, U, n + 4) == 77).all()
            sc.world.setInstances([(sc.ths[0], NQ.IDENTITY), (sc.ths[1], NQ.IDENTITY)])
            w = sc.world._w
            assert tris_call(16) == 0                                  # and the same buffers are fine at k = 16
            ctx.sync()
            assert (ctx.buf_download(hcnt, U, n) == 2).all()
            rows, irows = ctx.buf_download(hout, np.int32, 17 * n), ctx.buf_download(hinst, np.int32, 17 * n)
            assert (rows[:16 * n].reshape(n, 16) == [0, 0] + [-1] * 14).all() and (rows[16 * n:] == 7).all()
            assert (irows[:16 * n].reshape(n, 16) == [0, 1] + [-1] * 14).all() and (irows[16 * n:] == 9).all()
        finally:
            for h in (hin, hout, hinst, hcnt):
                ctx.buf_free(h)


def test_world_box_torch_tensors_on_a_side_stream(psm, ctx):
    if torch is None:
        pytest.skip("torch is not installed")
    rng = np.random.RandomState(54)
    entries = [(k % 2, NQ.random_pose(rng, reflect=bool(k & 1), shift=3.0)) for k in range(40)]
    centre = rng.uniform(-4, 4, (4099, 3))
    half = 10.0 ** rng.uniform(-2, 0, (4099, 3))
    lo, hi = (centre - half).astype(F), (centre + half).astype(F)
    with _World(psm, ctx, [IQ.icosphere(1, 0.6), _soup(55, 150, 0.8, 0.2)], entries) as sc:
        w = sc.world
        flag, count, lists = w.overlapsBox(lo, hi), w.countInBox(lo, hi), w.trianglesInBox(lo, hi, 5)
        assert flag.any() and not flag.all()
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            tlo, thi = (torch.from_numpy(x).to(dev, non_blocking=True) for x in (lo, hi))
            gflag, gcount, glists = w.overlapsBox(tlo, thi), w.countInBox(tlo, thi), w.trianglesInBox(tlo, thi, 5)
            bufs = [x.cpu() for x in (gflag, gcount, glists.tri, glists.geom, glists.count)]   # (on the side stream: in order)
        assert gflag.device == dev and gflag.dtype == torch.bool and gcount.dtype == torch.int32
        assert glists.tri.shape == (4099, 5) and glists.geom.shape == (4099, 5) and glists.geom.dtype == torch.int32
        _same(bufs[0].numpy(), flag, "torch overlapsBox")
        _same(bufs[1].numpy().view(U), count, "torch countInBox")
        _same(bufs[2].numpy(), lists.tri, "torch trianglesInBox tri")
        _same(bufs[3].numpy(), lists.geom, "torch trianglesInBox inst")
        _same(bufs[4].numpy().view(U), lists.count, "torch trianglesInBox count")
