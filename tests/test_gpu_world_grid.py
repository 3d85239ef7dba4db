"""The voxel grids over an instance world on the GPU (psm_grid_world_surface_dev / _counts_dev / _instances_dev / _solid_dev,
world_grid.hip; InstanceWorld.voxelize / voxelCounts / voxelInstances). The answer is defined as what the world's
box queries answer for every voxel's box, so the yardstick of every case is world.overlapsBox / countInBox / trianglesInBox(lo,
hi, 1).geom[:, 0] on psm.voxel_boxes(...) and world.inside() on psm.voxel_centres(...) -- code that is merged and held to numpy
models of its own --, and for grids of at most 1 000 voxels also tests/world_grid_query_model.py. Every comparison is exact, and in
every case voxelize(...).dense() == (voxelCounts(...) > 0) == (voxelInstances(...) >= 0)."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import grid_query_model as GQ
import inside_query_model as IQ
import instance_query_model as NQ
import query_model as Q
import world_grid_query_model as WG
from test_gpu_grid_query import GRID_CAP, SHEAR
from test_gpu_world_box import _World, _soup
from util import ROOT

try:   # (imported before the library loads its HIP runtime: see test_gpu_query.py)
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = np.argwhere(a != b)
    assert bad.shape[0] == 0, "%s: %d differ, first at %s: %s against %s" % (what, bad.shape[0], bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


def _world_grid(sc, dims, grow=0.02):
    """a grid of `dims` voxels over the bounds of the posed triangles of every instance, grown by a fraction of the extent"""
    pts = np.concatenate([NQ.to_world(m, sc.meshes[k].reshape(-1, 3)) for k, m in zip(sc.which, sc.world.transforms())])
    lo, hi = pts.min(0), pts.max(0)
    lo, hi = lo - grow * (hi - lo), hi + grow * (hi - lo)
    return tuple(lo), tuple((hi - lo) / np.asarray(dims, np.float64)), tuple(dims)


def check_grid(psm, sc, grid, model=None):
    """surface, counts and owners of `grid` against the world's box queries on the voxels' boxes, against the model where the
    grid is small (or where `model` says), and against one another; returns (dense flags, counts, owners)"""
    nx, ny, nz = grid[2]
    w = sc.world
    lo, hi = psm.voxel_boxes(*grid)
    flag = w.overlapsBox(lo, hi).reshape(nz, ny, nx)
    count = w.countInBox(lo, hi).reshape(nz, ny, nx)
    owner = np.ascontiguousarray(w.trianglesInBox(lo, hi, 1).geom[:, 0]).reshape(nz, ny, nx)
    vg = w.voxelize(*grid)
    got = w.voxelCounts(*grid)
    lab = w.voxelInstances(*grid)
    nb = ((nz + 3) // 4, (ny + 3) // 4, (nx + 3) // 4)
    assert vg.bricks.shape == nb and vg.bricks.dtype == np.uint64 and vg.dims == (nx, ny, nz)
    assert got.shape == (nz, ny, nx) and got.dtype == U and lab.shape == (nz, ny, nx) and lab.dtype == np.int32
    _same(got, count, "voxelCounts against countInBox")
    _same(lab, owner, "voxelInstances against trianglesInBox(k = 1)")
    dense = vg.dense()
    _same(dense, flag, "voxelize against overlapsBox")
    assert vg.occupied() == int(flag.sum())                         # the padding bits are 0 ...
    if nx * ny * nz <= 100000:
        _same(vg.bricks, GQ.pack_bricks(flag), "the brick words")   # ... and every bit is where the header says
    assert np.array_equal(dense, got > 0) and np.array_equal(dense, lab >= 0)
    if model if model is not None else nx * ny * nz <= 1000:
        mdense, mcount, mowner = WG.answers(sc.insts(), grid)
        _same(got, mcount, "voxelCounts against the model")
        _same(lab, mowner, "voxelInstances against the model")
        _same(vg.bricks, GQ.pack_bricks(mdense), "voxelize against the model")
    return dense, got, lab


def _rigid(n, seed, shift=1.0, reflect=(1,)):
    rng = np.random.RandomState(seed)
    return [NQ.random_pose(rng, reflect=k in reflect, shift=shift) for k in range(n)]


def test_world_grid_lattice_world(psm, ctx):
    """all arithmetic exact: two lattice soups at five signed axis permutations with translations on the 1/8 lattice, the 8^3 grid
    of [-1, 1]^3 and the same moved by half a cell along one, two and three axes; the counts are the integers'"""
    soups, entries = WG.lattice_world()
    with _World(psm, ctx, soups, entries) as sc:
        for grid in GQ.LATTICE_GRIDS:
            dense, count, owner = check_grid(psm, sc, grid)
            _same(count, WG.exact_counts(sc.insts(), grid), "the counts against the integers'")
            assert dense.sum() > 100 and (~dense).sum() > 5 and count.max() > 4 and len(np.unique(owner)) > 3
    # and directly: a triangle posed into the face y = 0 is counted by the voxel on either side of it, and by no other
    face = np.array([[[0, 0.05, 0.05], [0, 0.2, 0.05], [0, 0.05, 0.2]]], F)
    pose = np.array([[0, 1, 0, 0.5], [1, 0, 0, 0.0], [0, 0, -1, 0.25]], F)
    with _World(psm, ctx, [face], [(0, pose)]) as sc:
        _, c2, o2 = check_grid(psm, sc, GQ.LATTICE_GRIDS[0])
        assert c2.sum() == 2 and c2[4, 3, 6] == 1 and c2[4, 4, 6] == 1 and (o2[c2 > 0] == 0).all()


@pytest.mark.parametrize("dims", [(5, 7, 9), (1, 1, 1), (4, 4, 4), (3, 1, 130)], ids=lambda d: "x".join(map(str, d)))
def test_world_grid_partial_bricks(psm, ctx, dims):
    meshes = [_soup(41, 300, 1.0, 0.15), _soup(42, 300, 0.7, 0.1)]
    poses = _rigid(6, 43, shift=1.5, reflect=(3,))
    assert np.linalg.det(poses[3][:, :3].astype(np.float64)) < 0
    with _World(psm, ctx, meshes, [(k % 2, m) for k, m in enumerate(poses)]) as sc:
        dense, count, owner = check_grid(psm, sc, _world_grid(sc, dims))
        assert count.size == dims[0] * dims[1] * dims[2] and dense.any()
        if dims == (1, 1, 1):
            assert count[0, 0, 0] == 3 * sum(th.info().leaf_count for th in sc.ths) and owner[0, 0, 0] == 0   # the whole world
        else:
            assert len(np.unique(owner)) > 3 and (dims == (4, 4, 4) or not dense.all())


def test_world_grid_of_one_at_the_identity_equals_the_hierarchy(psm, ctx):
    """no tree over the instances: the one instance is entered directly; bricks and counts are the hierarchy's own, byte for byte"""
    tris = _soup(44, 700, 1.0, 0.1)
    with _World(psm, ctx, [tris], [(0, NQ.IDENTITY)]) as sc:
        th = sc.ths[0]
        for dims in ((9, 9, 9), (21, 6, 13)):
            grid = _world_grid(sc, dims)
            dense, count, owner = check_grid(psm, sc, grid)
            _same(sc.world.voxelize(*grid).bricks, th.voxelize(*grid).bricks, "the world's bricks against the hierarchy's")
            _same(count, th.voxelCounts(*grid), "the world's counts against the hierarchy's")
            assert dense.any() and not dense.all() and np.array_equal(owner, np.where(dense, 0, -1).astype(np.int32))


def test_world_grid_empty_and_tiny_instances(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    degenerate = np.repeat(tri[:, :1], 3, axis=1)                    # three equal vertices: the build keeps no leaf
    grid = ((-1.5, -1.5, -1.5), 0.6, (5, 5, 5))
    with _World(psm, ctx, [tri], []) as sc:                          # an empty world: zeros and -1, no query kernel
        assert len(sc.world) == 0
        dense, count, owner = check_grid(psm, sc, grid)
        assert not dense.any() and not count.any() and (owner == -1).all()
        assert not sc.world.voxelize(*grid, solid=True).bricks.any()
    body = _soup(45, 60, 0.8, 0.2)
    shift = np.array([[1, 0, 0, -1.0], [0, 1, 0, 0.25], [0, 0, 1, 0.0]], F)
    with _World(psm, ctx, [np.concatenate([degenerate] * 4), np.concatenate([degenerate, tri, degenerate]), body],
                [(0, NQ.IDENTITY), (1, shift), (2, NQ.IDENTITY), (1, shift)]) as sc:
        assert [th.info().leaf_count for th in sc.ths] == [0, 1, 60]
        dense, count, owner = check_grid(psm, sc, grid)
        assert dense.any() and not dense.all() and set(np.unique(owner)) == {-1, 1, 2}   # the zero-leaf body owns nothing
        # the one-leaf body stands there twice: its counts double, and the owner is the lower index
        with _World(psm, ctx, [tri], [(0, shift)]) as one, _World(psm, ctx, [body], [(0, NQ.IDENTITY)]) as rest:
            c1, c2 = one.world.voxelCounts(*grid), rest.world.voxelCounts(*grid)
        _same(count, (2 * c1 + c2).astype(U), "two coincident instances count twice")
        assert c1.any() and (owner[c1 > 0] == 1).all() and not (owner == 3).any()


def test_world_grid_many_small_bodies(psm, ctx):
    """300 instances of one 20-triangle hierarchy: a brick meets many instances, the tree over them is several levels deep"""
    rng = np.random.RandomState(46)
    poses = [NQ.random_pose(rng, reflect=bool(k % 7 == 0), shift=3.0) for k in range(300)]
    with _World(psm, ctx, [_soup(47, 20, 0.3, 0.15)], [(0, m) for m in poses]) as sc:
        dense, count, owner = check_grid(psm, sc, _world_grid(sc, (9, 9, 9)))
        assert dense.any() and not dense.all() and len(np.unique(owner)) > 30 and count.max() > 5


def test_world_grid_more_bricks_than_workgroups(psm, ctx, scenes):
    """9 261 bricks: the grid-stride loop takes a second trip, and the per-brick state starts again for every brick"""
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3)
    assert (84 // 4) ** 3 > GRID_CAP
    poses = _rigid(3, 48, shift=0.8, reflect=(2,))
    with _World(psm, ctx, [tris], [(0, m) for m in poses]) as sc:
        dense, count, owner = check_grid(psm, sc, _world_grid(sc, (84, 84, 84), 0.01))
        far = dense.reshape(-1)[GRID_CAP * 64:]                       # (dense order is not brick order: a coarse look at both ends)
        assert dense.any() and not dense.all() and far.any() and not far.all() and len(np.unique(count)) > 2
        assert len(np.unique(owner)) >= 3


def test_world_grid_deep_hierarchy_among_others(psm, ctx):
    """a hierarchy deeper than the 16 LDS entries of a lane's own stack, posed, among three others: the wave's one stack carries
    the tree over the instances and the deep hierarchy"""
    deep, _, _ = Q.deep_fixture()
    poses = _rigid(4, 49, shift=1.0, reflect=(0,))
    with _World(psm, ctx, [deep, _soup(50, 100, 0.8, 0.2)], [(1, poses[0]), (0, poses[1]), (1, poses[2]), (1, poses[3])]) as sc:
        dense, count, owner = check_grid(psm, sc, _world_grid(sc, (6, 6, 6)))
        assert int(count.max()) > 64 and dense.any() and not dense.all() and len(np.unique(owner)) >= 3
        one = _world_grid(sc, (1, 1, 1))
        assert sc.world.voxelCounts(*one)[0, 0, 0] == sc.ths[0].info().leaf_count + 3 * sc.ths[1].info().leaf_count


def test_world_grid_build_matrix(psm, ctx):
    """a hierarchy built under a shear, as an instance at a rotated pose: the intervals of the prune use the full 3 x 3 part"""
    rng = np.random.RandomState(35)
    c = rng.uniform(-1, 1, (1500, 1, 3)) * [1.0, 0.3, 2.0]
    tris = (c + rng.uniform(-0.08, 0.08, (1500, 3, 3))).astype(F)
    poses = _rigid(2, 51, shift=0.5, reflect=())
    with _World(psm, ctx, [tris, _soup(52, 80, 0.5, 0.2)], [(0, poses[0]), (1, poses[1])], opts=[SHEAR, None]) as sc:
        m = np.array(sc.ths[0].info().transform).reshape(4, 4)[:3, :3]
        assert np.abs(m - np.diag(np.diag(m))).max() > 0.01
        dense, count, owner = check_grid(psm, sc, _world_grid(sc, (9, 9, 9), 0.05))
        assert count.max() >= 10 and (~dense).sum() > 20 and (owner == 0).any() and (owner == 1).any()


def test_world_grid_after_moving_a_body(psm, ctx):
    poses = _rigid(4, 53, shift=1.0, reflect=(2,))
    with _World(psm, ctx, [IQ.icosphere(1, 0.6), _soup(54, 150, 0.6, 0.2)], [(k % 2, m) for k, m in enumerate(poses)]) as sc:
        grid = _world_grid(sc, (9, 9, 9), 0.3)
        before = check_grid(psm, sc, grid)
        sc.world.setTransform(1, NQ.random_pose(np.random.RandomState(55), reflect=True, shift=1.0))
        after = check_grid(psm, sc, grid)
        assert (before[0] != after[0]).any() and (before[2] != after[2]).any() and after[0].any() and not after[0].all()


def test_world_grid_after_refit(psm, ctx, scenes):
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3).copy()
    poses = _rigid(2, 56, shift=0.5, reflect=(1,))
    with _World(psm, ctx, [tris], [(0, m) for m in poses]) as sc:
        th = sc.ths[0]
        grid = _world_grid(sc, (9, 9, 9))
        before, _, _ = check_grid(psm, sc, grid)
        blo, bhi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
        moved = tris.copy()
        rng = np.random.RandomState(9)
        k = rng.choice(tris.shape[0], 8, replace=False)
        c = moved[k].mean(axis=1, keepdims=True)
        moved[k] = (c + (moved[k] - c) * F(0.5) + rng.uniform(-0.3, 0.3, (8, 1, 3)).astype(F)).astype(F)
        moved = np.clip(moved, blo, bhi).astype(F)                    # within the build's bounds
        th.clearTribuffer()
        th.loadTriangles(moved.reshape(-1, 9))
        th.refit()
        sc.world.refresh()                                            # (the world stays valid: no instance is set anew)
        sc.meshes[0] = moved
        after, _, _ = check_grid(psm, sc, grid)
        assert (before != after).any() and after.any() and not after.all()


SPHERE_GRID = ((-1.6, -1.6, -1.6), 0.2, (16, 16, 16))
SPHERE_POSES = [np.array([[1, 0, 0, -0.4], [0, 1, 0, 0.1], [0, 0, 1, 0.0]], F),
                np.array([[0, -1, 0, 0.5], [-1, 0, 0, -0.2], [0, 0, 1, 0.3]], F)]      # the second: a reflection


def _solid_expected(psm, w, grid, samples):
    nx, ny, nz = grid[2]
    lo, hi = psm.voxel_boxes(*grid)
    return (w.overlapsBox(lo, hi) | w.inside(psm.voxel_centres(*grid), samples)).reshape(nz, ny, nx)


@pytest.mark.parametrize("samples", [1, 3, 5])
def test_world_grid_solid_fills_closed_bodies(psm, ctx, samples):
    assert np.linalg.det(SPHERE_POSES[1][:, :3].astype(np.float64)) < 0
    with _World(psm, ctx, [IQ.icosphere(2)], [(0, m) for m in SPHERE_POSES]) as sc:
        w = sc.world
        for grid in (SPHERE_GRID, ((-1.6, -1.5, -1.7), (0.65, 0.43, 0.38), (5, 7, 9))):   # whole bricks, and partial ones
            expect = _solid_expected(psm, w, grid, samples)
            vg = w.voxelize(*grid, solid=True, samples=samples)
            _same(vg.dense(), expect, "solid against surface | inside")
            _same(vg.bricks, GQ.pack_bricks(expect), "the solid brick words")            # the padding bits stay 0
        surface = w.voxelize(*SPHERE_GRID).occupied()
        filled = w.voxelize(*SPHERE_GRID, solid=True, samples=samples).occupied()
        assert 0 < surface < filled < 16 ** 3


def test_world_grid_solid_takes_more_than_one_slab(psm, ctx):
    """68 921 bricks: more than the 65 536 whose centres and flags solid's scratch holds at a time"""
    dims = (164, 164, 164)
    grid = ((-1.6, -1.6, -1.6), 3.2 / 164, dims)
    with _World(psm, ctx, [IQ.icosphere(2)], [(0, m) for m in SPHERE_POSES]) as sc:
        vg = sc.world.voxelize(*grid, solid=True, samples=1)
        expect = _solid_expected(psm, sc.world, grid, 1)
        _same(vg.dense(), expect, "solid over two slabs")
        assert vg.occupied() == int(expect.sum()) and expect[-40:].any() and not expect.all() and expect[82, 87, 61]


def test_world_grid_torch_side_stream_and_graph(psm, ctx, scenes):
    if torch is None:
        pytest.skip("torch is not installed")
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3)
    poses = _rigid(3, 57, shift=0.8, reflect=(1,))
    with _World(psm, ctx, [tris], [(0, m) for m in poses]) as sc:
        w = sc.world
        grid = _world_grid(sc, (21, 18, 23))
        vg, count, owner = w.voxelize(*grid), w.voxelCounts(*grid), w.voxelInstances(*grid)
        solid = w.voxelize(*grid, solid=True, samples=3)
        assert vg.dense().any() and not vg.dense().all()
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            tvg, tcount = w.voxelize(*grid, as_torch=True), w.voxelCounts(*grid, as_torch=True)
            towner = w.voxelInstances(*grid, as_torch=True)
            tsolid = w.voxelize(*grid, solid=True, samples=3, as_torch=True)
            agree = torch.equal(tvg.dense(), tcount > 0) and torch.equal(tcount > 0, towner >= 0)   # no host synchronisation before it
            bufs = [x.cpu() for x in (tvg.bricks, tcount, towner, tsolid.bricks)]   # (on the side stream: in order)
        assert agree and tvg.bricks.device == dev and tvg.bricks.dtype == torch.int64 and tcount.dtype == torch.int32
        assert towner.dtype == torch.int32 and tuple(towner.shape) == (23, 18, 21) and tvg.dims == (21, 18, 23)
        _same(bufs[0].numpy().view(np.uint64), vg.bricks, "torch voxelize")
        _same(bufs[1].numpy().view(U), count, "torch voxelCounts")
        _same(bufs[2].numpy(), owner, "torch voxelInstances")
        _same(bufs[3].numpy().view(np.uint64), solid.bricks, "torch voxelize solid")
        # surface, counts and instances allocate nothing: captured after the warm calls above into one linear chain, replayed twice
        lib = psm.lib()
        g = psm._grid(*grid)
        words = torch.zeros(tuple(vg.bricks.shape), dtype=torch.int64, device=dev)
        cells = torch.zeros(tuple(count.shape), dtype=torch.int32, device=dev)
        labels = torch.zeros(tuple(owner.shape), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            def launch():
                assert lib.psm_grid_world_surface_dev(w._w, ctypes.byref(g), ctypes.c_void_p(words.data_ptr())) == 0
                assert lib.psm_grid_world_counts_dev(w._w, ctypes.byref(g), ctypes.c_void_p(cells.data_ptr())) == 0
                assert lib.psm_grid_world_instances_dev(w._w, ctypes.byref(g), ctypes.c_void_p(labels.data_ptr())) == 0
            psm._torch_ordered(ctx, dev, launch)     # side -> the context's stream (the three launches, in order) -> side
        for _ in range(2):
            words.fill_(0x55)
            cells.fill_(7)
            labels.fill_(9)
            graph.replay()
            torch.cuda.synchronize()
            _same(words.cpu().numpy().view(np.uint64), vg.bricks, "replayed surface")
            _same(cells.cpu().numpy().view(U), count, "replayed counts")
            _same(labels.cpu().numpy(), owner, "replayed instances")
    torch.cuda.synchronize()


def test_world_grid_refusals_launch_nothing(psm, ctx):
    """invalid grids, NULL and misaligned outputs, samples = 0, 2, 4, 6 and a stale world are refused on the host: the outputs
    keep what they held; the same buffers then take a good call, which writes its extent and nothing past it"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    good = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
    hw, hc = ctx.buf_alloc(8 * 8 + 16), ctx.buf_alloc(4 * 512 + 16)
    with _World(psm, ctx, [tri, _soup(58, 30, 0.8, 0.3)], [(0, NQ.IDENTITY), (1, NQ.IDENTITY)]) as sc:
        w = sc.world
        try:
            ctx.buf_upload(hw, np.full(10, 0x7777777777777777, np.uint64))
            ctx.buf_upload(hc, np.full(516, 77, U))
            pw, pc = ctx.buf_ptr(hw)[0], ctx.buf_ptr(hc)[0]

            def by(grid):
                return ctypes.byref(grid) if grid is not None else None

            def surface(grid=good, p=pw, world=w._w):
                return lib.psm_grid_world_surface_dev(world, by(grid), ctypes.c_void_p(p))

            def counts(grid=good, p=pc, world=w._w):
                return lib.psm_grid_world_counts_dev(world, by(grid), ctypes.c_void_p(p))

            def instances(grid=good, p=pc, world=w._w):
                return lib.psm_grid_world_instances_dev(world, by(grid), ctypes.c_void_p(p))

            def solid(samples=3, grid=good, p=pw, world=w._w):
                return lib.psm_grid_world_solid_dev(world, by(grid), ctypes.c_uint32(samples), ctypes.c_void_p(p))

            calls = (surface, counts, instances, solid)
            bad = []
            for field, k, value in (("dims", 0, 0), ("dims", 2, (1 << 20) + 1), ("cell", 1, 0.0), ("cell", 0, -1.0), ("cell", 2, np.nan),
                                    ("cell", 1, np.inf), ("origin", 0, np.inf), ("origin", 2, np.nan), ("cell", 1, 1e38)):
                g = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
                getattr(g, field)[k] = value                           # (the last one: the last voxel's hi, -2 + 8e38, is not finite)
                bad.append(g)
            huge = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
            huge.dims[:] = [1 << 20, 1 << 20, 8]                       # 2^37 bricks
            huge.cell[:] = [1e-3, 1e-3, 1e-3]
            for g in bad + [huge]:
                for call in calls:
                    assert call(grid=g) == -1 and b"invalid grid" in lib.psm_last_error(ctx._h)
            for call in calls:
                assert call(grid=None) == -1 and call(p=None) == -1 and call(world=None) == -1
            assert surface(p=pw + 4) == -1 and b"bricks not 8-byte aligned" in lib.psm_last_error(ctx._h)
            assert solid(p=pw + 4) == -1 and counts(p=pc + 2) == -1 and b"counts not 4-byte aligned" in lib.psm_last_error(ctx._h)
            assert instances(p=pc + 2) == -1 and b"inst not 4-byte aligned" in lib.psm_last_error(ctx._h)
            for s in (0, 2, 4, 6):
                assert solid(samples=s) == -1 and b"samples must be 1, 3 or 5" in lib.psm_last_error(ctx._h)
            with pytest.raises(psm.PsmError):
                w.voxelize((-2, -2, -2), 0.5, (8, 8, 8), solid=True, samples=2)
            with pytest.raises(ValueError):
                w.voxelInstances((-2, -2, -2), 0.0, (8, 8, 8))
            sc.ths[1].markDirty()
            sc.ths[1].build()                                          # a member is rebuilt: the world is stale until it is set anew
            for call in calls:
                assert call() == -5 and b"set the instances again" in lib.psm_last_error(ctx._h)      # PSM_ERR_STATE
            ctx.sync()
            assert (ctx.buf_download(hw, np.uint64, 10) == 0x7777777777777777).all() and (ctx.buf_download(hc, U, 516) == 77).all()
            w.setInstances([(sc.ths[0], NQ.IDENTITY), (sc.ths[1], NQ.IDENTITY)])
            # and the same buffers are fine: 8 words and 512 counts are written, nothing past them
            assert surface() == 0 and counts(p=pc + 4) == 0
            ctx.sync()
            words, cells = ctx.buf_download(hw, np.uint64, 10), ctx.buf_download(hc, U, 516)
            assert (words[8:] == 0x7777777777777777).all() and cells[0] == 77 and (cells[513:] == 77).all()
            _same(words[:8].reshape(2, 2, 2), w.voxelize((-2, -2, -2), 0.5, (8, 8, 8)).bricks, "the raw call")
            _same(cells[1:513].reshape(8, 8, 8), w.voxelCounts((-2, -2, -2), 0.5, (8, 8, 8)), "the raw counts")
            assert words[:8].any() and (cells[1:513] == 0).any() and cells[1:513].sum() > 4
            assert instances(p=pc + 4) == 0
            ctx.sync()
            cells = ctx.buf_download(hc, np.int32, 516)
            assert cells[0] == 77 and (cells[513:] == 77).all()
            _same(cells[1:513].reshape(8, 8, 8), w.voxelInstances((-2, -2, -2), 0.5, (8, 8, 8)), "the raw labels")
            assert set(np.unique(cells[1:513])) == {-1, 0, 1}
        finally:
            ctx.buf_free(hw)
            ctx.buf_free(hc)


def test_world_grid_header_layer(psm, ctx, tmp_path):
    """psm::InstanceWorld::voxelize / voxelizeSolid / voxelCounts / voxelInstances (tests/cpp/world_grid_host.cpp, a process of
    its own): the same bricks, counts and labels as Python's"""
    exe = str(tmp_path / "world_grid_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "world_grid_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    tris = IQ.icosphere(2)
    grid = ((-1.6, -1.5, -1.7), (0.29, 0.27, 0.34), (11, 12, 10))
    g = psm._grid(*grid)
    inp, out = str(tmp_path / "grid.in"), str(tmp_path / "grid.out")
    with open(inp, "wb") as f:
        f.write(struct.pack("<i", tris.shape[0]))
        f.write(tris.astype("<f4").tobytes())
        f.write(struct.pack("<i", len(SPHERE_POSES)))
        for m in SPHERE_POSES:
            m4 = np.eye(4, dtype=F)
            m4[:3] = m
            f.write(np.ascontiguousarray(m4.T).astype("<f4").tobytes())    # glm::mat4: column-major
        f.write(bytes(g))
        f.write(struct.pack("<I", 3))
    subprocess.check_call([exe, inp, out], timeout=120)
    raw = open(out, "rb").read()
    nb = struct.unpack_from("<Q", raw, 0)[0]
    assert nb == 3 * 3 * 3
    surface = np.frombuffer(raw, np.uint64, nb, 8).reshape(3, 3, 3)
    solid = np.frombuffer(raw, np.uint64, nb, 8 + 8 * nb).reshape(3, 3, 3)
    nv = struct.unpack_from("<Q", raw, 8 + 16 * nb)[0]
    assert nv == 11 * 12 * 10
    cells = np.frombuffer(raw, U, nv, 16 + 16 * nb).reshape(10, 12, 11)
    labels = np.frombuffer(raw, np.int32, nv, 16 + 16 * nb + 4 * nv).reshape(10, 12, 11)
    with _World(psm, ctx, [tris], [(0, m) for m in SPHERE_POSES]) as sc:
        w = sc.world
        _same(surface, w.voxelize(*grid).bricks, "the header layer's voxelize")
        _same(solid, w.voxelize(*grid, solid=True, samples=3).bricks, "the header layer's voxelizeSolid")
        _same(cells, w.voxelCounts(*grid), "the header layer's voxelCounts")
        _same(labels, w.voxelInstances(*grid), "the header layer's voxelInstances")
        assert surface.any() and (solid != surface).any() and set(np.unique(labels)) == {-1, 0, 1}
