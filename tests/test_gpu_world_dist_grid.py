"""The distance-field grids over an instance world on the GPU (psm_grid_world_distance_dev / psm_grid_world_signed_distance_dev,
world_grid_dist.hip; InstanceWorld.distanceField). The answer is defined as what the world's point queries answer
for every voxel's centre, so the yardstick of every case is world.closestPoint / world.signedDistance on psm.voxel_centres(...)
with the same rmax and samples -- code that is merged and held to numpy models of its own --, and for grids of at most 1 000
voxels also tests/world_dist_grid_model.py over the downloaded leaves. Every comparison is exact: dist is compared through a
uint32 view, so -0.0, +inf and NaN cannot hide."""
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
import world_dist_grid_model as WD
import world_grid_query_model as WG
import world_pose_cases as PC
from test_gpu_grid_query import GRID_CAP, ROT_SCALE, SHEAR
from test_gpu_world_box import _World, _soup
from test_gpu_world_grid import _rigid, _world_grid
from test_world_dist_grid_cpu import (LATTICE_RMAX, LATTICE_WORTH, SIGNED_GRIDS, SIGNED_KINDS, SIGNED_POSES, SIGNED_RMAX, signed_world)
from util import ROOT

try:   # (imported before the library loads its HIP runtime: see test_gpu_query.py)
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
INF_BITS = 0x7F800000


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == F:
        a, b = a.view(U), b.view(U)
    bad = np.argwhere(a != b)
    assert bad.shape[0] == 0, "%s: %d differ, first at %s: %s against %s" % (what, bad.shape[0], bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


def check_field(psm, sc, grid, rmax=np.inf, signed=False, samples=3, model=None, insts=None):
    """the field of `grid` against the world's point query over the voxels' centres, with and without the ids, and against the
    model where the grid is small (or where `model` says); returns (dist, tri, inst)"""
    nx, ny, nz = grid[2]
    w = sc.world
    centres = psm.voxel_centres(*grid)
    ref = w.signedDistance(centres, rmax, samples) if signed else w.closestPoint(centres, rmax)
    got = w.distanceField(*grid, rmax=rmax, signed=signed, samples=samples)
    assert got.dist.shape == got.tri.shape == got.inst.shape == (nz, ny, nx)
    assert got.dist.dtype == F and got.tri.dtype == np.int32 and got.inst.dtype == np.int32
    assert got.dims == (nx, ny, nz) and got.dist.size == nx * ny * nz
    kind = "signedDistance" if signed else "closestPoint"
    _same(got.dist, np.ascontiguousarray(ref.t).reshape(nz, ny, nx), "dist against %s" % kind)
    _same(got.tri, np.ascontiguousarray(ref.tri).reshape(nz, ny, nx), "tri against %s" % kind)
    _same(got.inst, np.ascontiguousarray(ref.geom).reshape(nz, ny, nx), "inst against %s" % kind)
    alone = w.distanceField(*grid, rmax=rmax, signed=signed, samples=samples, nearest=False)
    assert alone.tri is None and alone.inst is None
    _same(alone.dist, got.dist, "dist without the ids")
    miss = got.tri < 0
    assert np.array_equal(miss, got.inst < 0) and (got.tri[miss] == -1).all() and (got.inst[miss] == -1).all()
    assert (got.dist[miss].view(U) == INF_BITS).all() and np.isfinite(got.dist[~miss]).all()
    if model if model is not None else nx * ny * nz <= 1000:
        insts = sc.insts() if insts is None else insts
        mdist, mtri, minst = WD.signed_field(insts, grid, rmax, samples) if signed else WD.field(insts, grid, rmax)
        _same(got.dist, mdist, "dist against the model")
        _same(got.tri, mtri, "tri against the model")
        _same(got.inst, minst, "inst against the model")
    return got.dist, got.tri, got.inst


def test_world_dist_grid_lattice_world(psm, ctx):
    """all arithmetic exact: two lattice soups at five signed axis permutations with translations on the 1/8 lattice, the 8^3 grid
    of [-1, 1]^3 and the same moved by half a cell along one, two and three axes: voxels where two or more instances hold the
    bit-equal smallest d2 (tests/test_world_dist_grid_cpu.py counts them), centres that lie on a triangle, and misses"""
    soups, entries = WG.lattice_world()
    with _World(psm, ctx, soups, entries) as sc:
        for grid, (_, _, zeros, misses) in zip(GQ.LATTICE_GRIDS, LATTICE_WORTH):
            dist, tri, inst = check_field(psm, sc, grid)
            assert int((dist == 0).sum()) == zeros and (tri >= 0).all() and not (inst == 4).any() and (inst == 1).any()
            near, ntri, ninst = check_field(psm, sc, grid, rmax=LATTICE_RMAX)
            assert int((ntri < 0).sum()) == misses and not (ninst == 4).any()
            hit = ntri >= 0
            _same(near[hit], dist[hit], "the band keeps the values within it")


@pytest.mark.parametrize("dims", [(5, 7, 9), (1, 1, 1), (4, 4, 4), (3, 1, 130)], ids=lambda d: "x".join(map(str, d)))
def test_world_dist_grid_partial_bricks(psm, ctx, dims):
    meshes = [_soup(41, 300, 1.0, 0.15), _soup(42, 300, 0.7, 0.1)]
    poses = _rigid(6, 43, shift=1.5, reflect=(3,))
    assert np.linalg.det(poses[3][:, :3].astype(np.float64)) < 0
    with _World(psm, ctx, meshes, [(k % 2, m) for k, m in enumerate(poses)]) as sc:
        grid = _world_grid(sc, dims, 0.15)
        dist, tri, inst = check_field(psm, sc, grid)
        assert (tri >= 0).all() and (dims == (1, 1, 1) or len(np.unique(inst)) > 3)
        if dims != (1, 1, 1):
            band = float(np.median(dist))          # half of the voxels lie within it
            near, ntri, _ = check_field(psm, sc, grid, rmax=band)
            assert (ntri >= 0).any() and (ntri < 0).any()


def test_world_dist_grid_of_one_at_the_identity_equals_the_hierarchy(psm, ctx):
    """no tree over the instances: the one instance is entered directly; dist and tri are the hierarchy's own, byte for byte"""
    tris = _soup(44, 700, 1.0, 0.1)
    with _World(psm, ctx, [tris], [(0, NQ.IDENTITY)]) as sc:
        th = sc.ths[0]
        for dims, rmax in (((9, 9, 9), np.inf), ((21, 6, 13), 0.12)):
            grid = _world_grid(sc, dims, 0.2)
            dist, tri, inst = check_field(psm, sc, grid, rmax=rmax)
            own = th.distanceField(*grid, rmax=rmax)
            _same(dist, own.dist, "the world's dist against the hierarchy's")
            _same(tri, own.tri, "the world's tri against the hierarchy's")
            assert np.array_equal(inst, np.where(tri >= 0, 0, -1).astype(np.int32)) and (tri >= 0).any()
            signed = sc.world.distanceField(*grid, rmax=rmax, signed=True, samples=3)
            _same(signed.dist, th.distanceField(*grid, rmax=rmax, signed=True, samples=3).dist, "the world's signed dist against the hierarchy's")
        assert (tri < 0).any()


def test_world_dist_grid_empty_and_tiny_instances(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    degenerate = np.repeat(tri[:, :1], 3, axis=1)                    # three equal vertices: the build keeps no leaf
    grid = ((-1.5, -1.5, -1.5), 0.6, (5, 5, 5))
    with _World(psm, ctx, [tri], []) as sc:                          # an empty world: +inf, -1, -1, no query kernel
        assert len(sc.world) == 0
        for signed in (False, True):
            dist, ids, inst = check_field(psm, sc, grid, signed=signed, model=False)
            assert (dist.view(U) == INF_BITS).all() and (ids == -1).all() and (inst == -1).all()
    body = _soup(45, 60, 0.8, 0.2)
    shift = np.array([[1, 0, 0, -1.0], [0, 1, 0, 0.25], [0, 0, 1, 0.0]], F)
    with _World(psm, ctx, [np.concatenate([degenerate] * 4), np.concatenate([degenerate, tri, degenerate]), body],
                [(0, NQ.IDENTITY), (1, shift), (2, NQ.IDENTITY), (1, shift)]) as sc:
        assert [th.info().leaf_count for th in sc.ths] == [0, 1, 60]
        dist, ids, inst = check_field(psm, sc, grid)
        assert set(np.unique(inst)) == {1, 2}                        # the zero-leaf body owns nothing, the second copy never wins
        near, nids, ninst = check_field(psm, sc, grid, rmax=0.4)
        assert set(np.unique(ninst)) == {-1, 1, 2}
        check_field(psm, sc, grid, rmax=0.4, signed=True)
    # two coincident instances: the lower one owns every voxel
    with _World(psm, ctx, [body], [(0, shift), (0, shift)]) as sc:
        _, _, inst = check_field(psm, sc, grid)
        assert (inst == 0).all()


def test_world_dist_grid_many_small_bodies(psm, ctx):
    """300 instances of one 20-triangle hierarchy: a brick meets many instances, the tree over them is several levels deep"""
    rng = np.random.RandomState(46)
    poses = [NQ.random_pose(rng, reflect=bool(k % 7 == 0), shift=3.0) for k in range(300)]
    with _World(psm, ctx, [_soup(47, 20, 0.3, 0.15)], [(0, m) for m in poses]) as sc:
        grid = _world_grid(sc, (12, 12, 12))
        dist, tri, inst = check_field(psm, sc, grid, model=False)
        assert len(np.unique(inst)) > 100 and (tri >= 0).all()
        near, ntri, ninst = check_field(psm, sc, grid, rmax=0.3, model=False)
        assert (ntri >= 0).any() and (ntri < 0).any() and len(np.unique(ninst)) > 50


def test_world_dist_grid_more_bricks_than_workgroups(psm, ctx, scenes):
    """9 261 bricks: the grid-stride loop takes a second trip, and the per-brick state starts again for every brick; a band of
    two cell diagonals keeps the walks short"""
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3)
    assert (84 // 4) ** 3 > GRID_CAP
    poses = _rigid(3, 48, shift=0.8, reflect=(2,))
    with _World(psm, ctx, [tris], [(0, m) for m in poses]) as sc:
        grid = _world_grid(sc, (84, 84, 84), 0.01)
        rmax = 2.0 * float(np.linalg.norm(np.asarray(grid[1], np.float64)))
        dist, tri, inst = check_field(psm, sc, grid, rmax=rmax)
        far = tri.reshape(-1)[GRID_CAP * 64:]                         # (dense order is not brick order: a coarse look at both ends)
        assert (tri >= 0).any() and (tri < 0).any() and (far >= 0).any() and (far < 0).any() and len(np.unique(inst)) == 4


def test_world_dist_grid_deep_hierarchy_among_others(psm, ctx):
    """a hierarchy deeper than the 16 LDS entries of a lane's own stack, posed, among three others: the wave's one stack carries
    the tree over the instances and the deep hierarchy"""
    deep, _, _ = Q.deep_fixture()
    poses = _rigid(4, 49, shift=1.0, reflect=(0,))
    with _World(psm, ctx, [deep, _soup(50, 100, 0.8, 0.2)], [(1, poses[0]), (0, poses[1]), (1, poses[2]), (1, poses[3])]) as sc:
        dist, tri, inst = check_field(psm, sc, _world_grid(sc, (6, 6, 6)))
        assert len(np.unique(inst)) >= 3 and (inst == 1).any()
        # and a fine grid around the deep body's dense end, where its clusters shrink by halves
        tip = NQ.to_world(poses[1], np.zeros((1, 3)))[0]
        fine = (tuple(tip - 0.05), 0.0125, (8, 8, 8))
        _, _, finst = check_field(psm, sc, fine)
        assert (finst == 1).sum() > 100


@pytest.mark.parametrize("opt", [ROT_SCALE, SHEAR], ids=["rotate_scale", "shear"])
def test_world_dist_grid_build_matrix(psm, ctx, opt):
    """a hierarchy built under an optimisation matrix, as an instance at a rotated pose: the bound of the prune uses the full 3 x 3
    part (the orthogonal form for the rotate-scale, the largest-axis form for the shear)"""
    rng = np.random.RandomState(35)
    c = rng.uniform(-1, 1, (1500, 1, 3)) * [1.0, 0.3, 2.0]
    tris = (c + rng.uniform(-0.08, 0.08, (1500, 3, 3))).astype(F)
    poses = _rigid(2, 51, shift=0.5, reflect=())
    with _World(psm, ctx, [tris, _soup(52, 80, 0.5, 0.2)], [(0, poses[0]), (1, poses[1])], opts=[opt, None]) as sc:
        m = np.array(sc.ths[0].info().transform).reshape(4, 4)[:3, :3]
        assert np.abs(m - np.diag(np.diag(m))).max() > 0.01
        grid = _world_grid(sc, (9, 9, 9), 0.25)
        dist, tri, inst = check_field(psm, sc, grid)
        assert (inst == 0).any() and (inst == 1).any()
        _, ntri, _ = check_field(psm, sc, grid, rmax=0.15)
        assert (ntri >= 0).any() and (ntri < 0).any()


def test_world_dist_grid_after_moving_bodies(psm, ctx):
    poses = _rigid(4, 53, shift=1.0, reflect=(2,))
    with _World(psm, ctx, [IQ.icosphere(1, 0.6), _soup(54, 150, 0.6, 0.2)], [(k % 2, m) for k, m in enumerate(poses)]) as sc:
        grid = _world_grid(sc, (9, 9, 9), 0.3)
        before = check_field(psm, sc, grid)
        sc.world.setTransform(1, NQ.random_pose(np.random.RandomState(55), reflect=True, shift=1.0))
        after = check_field(psm, sc, grid)
        assert (before[0].view(U) != after[0].view(U)).any() and (before[2] != after[2]).any()
        rng = np.random.RandomState(59)
        sc.world.setTransforms(2, np.stack([NQ.random_pose(rng, shift=1.0), NQ.random_pose(rng, shift=1.0)]))
        again = check_field(psm, sc, grid, signed=True)
        assert (np.abs(again[0]).view(U) != after[0].view(U)).any()


def test_world_dist_grid_after_refit(psm, ctx, scenes):
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3).copy()
    poses = _rigid(2, 56, shift=0.5, reflect=(1,))
    with _World(psm, ctx, [tris], [(0, m) for m in poses]) as sc:
        th = sc.ths[0]
        grid = _world_grid(sc, (9, 9, 9))
        before, _, _ = check_field(psm, sc, grid)
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
        after, _, _ = check_field(psm, sc, grid)
        assert (before.view(U) != after.view(U)).any()


@pytest.mark.parametrize("samples", [1, 3, 5])
def test_world_dist_grid_signed(psm, ctx, samples):
    meshes, entries = signed_world()
    with _World(psm, ctx, meshes, entries) as sc:
        w = sc.world
        for grid, kinds in zip(SIGNED_GRIDS, SIGNED_KINDS[samples]):   # whole and partial bricks
            nx, ny, nz = grid[2]
            model = grid is SIGNED_GRIDS[1]                            # (455 voxels)
            dist, tri, inst = check_field(psm, sc, grid, signed=True, samples=samples, model=model)
            assert (tri >= 0).all() and np.signbit(dist).any() and not np.signbit(dist).all()
            near, ntri, ninst = check_field(psm, sc, grid, rmax=SIGNED_RMAX, signed=True, samples=samples, model=model)
            inside = w.inside(psm.voxel_centres(*grid), samples).reshape(nz, ny, nx)
            hit = ntri >= 0
            assert np.array_equal(np.signbit(near), hit & inside)       # (-0.0 too: the sign bit, not the value)
            deep = ~hit & inside                                      # inside, no triangle within rmax: +inf, the sign bit clear
            assert (near[deep].view(U) == INF_BITS).all()
            assert (int((hit & inside).sum()), int((hit & ~inside).sum()), int(deep.sum())) == kinds
            plain = w.distanceField(*grid, rmax=SIGNED_RMAX)
            _same(ntri, plain.tri, "tri is unchanged by the sign")
            _same(ninst, plain.inst, "inst is unchanged by the sign")
            _same(np.abs(near), plain.dist, "the sign changes the sign bit alone")


def test_world_dist_grid_signed_takes_more_than_one_slab(psm, ctx):
    """42 875 bricks: more than the 32 768 whose centres and records the scratch holds at a time; a band of three cells"""
    dims = (140, 140, 140)
    cell = 3.4 / 140
    grid = ((-1.5, -1.4, -2.5), cell, dims)
    assert (140 // 4) ** 3 > 32768
    meshes, entries = signed_world()
    with _World(psm, ctx, meshes, entries) as sc:
        dist, tri, inst = check_field(psm, sc, grid, rmax=3 * cell, signed=True, samples=1)
        hit = tri >= 0
        assert hit[-40:].any() and hit[:40].any() and (~hit).any() and set(np.unique(inst)) == {-1, 0, 1, 2}
        assert np.signbit(dist).any() and (dist[hit] > 0).any()
        last = dist.reshape(-1)[-1]                                    # the far corner: outside every band
        assert last.view(U) == INF_BITS


@pytest.mark.parametrize("name", PC.CASES)
def test_world_dist_grid_edge_poses(psm, ctx, name):
    """the worlds of tests/world_pose_cases.py -- far from the origin, stored far from their own origin, mixed scales, poses at
    the edge of what counts as rigid -- under the case's far grid: rmax inf, then rmax set to the median of the first field's
    finite distances, a float32 some voxel holds exactly, so that voxel sits on the limit; unsigned and signed"""
    c = PC.case(name)
    grid = PC.far_grid(c)
    with _World(psm, ctx, c.meshes, c.entries) as sc:
        for th, t in zip(sc.ths, sc.meshes):
            assert th.info().leaf_count == t.shape[0]                  # the case's own instance list is the world's
        insts = c.insts()
        dist, tri, inst = check_field(psm, sc, grid, model=True, insts=insts)
        finite = np.sort(dist[np.isfinite(dist)])
        rmax = float(finite[finite.size // 2])
        assert (dist == F(rmax)).any()
        near, ntri, _ = check_field(psm, sc, grid, rmax=rmax, model=True, insts=insts)
        assert (ntri >= 0).any() and (ntri < 0).any() and (near == F(rmax)).any()
        check_field(psm, sc, grid, signed=True, samples=3)
        check_field(psm, sc, grid, rmax=rmax, signed=True, samples=3)


def test_world_dist_grid_torch_side_stream_and_graph(psm, ctx, scenes):
    if torch is None:
        pytest.skip("torch is not installed")
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3)
    poses = _rigid(3, 57, shift=0.8, reflect=(1,))
    with _World(psm, ctx, [tris], [(0, m) for m in poses]) as sc:
        w = sc.world
        grid = _world_grid(sc, (21, 18, 23))
        rmax = 4 * max(grid[1])
        plain = w.distanceField(*grid, rmax=rmax)
        signed = w.distanceField(*grid, rmax=rmax, signed=True, samples=3)
        assert (plain.tri >= 0).any() and (plain.tri < 0).any()
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            tplain = w.distanceField(*grid, rmax=rmax, as_torch=True)
            tsigned = w.distanceField(*grid, rmax=rmax, signed=True, samples=3, as_torch=True)
            talone = w.distanceField(*grid, rmax=rmax, nearest=False, as_torch=True)
            agree = torch.equal(tplain.dist.abs(), tsigned.dist.abs())   # a torch op on the results, no host synchronisation before it
            bufs = [x.cpu() for x in (tplain.dist, tplain.tri, tplain.inst, tsigned.dist, tsigned.tri, tsigned.inst, talone.dist)]
        assert agree and tplain.dist.device == dev and tplain.dist.dtype == torch.float32 and tplain.tri.dtype == torch.int32
        assert tplain.inst.dtype == torch.int32 and tuple(tplain.inst.shape) == (23, 18, 21) and tplain.dims == (21, 18, 23)
        assert talone.tri is None and talone.inst is None
        for got, want, what in zip(bufs, (plain.dist, plain.tri, plain.inst, signed.dist, signed.tri, signed.inst, plain.dist),
                                   ("dist", "tri", "inst", "signed dist", "signed tri", "signed inst", "dist without the ids")):
            _same(got.numpy(), want, "torch " + what)
        # the unsigned call allocates nothing: captured after the warm calls above, replayed into pre-filled buffers; then a body
        # moves, the world is refreshed, and the same graph answers the moved world
        lib = psm.lib()
        g = psm._grid(*grid)
        dist = torch.zeros((23, 18, 21), dtype=torch.float32, device=dev)
        ids = torch.zeros((23, 18, 21), dtype=torch.int32, device=dev)
        owners = torch.zeros((23, 18, 21), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            def launch():
                assert lib.psm_grid_world_distance_dev(w._w, ctypes.byref(g), ctypes.c_float(rmax), ctypes.c_void_p(dist.data_ptr()),
                                                       ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(owners.data_ptr())) == 0
            psm._torch_ordered(ctx, dev, launch)     # side -> the context's stream -> side
        for step in range(2):
            dist.fill_(-7.0)
            ids.fill_(7)
            owners.fill_(9)
            graph.replay()
            torch.cuda.synchronize()
            _same(dist.cpu().numpy(), plain.dist, "replayed dist")
            _same(ids.cpu().numpy(), plain.tri, "replayed tri")
            _same(owners.cpu().numpy(), plain.inst, "replayed inst")
            if step == 0:
                continue
            w.setTransform(1, NQ.random_pose(np.random.RandomState(60), reflect=False, shift=0.8))
            w.refresh()
            ctx.sync()
            moved = w.distanceField(*grid, rmax=rmax)
            assert (moved.dist.view(U) != plain.dist.view(U)).any()
            graph.replay()
            torch.cuda.synchronize()
            _same(dist.cpu().numpy(), moved.dist, "replayed dist after the move")
            _same(owners.cpu().numpy(), moved.inst, "replayed inst after the move")
    torch.cuda.synchronize()


def _bad_grids(psm):
    bad = []
    for field, k, value in (("dims", 0, 0), ("dims", 2, (1 << 20) + 1), ("cell", 1, 0.0), ("cell", 0, -1.0), ("cell", 2, np.nan),
                            ("cell", 1, np.inf), ("origin", 0, np.inf), ("origin", 2, np.nan), ("cell", 1, 1e38)):
        g = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
        getattr(g, field)[k] = value                                   # (the last one: the last voxel's hi, -2 + 8e38, is not finite)
        bad.append(g)
    huge = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
    huge.dims[:] = [1 << 20, 1 << 20, 8]                               # 2^37 bricks
    huge.cell[:] = [1e-3, 1e-3, 1e-3]
    return bad + [huge]


def test_world_dist_grid_refusals_launch_nothing(psm, ctx):
    """invalid grids, NULL and misaligned outputs, a NaN or negative rmax, samples = 0, 2, 4, 6 and a stale world are refused on
    the host, in the header's order -- calls that break several rules say which one wins --: the outputs keep what they held;
    the same buffers then take a good call, which writes its extent and nothing past it"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    good = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
    hd, ht, hi = (ctx.buf_alloc(4 * 512 + 16) for _ in range(3))
    with _World(psm, ctx, [tri, _soup(58, 30, 0.8, 0.3)], [(0, NQ.IDENTITY), (1, NQ.IDENTITY)]) as sc:
        w = sc.world
        try:
            ctx.buf_upload(hd, np.full(516, 77.0, F))
            ctx.buf_upload(ht, np.full(516, 77, np.int32))
            ctx.buf_upload(hi, np.full(516, 77, np.int32))
            pd, pt, pi = ctx.buf_ptr(hd)[0], ctx.buf_ptr(ht)[0], ctx.buf_ptr(hi)[0]

            def by(grid):
                return ctypes.byref(grid) if grid is not None else None

            def plain(grid=good, rmax=np.inf, d=pd, t=pt, i=pi, world=w._w):
                return lib.psm_grid_world_distance_dev(world, by(grid), ctypes.c_float(rmax), ctypes.c_void_p(d), ctypes.c_void_p(t),
                                                       ctypes.c_void_p(i))

            def signed(grid=good, rmax=np.inf, samples=3, d=pd, t=pt, i=pi, world=w._w):
                return lib.psm_grid_world_signed_distance_dev(world, by(grid), ctypes.c_float(rmax), ctypes.c_uint32(samples),
                                                              ctypes.c_void_p(d), ctypes.c_void_p(t), ctypes.c_void_p(i))

            def said(text):
                return text in lib.psm_last_error(ctx._h)

            bad = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
            bad.cell[1] = 0.0
            for call, name in ((plain, b"psm_grid_world_distance_dev"), (signed, b"psm_grid_world_signed_distance_dev")):
                # each refusal wins over those after it
                assert call(world=None, grid=None, rmax=np.nan) == -1
                assert call(grid=None, rmax=np.nan, d=pd + 2) == -1 and said(name + b": NULL pointer")
                assert call(d=None, grid=bad) == -1 and said(name + b": NULL pointer")
                assert call(grid=bad, d=pd + 2, rmax=-1.0) == -1 and said(name + b": invalid grid: cell must be finite and > 0")
                assert call(d=pd + 2, rmax=-1.0) == -1 and said(name + b": dist, tri or inst not 4-byte aligned")
                assert call(t=pt + 1, rmax=np.nan) == -1 and said(name + b": dist, tri or inst not 4-byte aligned")
                assert call(i=pi + 2, rmax=np.nan) == -1 and said(name + b": dist, tri or inst not 4-byte aligned")
                for r in (np.nan, -1.0, -np.inf, -1e-30):
                    assert call(rmax=r) == -1 and said(name + b": rmax must be >= 0")
                for g in _bad_grids(psm):
                    assert call(grid=g) == -1 and said(b"invalid grid")
            assert signed(rmax=-1.0, samples=2) == -1 and said(b"rmax must be >= 0")
            for s in (0, 2, 4, 6):
                assert signed(samples=s) == -1 and said(b"psm_grid_world_signed_distance_dev: samples must be 1, 3 or 5")
            with pytest.raises(psm.PsmError):
                w.distanceField((-2, -2, -2), 0.5, (8, 8, 8), signed=True, samples=2)
            with pytest.raises(ValueError):
                w.distanceField((-2, -2, -2), 0.0, (8, 8, 8))
            sc.ths[1].markDirty()
            sc.ths[1].build()                                          # a member is rebuilt: the world is stale until it is set anew
            for call in (plain, signed):
                assert call() == -5 and said(b"set the instances again")                            # PSM_ERR_STATE
                assert call(rmax=np.nan) == -1 and said(b"rmax must be >= 0")                       # (the host checks come first)
            assert signed(samples=2) == -1 and said(b"samples must be 1, 3 or 5")
            ctx.sync()
            assert (ctx.buf_download(hd, F, 516) == 77.0).all() and (ctx.buf_download(ht, np.int32, 516) == 77).all()
            assert (ctx.buf_download(hi, np.int32, 516) == 77).all()
            w.setInstances([(sc.ths[0], NQ.IDENTITY), (sc.ths[1], NQ.IDENTITY)])
            # and the same buffers are fine: 512 entries each are written, nothing before or past them; -0 is 0
            want = w.distanceField((-2, -2, -2), 0.5, (8, 8, 8), rmax=0.6)
            assert plain(rmax=0.6, d=pd + 4, t=pt + 4, i=pi + 4) == 0
            ctx.sync()
            for h, dtype, ref in ((hd, F, want.dist), (ht, np.int32, want.tri), (hi, np.int32, want.inst)):
                raw = ctx.buf_download(h, dtype, 516)
                assert raw[0] == 77 and (raw[513:] == 77).all()
                _same(raw[1:513].reshape(8, 8, 8), ref, "the raw call")
            assert (want.tri >= 0).any() and (want.tri < 0).any() and set(np.unique(want.inst)) == {-1, 0, 1}
            assert signed(rmax=0.6, samples=3, d=pd, t=None, i=pi) == 0 and plain(rmax=-0.0, t=None, i=None) == 0
            ctx.sync()
            assert (ctx.buf_download(ht, np.int32, 516)[[0, 513, 514, 515]] == 77).all()           # a NULL tri: not written
        finally:
            for h in (hd, ht, hi):
                ctx.buf_free(h)


def test_world_dist_grid_header_layer(psm, ctx, tmp_path):
    """psm::InstanceWorld::distanceField / signedDistanceField (tests/cpp/world_dist_grid_host.cpp, a process of its own): the
    same fields as Python's, with and without the ids, and a refusal leaves the vectors empty"""
    exe = str(tmp_path / "world_dist_grid_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "world_dist_grid_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    meshes, entries = signed_world()
    tris = meshes[0]
    grid = ((-1.4, -1.1, -2.5), (0.29, 0.27, 0.34), (10, 9, 11))
    g = psm._grid(*grid)
    inp, out = str(tmp_path / "grid.in"), str(tmp_path / "grid.out")
    with open(inp, "wb") as f:
        f.write(struct.pack("<i", tris.shape[0]))
        f.write(tris.astype("<f4").tobytes())
        f.write(struct.pack("<i", len(SIGNED_POSES)))
        for m in SIGNED_POSES:
            m4 = np.eye(4, dtype=F)
            m4[:3] = m
            f.write(np.ascontiguousarray(m4.T).astype("<f4").tobytes())    # glm::mat4: column-major
        f.write(bytes(g))
        f.write(struct.pack("<fI", SIGNED_RMAX, 3))
    subprocess.check_call([exe, inp, out], timeout=120)
    raw = open(out, "rb").read()
    nv = struct.unpack_from("<Q", raw, 0)[0]
    assert nv == 10 * 9 * 11 and len(raw) == 8 + 9 * 4 * nv
    parts = [np.frombuffer(raw, dt, nv, 8 + 4 * nv * k).reshape(11, 9, 10)
             for k, dt in enumerate((F, np.int32, np.int32, F, F, np.int32, F, np.int32, np.int32))]
    with _World(psm, ctx, meshes, entries) as sc:
        plain = sc.world.distanceField(*grid, rmax=SIGNED_RMAX)
        signed = sc.world.distanceField(*grid, rmax=SIGNED_RMAX, signed=True, samples=3)
    for got, want, what in zip(parts, (plain.dist, plain.tri, plain.inst, plain.dist, plain.dist, plain.inst, signed.dist, signed.tri, signed.inst),
                               ("dist", "tri", "inst", "dist alone", "dist with inst", "inst alone", "signed dist", "signed tri", "signed inst")):
        _same(got, want, "the header layer's " + what)
    assert (plain.tri >= 0).any() and (plain.tri < 0).any() and np.signbit(signed.dist).any() and set(np.unique(plain.inst)) == {-1, 0, 1, 2}
