"""The distance-field grids on the GPU (psm_grid_distance_dev / psm_grid_signed_distance_dev, grid_dist.hip;
TriangleHierarchy.distanceField). The answer is defined as what the point queries answer for every voxel's
centre, so the yardstick of every case is th.closestPoint / th.signedDistance on psm.voxel_centres(...) with the same rmax and
samples -- code that is merged and held to a numpy model of its own --, and for grids of at most 1 000 voxels also
tests/point_query_model.py over the downloaded leaves (tests/dist_grid_model.py). Every comparison is exact: dist is compared
through a uint32 view, so -0.0, +inf and NaN cannot hide."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import dist_grid_model as DG
import grid_query_model as GQ
import inside_query_model as IQ
import query_model as Q
from util import ROOT

try:   # (imported before the library loads its HIP runtime: see test_gpu_query.py)
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
INF_BITS = 0x7F800000
GRID_CAP = int(re.search(r"#define PSM_QUERY_GRID_CAP (\d+)",
                         open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "psm_query_dev.h")).read()).group(1))


def _hier(psm, ctx, tris, opt=None):
    tris = np.ascontiguousarray(tris, F).reshape(-1, 9)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(max(tris.shape[0], 1))
    th.loadTriangles(tris)
    th.build(opt)
    return th


def _leaves(psm, th):
    return th.download(psm.BVH_LEAF_TRI, np.int32, th.info().leaf_count)


def _bounds_grid(tris, dims, grow=0.0):
    """a grid of `dims` voxels over the triangles' bounds (grown by a fraction of the extent on every side)"""
    pts = np.asarray(tris, np.float64).reshape(-1, 3)
    lo, hi = pts.min(0), pts.max(0)
    lo, hi = lo - grow * (hi - lo), hi + grow * (hi - lo)
    return tuple(lo), tuple((hi - lo) / np.asarray(dims, np.float64)), tuple(dims)


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == F:
        a, b = a.view(U), b.view(U)
    bad = np.argwhere(a != b)
    assert bad.shape[0] == 0, "%s: %d differ, first at %s: %s against %s" % (what, bad.shape[0], bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


def check_field(psm, th, tris, grid, rmax=np.inf, signed=False, samples=3, model=None):
    """the field of `grid` against the point query over the voxels' centres, with and without the ids, and against the model
    where the grid is small (or where `model` says); returns (dist, tri)"""
    nx, ny, nz = grid[2]
    centres = psm.voxel_centres(*grid)
    ref = th.signedDistance(centres, rmax, samples) if signed else th.closestPoint(centres, rmax)
    got = th.distanceField(*grid, rmax=rmax, signed=signed, samples=samples)
    assert got.dist.shape == got.tri.shape == (nz, ny, nx) and got.dist.dtype == F and got.tri.dtype == np.int32
    assert got.dims == (nx, ny, nz) and got.dist.size == nx * ny * nz
    kind = "signedDistance" if signed else "closestPoint"
    _same(got.dist, ref.t.reshape(nz, ny, nx), "dist against %s" % kind)
    _same(got.tri, ref.tri.reshape(nz, ny, nx), "tri against %s" % kind)
    alone = th.distanceField(*grid, rmax=rmax, signed=signed, samples=samples, nearest=False)
    assert alone.tri is None
    _same(alone.dist, got.dist, "dist without the ids")
    miss = got.tri < 0
    assert (got.dist[miss].view(U) == INF_BITS).all() and np.isfinite(got.dist[~miss]).all()
    if model if model is not None else nx * ny * nz <= 1000:
        leaves = _leaves(psm, th)
        mdist, mtri = DG.signed_field(tris, leaves, grid, rmax, samples) if signed else DG.field(tris, leaves, grid, rmax)
        _same(got.dist, mdist, "dist against the model")
        _same(got.tri, mtri, "tri against the model")
    return got.dist, got.tri


@pytest.fixture(scope="module")
def soup():
    rng = np.random.RandomState(41)
    c = rng.uniform(-1, 1, (300, 1, 3))
    return (c + rng.uniform(-0.15, 0.15, (300, 3, 3))).astype(F)


@pytest.mark.parametrize("dims", [(5, 7, 9), (1, 1, 1), (4, 4, 4), (3, 1, 130)], ids=lambda d: "x".join(map(str, d)))
def test_dist_grid_partial_bricks(psm, ctx, soup, dims):
    th = _hier(psm, ctx, soup)
    try:
        grid = _bounds_grid(soup, dims)
        _, tri = check_field(psm, th, soup, grid)
        assert (tri >= 0).all()
        _, near = check_field(psm, th, soup, grid, rmax=0.25)
        if dims != (1, 1, 1):        # (the one voxel's centre is the middle of the soup: a hit)
            assert (near >= 0).any() and (near < 0).any()
    finally:
        th.close()


def test_dist_grid_lattice_ties_and_zeros(psm, ctx):
    """all arithmetic exact: triangles on the 1/8 lattice under the 8^3 grid of [-1, 1]^3 and the same grid moved by half a cell:
    voxels with several triangles at the bit-equal smallest d2 (the lowest id wins), voxels at distance exactly 0, misses"""
    tris = GQ.lattice_soup(31, 500)
    th = _hier(psm, ctx, tris)
    try:
        leaves = _leaves(psm, th)
        for grid in GQ.LATTICE_GRIDS:
            ties, zeros, misses = DG.ties_zeros_misses(tris, leaves, grid, 0.25)
            assert ties >= 1 and zeros >= 1 and misses >= 1
            dist, tri = check_field(psm, th, tris, grid)
            assert int((dist == 0).sum()) == zeros and (tri >= 0).all()
            _, near = check_field(psm, th, tris, grid, rmax=0.25)
            assert int((near < 0).sum()) == misses
    finally:
        th.close()


def test_dist_grid_tiny_hierarchies(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    degenerate = np.repeat(tri[:, :1], 3, axis=1)                    # three equal vertices: the build keeps no leaf
    grid = ((-0.5, -1.5, -1.5), 0.6, (5, 5, 5))
    for tris, leaves in ((np.concatenate([degenerate] * 4), 0), (np.concatenate([degenerate, tri, degenerate]), 1),
                         (np.concatenate([tri] * 7), 7)):            # ... and coincident triangles: one run of equal codes
        th = _hier(psm, ctx, tris)
        try:
            assert th.info().leaf_count == leaves
            for rmax in (np.inf, 0.7):
                dist, ids = check_field(psm, th, tris, grid, rmax=rmax)
                sdist, sids = check_field(psm, th, tris, grid, rmax=rmax, signed=True)
                if leaves == 0:
                    assert (dist.view(U) == INF_BITS).all() and (ids == -1).all()
                    assert (sdist.view(U) == INF_BITS).all() and (sids == -1).all()
                else:
                    first = 1 if leaves == 1 else 0                  # the lone leaf; the lowest of the seven coincident ids
                    assert (ids[ids >= 0] == first).all() and (ids >= 0).any() and ((ids < 0).any() == (rmax == 0.7))
        finally:
            th.close()


def test_dist_grid_more_bricks_than_workgroups(psm, ctx, scenes):
    """9 261 bricks: the grid-stride loop takes a second trip, and best / btri / found start again for every brick"""
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3)
    dims = (84, 84, 84)
    assert (84 // 4) ** 3 > GRID_CAP
    th = _hier(psm, ctx, tris)
    try:
        grid = _bounds_grid(tris, dims, 0.01)
        cell = max(grid[1])
        dist, tri = check_field(psm, th, tris, grid, rmax=3 * cell)
        far = tri.reshape(-1)[GRID_CAP * 64:]                        # (dense order is not brick order: a coarse look at both ends)
        assert (tri >= 0).any() and (tri < 0).any() and (far >= 0).any() and (far < 0).any() and len(np.unique(tri)) > 8
    finally:
        th.close()


def test_dist_grid_deep_tree(psm, ctx):
    """a hierarchy deeper than the 16 LDS entries of a lane's own stack: the wave's one stack holds the depth"""
    tris, _, _ = Q.deep_fixture()
    th = _hier(psm, ctx, tris)
    try:
        grid = _bounds_grid(tris, (6, 6, 6))
        _, tri = check_field(psm, th, tris, grid)
        assert len(np.unique(tri)) > 20 and (tri >= 0).all()
        _, near = check_field(psm, th, tris, grid, rmax=0.05)
        assert (near >= 0).any() and (near < 0).any()
    finally:
        th.close()


# the optimisation matrices of test_gpu_grid_query.py: the fit transform's 3 x 3 part is full; a rotation and a scale keep the
# rows orthogonal (the sum form of the bound), a shear does not (the max form)
ROT_SCALE = np.array([[np.cos(0.3), 0, np.sin(0.3), 0.5], [0, 1.3, 0, -1.0], [-np.sin(0.3), 0, np.cos(0.3), 2.0], [0, 0, 0, 1]])
SHEAR = np.array([[1, 0.6, 0, 0.2], [0, 1, -0.4, 0], [0.3, 0, 1, -1], [0, 0, 0, 1]])


@pytest.mark.parametrize("opt", [ROT_SCALE, SHEAR], ids=["rotate_scale", "shear"])
def test_dist_grid_optimisation_matrix(psm, ctx, opt):
    rng = np.random.RandomState(35)
    c = rng.uniform(-1, 1, (1500, 1, 3)) * [1.0, 0.3, 2.0]
    tris = (c + rng.uniform(-0.08, 0.08, (1500, 3, 3))).astype(F)
    th = _hier(psm, ctx, tris, opt)
    try:
        m = np.array(th.info().transform).reshape(4, 4)[:3, :3]
        assert np.abs(m - np.diag(np.diag(m))).max() > 0.01
        grid = _bounds_grid(tris, (9, 9, 9), 0.05)
        _, tri = check_field(psm, th, tris, grid)
        assert len(np.unique(tri)) > 100
        _, near = check_field(psm, th, tris, grid, rmax=0.1)
        assert (near >= 0).any() and (near < 0).any()
    finally:
        th.close()


def test_dist_grid_after_refit(psm, ctx, scenes):
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3).copy()
    th = _hier(psm, ctx, tris)
    try:
        grid = _bounds_grid(tris, (9, 9, 9))
        before, _ = check_field(psm, th, tris, grid)
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
        after, _ = check_field(psm, th, moved, grid)
        assert (before.view(U) != after.view(U)).any()                # the refitted boxes and the moved triangles are used
    finally:
        th.close()


SPHERE_GRID = ((-1.2, -1.2, -1.2), 0.2, (12, 12, 12))
PARTIAL_GRID = ((-1.2, -1.1, -1.3), (0.5, 0.33, 0.29), (5, 7, 9))


@pytest.mark.parametrize("samples", [1, 3, 5])
def test_dist_grid_signed(psm, ctx, samples):
    tris = IQ.icosphere(2)
    th = _hier(psm, ctx, tris)
    try:
        for grid in (SPHERE_GRID, PARTIAL_GRID):                     # whole bricks, and partial ones
            nx, ny, nz = grid[2]
            dist, tri = check_field(psm, th, tris, grid, signed=True, samples=samples, model=samples == 3)
            assert (tri >= 0).all() and np.signbit(dist).any() and not np.signbit(dist).all()
            near, ntri = check_field(psm, th, tris, grid, rmax=0.3, signed=True, samples=samples, model=samples == 3)
            inside = th.inside(psm.voxel_centres(*grid), samples).reshape(nz, ny, nx)
            hit = ntri >= 0
            assert np.array_equal(np.signbit(near), hit & inside)
            deep = ~hit & inside                                      # inside, no triangle within rmax: +inf, the sign bit clear
            assert (near[hit & inside] < 0).any() and (near[hit & ~inside] > 0).any() and deep.any()
            assert (near[deep].view(U) == INF_BITS).all()
            _same(ntri, th.distanceField(*grid, rmax=0.3).tri, "tri is unchanged by the sign")
            if samples == 3:
                kinds = (int((hit & inside).sum()), int((hit & ~inside).sum()), int(deep.sum()))
                assert kinds == ((320, 608, 160) if grid is SPHERE_GRID else (49, 108, 32))
    finally:
        th.close()


def test_dist_grid_signed_takes_more_than_one_slab(psm, ctx):
    """68 921 bricks: more than the 32 768 whose centres and records the scratch holds at a time"""
    tris = IQ.icosphere(2)
    dims = (164, 164, 164)
    cell = 2.4 / 164
    grid = ((-1.2, -1.2, -1.2), cell, dims)
    th = _hier(psm, ctx, tris)
    try:
        dist, tri = check_field(psm, th, tris, grid, rmax=3 * cell, signed=True, samples=1)
        hit = tri >= 0
        assert hit[-20:].any() and hit[:20].any() and not hit[82, 82, 82] and dist[82, 82, 82].view(U) == INF_BITS
        assert np.signbit(dist).any() and (dist[hit] > 0).any()
    finally:
        th.close()


def test_dist_grid_torch_side_stream_and_graph(psm, ctx, scenes):
    if torch is None:
        pytest.skip("torch is not installed")
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3)
    grid = _bounds_grid(tris, (21, 18, 23), 0.02)
    rmax = 4 * max(grid[1])
    th = _hier(psm, ctx, tris)
    try:
        plain = th.distanceField(*grid, rmax=rmax)
        signed = th.distanceField(*grid, rmax=rmax, signed=True, samples=3)
        assert (plain.tri >= 0).any() and (plain.tri < 0).any()
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            tplain = th.distanceField(*grid, rmax=rmax, as_torch=True)
            tsigned = th.distanceField(*grid, rmax=rmax, signed=True, samples=3, as_torch=True)
            talone = th.distanceField(*grid, rmax=rmax, nearest=False, as_torch=True)
            agree = torch.equal(tplain.dist.abs(), tsigned.dist.abs())   # a torch op on the results, no host synchronisation before it
            bufs = [x.cpu() for x in (tplain.dist, tplain.tri, tsigned.dist, tsigned.tri, talone.dist)]   # (on the side stream: in order)
        assert agree and tplain.dist.device == dev and tplain.dist.dtype == torch.float32 and tplain.tri.dtype == torch.int32
        assert tuple(tplain.dist.shape) == tuple(tplain.tri.shape) == (23, 18, 21) and tplain.dims == (21, 18, 23) and talone.tri is None
        _same(bufs[0].numpy(), plain.dist, "torch dist")
        _same(bufs[1].numpy(), plain.tri, "torch tri")
        _same(bufs[2].numpy(), signed.dist, "torch signed dist")
        _same(bufs[3].numpy(), signed.tri, "torch signed tri")
        _same(bufs[4].numpy(), plain.dist, "torch dist without the ids")
        # the unsigned call allocates nothing: captured after the warm calls above, replayed twice into pre-filled buffers
        lib = psm.lib()
        g = psm._grid(*grid)
        dist = torch.zeros((23, 18, 21), dtype=torch.float32, device=dev)
        ids = torch.zeros((23, 18, 21), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            def launch():
                assert lib.psm_grid_distance_dev(th._h, ctypes.byref(g), ctypes.c_float(rmax), ctypes.c_void_p(dist.data_ptr()),
                                                 ctypes.c_void_p(ids.data_ptr())) == 0
            psm._torch_ordered(ctx, dev, launch)     # side -> the context's stream -> side
        for _ in range(2):
            dist.fill_(-7.0)
            ids.fill_(7)
            graph.replay()
            torch.cuda.synchronize()
            _same(dist.cpu().numpy(), plain.dist, "replayed dist")
            _same(ids.cpu().numpy(), plain.tri, "replayed tri")
    finally:
        th.close()
    torch.cuda.synchronize()


def test_dist_grid_refusals_launch_nothing(psm, ctx):
    """a call before the build, invalid grids, misaligned and NULL outputs, a NaN or negative rmax and samples = 2 are refused on
    the host, in the header's order: the outputs keep what they held"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(4)
    th.loadTriangles(tri.reshape(1, 9))
    good = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
    hd, ht = ctx.buf_alloc(4 * 512 + 16), ctx.buf_alloc(4 * 512 + 16)
    try:
        ctx.buf_upload(hd, np.full(516, 77.0, F))
        ctx.buf_upload(ht, np.full(516, 77, np.int32))
        pd, pt = ctx.buf_ptr(hd)[0], ctx.buf_ptr(ht)[0]

        def plain(grid=good, rmax=np.inf, d=pd, t=pt):
            return lib.psm_grid_distance_dev(th._h, ctypes.byref(grid) if grid is not None else None, ctypes.c_float(rmax),
                                             ctypes.c_void_p(d), ctypes.c_void_p(t))

        def signed(grid=good, rmax=np.inf, samples=3, d=pd, t=pt):
            return lib.psm_grid_signed_distance_dev(th._h, ctypes.byref(grid) if grid is not None else None, ctypes.c_float(rmax),
                                                    ctypes.c_uint32(samples), ctypes.c_void_p(d), ctypes.c_void_p(t))

        def said(text):
            return text in lib.psm_last_error(ctx._h)

        bad = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
        bad.cell[1] = 0.0
        for call, name in ((plain, b"psm_grid_distance_dev"), (signed, b"psm_grid_signed_distance_dev")):
            # before the build, each refusal wins over those after it
            assert call(grid=None, rmax=np.nan, d=pd + 2) == -1 and said(name + b": NULL pointer")
            assert call(d=None, grid=bad) == -1 and said(name + b": NULL pointer")
            assert call(grid=bad, d=pd + 2, rmax=-1.0) == -1 and said(name + b": invalid grid: cell must be finite and > 0")
            assert call(d=pd + 2, rmax=-1.0) == -1 and said(name + b": dist or tri not 4-byte aligned")
            assert call(t=pt + 1, rmax=np.nan) == -1 and said(name + b": dist or tri not 4-byte aligned")
            assert call(rmax=np.nan) == -1 and said(name + b": rmax must be >= 0")
            assert call(rmax=-1.0) == -1 and said(name + b": rmax must be >= 0")
            assert call(rmax=-np.inf) == -1 and said(name + b": rmax must be >= 0")
            assert call() == -5 and said(b"grid query before build")                                # PSM_ERR_STATE
            assert call(rmax=-0.0) == -5                                                            # (-0 is 0: accepted)
        assert signed(rmax=-1.0, samples=2) == -1 and said(b"rmax must be >= 0")
        for s in (0, 2, 4, 6):
            assert signed(samples=s) == -1 and said(b"psm_grid_signed_distance_dev: samples must be 1, 3 or 5")
        th.build()
        for g in _bad_grids(psm):
            for call in (plain, signed):
                assert call(grid=g) == -1 and said(b"invalid grid")
        for call in (plain, signed):
            assert call(grid=None) == -1 and call(d=None) == -1 and call(d=pd + 2) == -1 and call(t=pt + 2) == -1
            assert call(rmax=np.nan) == -1 and call(rmax=-1e-30) == -1 and said(b"rmax must be >= 0")
        assert signed(samples=2) == -1 and said(b"samples must be 1, 3 or 5")
        ctx.sync()
        assert (ctx.buf_download(hd, F, 516) == 77.0).all() and (ctx.buf_download(ht, np.int32, 516) == 77).all()
        with pytest.raises(psm.PsmError):
            th.distanceField((-2, -2, -2), 0.5, (8, 8, 8), signed=True, samples=2)
        with pytest.raises(ValueError):
            th.distanceField((-2, -2, -2), 0.0, (8, 8, 8))
        with pytest.raises(ValueError):
            th.distanceField((-2, -2, -2), 0.5, (8, 8, 8), rmax=np.nan)
        want = th.distanceField((-2, -2, -2), 0.5, (8, 8, 8))
        swant = th.distanceField((-2, -2, -2), 0.5, (8, 8, 8), signed=True)
        # and the same buffers are fine: 512 entries of each output are written, nothing past them
        assert plain(d=pd + 4, t=pt + 4) == 0
        ctx.sync()
        dist, ids = ctx.buf_download(hd, F, 516), ctx.buf_download(ht, np.int32, 516)
        assert dist[0] == 77.0 and (dist[513:] == 77.0).all() and ids[0] == 77 and (ids[513:] == 77).all()
        _same(dist[1:513].reshape(8, 8, 8), want.dist, "the raw call's dist")
        _same(ids[1:513].reshape(8, 8, 8), want.tri, "the raw call's tri")
        assert (ids[1:513] == 0).all() and np.isfinite(dist[1:513]).all()
        # d_tri = NULL writes d_dist only; rmax = -0.0 is 0: no centre lies on the triangle, all misses
        ctx.buf_upload(hd, np.full(516, 77.0, F))
        ctx.buf_upload(ht, np.full(516, 77, np.int32))
        assert signed(d=pd + 4, t=None) == 0
        ctx.sync()
        dist = ctx.buf_download(hd, F, 516)
        assert dist[0] == 77.0 and (dist[513:] == 77.0).all() and (ctx.buf_download(ht, np.int32, 516) == 77).all()
        _same(dist[1:513].reshape(8, 8, 8), swant.dist, "the raw signed call's dist")
        assert plain(rmax=-0.0) == 0
        ctx.sync()
        assert (ctx.buf_download(hd, F, 512).view(U) == INF_BITS).all() and (ctx.buf_download(ht, np.int32, 512) == -1).all()
    finally:
        ctx.buf_free(hd)
        ctx.buf_free(ht)
        th.close()


def _bad_grids(psm):
    bad = []
    for field, k, value in (("dims", 0, 0), ("dims", 2, (1 << 20) + 1), ("cell", 1, 0.0), ("cell", 0, -1.0), ("cell", 2, np.nan),
                            ("cell", 1, np.inf), ("origin", 0, np.inf), ("origin", 2, np.nan), ("cell", 1, 1e38)):
        g = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
        getattr(g, field)[k] = value                               # (the last one: the last voxel's hi, -2 + 8e38, is not finite)
        bad.append(g)
    huge = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
    huge.dims[:] = [1 << 20, 1 << 20, 8]                           # 2^37 bricks
    huge.cell[:] = [1e-3, 1e-3, 1e-3]
    return bad + [huge]


def test_dist_grid_header_layer(psm, ctx, tmp_path):
    """psm::TriangleHierarchy::distanceField / signedDistanceField (tests/cpp/dist_grid_host.cpp, a process of its own): the same
    bytes as Python's"""
    exe = str(tmp_path / "dist_grid_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "dist_grid_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    tris = IQ.icosphere(2)
    grid = ((-1.2, -1.1, -1.3), (0.21, 0.2, 0.24), (11, 12, 10))
    g = psm._grid(*grid)
    rmax = 0.3
    inp, out = str(tmp_path / "dist.in"), str(tmp_path / "dist.out")
    with open(inp, "wb") as f:
        f.write(struct.pack("<i", tris.shape[0]))
        f.write(tris.astype("<f4").tobytes())
        f.write(bytes(g))
        f.write(struct.pack("<fI", rmax, 3))
    subprocess.check_call([exe, inp, out], timeout=120)
    raw = open(out, "rb").read()
    nv = struct.unpack_from("<Q", raw, 0)[0]
    assert nv == 11 * 12 * 10 and len(raw) == 8 + 5 * 4 * nv
    part = [np.frombuffer(raw, F if k in (0, 2, 3) else np.int32, nv, 8 + 4 * nv * k).reshape(10, 12, 11) for k in range(5)]
    th = _hier(psm, ctx, tris)
    try:
        r32 = float(F(rmax))
        plain, signed = th.distanceField(*grid, rmax=r32), th.distanceField(*grid, rmax=r32, signed=True, samples=3)
        _same(part[0], plain.dist, "the header layer's distanceField")
        _same(part[1], plain.tri, "the header layer's ids")
        _same(part[2], plain.dist, "the header layer's distanceField without ids")
        _same(part[3], signed.dist, "the header layer's signedDistanceField")
        _same(part[4], signed.tri, "the header layer's signed ids")
        assert (plain.tri >= 0).any() and (plain.tri < 0).any() and np.signbit(signed.dist).any()
    finally:
        th.close()
