"""The voxel grids on the GPU (psm_grid_surface_dev / psm_grid_counts_dev / psm_grid_solid_dev, grid.hip;
TriangleHierarchy.voxelize / voxelCounts). The answer is defined as what the box queries answer for every voxel's
box, so the yardstick of every case is th.boxOverlaps / th.boxCount on psm.voxel_boxes(...) -- code that is merged and held to a
numpy model of its own --, and for grids of at most 1 000 voxels also tests/grid_query_model.py. Every comparison is exact, and in
every case voxelize(...).dense() == (voxelCounts(...) > 0)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

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
    bad = np.argwhere(a != b)
    assert bad.shape[0] == 0, "%s: %d differ, first at %s: %s against %s" % (what, bad.shape[0], bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


def check_grid(psm, th, tris, grid, model=None):
    """surface and counts of `grid` against the box queries on the voxels' boxes, against the model where the grid is small (or
    where `model` says), and against one another; returns (dense flags, counts)"""
    nx, ny, nz = grid[2]
    lo, hi = psm.voxel_boxes(*grid)
    flag = th.boxOverlaps(lo, hi).reshape(nz, ny, nx)
    count = th.boxCount(lo, hi).reshape(nz, ny, nx)
    vg = th.voxelize(*grid)
    got = th.voxelCounts(*grid)
    nb = ((nz + 3) // 4, (ny + 3) // 4, (nx + 3) // 4)
    assert vg.bricks.shape == nb and vg.bricks.dtype == np.uint64 and vg.dims == (nx, ny, nz)
    assert got.shape == (nz, ny, nx) and got.dtype == U and got.size == nx * ny * nz
    _same(got, count, "voxelCounts against boxCount")
    dense = vg.dense()
    _same(dense, flag, "voxelize against boxOverlaps")
    assert vg.occupied() == int(flag.sum())                      # the padding bits are 0 ...
    if nx * ny * nz <= 100000:
        _same(vg.bricks, GQ.pack_bricks(flag), "the brick words")   # ... and every bit is where the header says
    assert np.array_equal(dense, got > 0)
    if model if model is not None else nx * ny * nz <= 1000:
        leaves = _leaves(psm, th)
        _same(got, GQ.counts(tris, leaves, grid), "voxelCounts against the model")
        _same(vg.bricks, GQ.surface(tris, leaves, grid), "voxelize against the model")
    return dense, got


def test_grid_lattice_soup(psm, ctx):
    """all arithmetic exact: the 8^3 grid of [-1, 1]^3 over triangles on the 1/8 lattice, and the same grid moved by half a cell
    along one, two and three axes; triangles lie in shared voxel faces, and the closed rule counts them on both sides"""
    tris = GQ.lattice_soup(31, 500)
    th = _hier(psm, ctx, tris)
    try:
        for grid in GQ.LATTICE_GRIDS:
            dense, count = check_grid(psm, th, tris, grid)
            assert dense.sum() > 100 and (~dense).sum() > 5 and (count > 16).any()
        assert GQ.shared_face_counts(tris, _leaves(psm, th), GQ.LATTICE_GRIDS[0]) >= 1
        # and directly: a triangle in the face x = 0 is counted by the voxel on either side of it, and by no other
        face = np.array([[[0, 0.05, 0.05], [0, 0.2, 0.05], [0, 0.05, 0.2]]], F)
        th2 = _hier(psm, ctx, face)
        try:
            _, c2 = check_grid(psm, th2, face, GQ.LATTICE_GRIDS[0])
            assert c2.sum() == 2 and c2[4, 4, 3] == 1 and c2[4, 4, 4] == 1
        finally:
            th2.close()
    finally:
        th.close()


@pytest.mark.parametrize("dims", [(5, 7, 9), (1, 1, 1), (4, 4, 4), (3, 1, 130)], ids=lambda d: "x".join(map(str, d)))
def test_grid_partial_bricks(psm, ctx, dims):
    rng = np.random.RandomState(41)
    c = rng.uniform(-1, 1, (300, 1, 3))
    tris = (c + rng.uniform(-0.15, 0.15, (300, 3, 3))).astype(F)
    th = _hier(psm, ctx, tris)
    try:
        dense, count = check_grid(psm, th, tris, _bounds_grid(tris, dims))
        assert count.size == dims[0] * dims[1] * dims[2] and dense.any()
        if dims == (1, 1, 1):
            assert count[0, 0, 0] == th.info().leaf_count          # the one voxel holds the whole mesh
    finally:
        th.close()


def test_grid_more_bricks_than_workgroups(psm, ctx, scenes):
    """9 261 bricks: the grid-stride loop takes a second trip, and found / cnt start again for every brick"""
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3)
    dims = (84, 84, 84)
    assert (84 // 4) ** 3 > GRID_CAP
    th = _hier(psm, ctx, tris)
    try:
        dense, count = check_grid(psm, th, tris, _bounds_grid(tris, dims, 0.01))
        far = dense.reshape(-1)[GRID_CAP * 64:]                     # (dense order is not brick order: a coarse look at both ends)
        assert dense.any() and not dense.all() and far.any() and not far.all() and len(np.unique(count)) > 2
    finally:
        th.close()


def test_grid_deep_tree(psm, ctx):
    """a hierarchy deeper than the 16 LDS entries of a lane's own stack: the wave's one stack holds the depth"""
    tris, _, _ = Q.deep_fixture()
    th = _hier(psm, ctx, tris)
    try:
        dense, count = check_grid(psm, th, tris, _bounds_grid(tris, (6, 6, 6)))
        assert int(count.max()) > 64 and dense.any() and not dense.all()   # the voxel at the origin holds the small clusters
        one = _bounds_grid(tris, (1, 1, 1))
        assert th.voxelCounts(*one)[0, 0, 0] == th.info().leaf_count        # every leaf is reached: the deepest too
    finally:
        th.close()


def test_grid_tiny_hierarchies(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    degenerate = np.repeat(tri[:, :1], 3, axis=1)                    # three equal vertices: the build keeps no leaf
    grid = ((-0.5, -1.5, -1.5), 0.6, (5, 5, 5))
    for tris, leaves in ((np.concatenate([degenerate] * 4), 0), (np.concatenate([degenerate, tri, degenerate]), 1),
                         (np.concatenate([tri] * 7), 7)):            # ... and coincident triangles: one run of equal codes
        th = _hier(psm, ctx, tris)
        try:
            assert th.info().leaf_count == leaves
            dense, count = check_grid(psm, th, tris, grid)
            assert count.max() == leaves and (leaves == 0 or (dense.any() and not dense.all()))
            if leaves == 0:
                assert not th.voxelize(*grid).bricks.any() and not th.voxelize(*grid, solid=True).bricks.any()
        finally:
            th.close()


# the optimisation matrices of test_gpu_box_query.py: the fit transform's 3 x 3 part is full, the prune's row sums matter
ROT_SCALE = np.array([[np.cos(0.3), 0, np.sin(0.3), 0.5], [0, 1.3, 0, -1.0], [-np.sin(0.3), 0, np.cos(0.3), 2.0], [0, 0, 0, 1]])
SHEAR = np.array([[1, 0.6, 0, 0.2], [0, 1, -0.4, 0], [0.3, 0, 1, -1], [0, 0, 0, 1]])


@pytest.mark.parametrize("opt", [ROT_SCALE, SHEAR], ids=["rotate_scale", "shear"])
def test_grid_optimisation_matrix(psm, ctx, opt):
    rng = np.random.RandomState(35)
    c = rng.uniform(-1, 1, (1500, 1, 3)) * [1.0, 0.3, 2.0]
    tris = (c + rng.uniform(-0.08, 0.08, (1500, 3, 3))).astype(F)
    th = _hier(psm, ctx, tris, opt)
    try:
        m = np.array(th.info().transform).reshape(4, 4)[:3, :3]
        assert np.abs(m - np.diag(np.diag(m))).max() > 0.01
        dense, count = check_grid(psm, th, tris, _bounds_grid(tris, (9, 9, 9), 0.05))
        assert count.max() >= 10 and (~dense).sum() > 20
    finally:
        th.close()


def test_grid_after_refit(psm, ctx, scenes):
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3).copy()
    th = _hier(psm, ctx, tris)
    try:
        grid = _bounds_grid(tris, (9, 9, 9))
        before, _ = check_grid(psm, th, tris, grid)
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
        after, _ = check_grid(psm, th, moved, grid)
        assert (before != after).any()                                # the refitted boxes and the moved triangles are used
    finally:
        th.close()


SPHERE_GRID = ((-1.2, -1.2, -1.2), 0.2, (12, 12, 12))


def _solid_expected(psm, th, grid, samples):
    nx, ny, nz = grid[2]
    lo, hi = psm.voxel_boxes(*grid)
    return (th.boxOverlaps(lo, hi) | th.inside(psm.voxel_centres(*grid), samples)).reshape(nz, ny, nx)


@pytest.mark.parametrize("samples", [1, 3, 5])
def test_grid_solid_fills_a_closed_mesh(psm, ctx, samples):
    tris = IQ.icosphere(2)
    th = _hier(psm, ctx, tris)
    try:
        for grid in (SPHERE_GRID, ((-1.2, -1.1, -1.3), (0.5, 0.33, 0.29), (5, 7, 9))):   # whole bricks, and partial ones
            expect = _solid_expected(psm, th, grid, samples)
            vg = th.voxelize(*grid, solid=True, samples=samples)
            _same(vg.dense(), expect, "solid against surface | inside")
            _same(vg.bricks, GQ.pack_bricks(expect), "the solid brick words")          # the padding bits stay 0
        if samples == 3:
            surface = th.voxelize(*SPHERE_GRID).occupied()
            filled = th.voxelize(*SPHERE_GRID, solid=True, samples=3).occupied()
            assert surface < filled < 12 ** 3
            _same(th.voxelize(*SPHERE_GRID, solid=True).bricks, GQ.solid(tris, _leaves(psm, th), SPHERE_GRID, 3), "solid against the model")
    finally:
        th.close()


def test_grid_solid_takes_more_than_one_slab(psm, ctx):
    """68 921 bricks: more than the 65 536 whose centres and flags solid's scratch holds at a time"""
    tris = IQ.icosphere(2)
    dims = (164, 164, 164)
    grid = ((-1.2, -1.2, -1.2), 2.4 / 164, dims)
    th = _hier(psm, ctx, tris)
    try:
        vg = th.voxelize(*grid, solid=True, samples=1)
        expect = _solid_expected(psm, th, grid, 1)
        _same(vg.dense(), expect, "solid over two slabs")
        assert vg.occupied() == int(expect.sum()) and expect[-20:].any() and expect[82, 82, 82]
    finally:
        th.close()


def test_grid_torch_side_stream_and_graph(psm, ctx, scenes):
    if torch is None:
        pytest.skip("torch is not installed")
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3)
    grid = _bounds_grid(tris, (21, 18, 23), 0.02)
    th = _hier(psm, ctx, tris)
    try:
        vg, count = th.voxelize(*grid), th.voxelCounts(*grid)
        solid = th.voxelize(*grid, solid=True, samples=3)
        assert vg.dense().any() and not vg.dense().all()
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            tvg, tcount = th.voxelize(*grid, as_torch=True), th.voxelCounts(*grid, as_torch=True)
            tsolid = th.voxelize(*grid, solid=True, samples=3, as_torch=True)
            agree = torch.equal(tvg.dense(), tcount > 0)          # a torch op on the results, no host synchronisation before it
            bufs = [x.cpu() for x in (tvg.bricks, tcount, tsolid.bricks, tvg.dense())]   # (on the side stream: in order)
        assert agree and tvg.bricks.device == dev and tvg.bricks.dtype == torch.int64 and tcount.dtype == torch.int32
        assert tuple(tcount.shape) == (23, 18, 21) and tvg.dims == (21, 18, 23)
        _same(bufs[0].numpy().view(np.uint64), vg.bricks, "torch voxelize")
        _same(bufs[1].numpy().view(U), count, "torch voxelCounts")
        _same(bufs[2].numpy().view(np.uint64), solid.bricks, "torch voxelize solid")
        _same(bufs[3].numpy(), vg.dense(), "torch dense")
        assert tvg.occupied() == vg.occupied()
        # surface and counts allocate nothing: captured after the warm calls above into one linear chain, replayed twice
        lib = psm.lib()
        g = psm._grid(*grid)
        words = torch.zeros(tuple(vg.bricks.shape), dtype=torch.int64, device=dev)
        cells = torch.zeros(tuple(count.shape), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            def launch():
                assert lib.psm_grid_surface_dev(th._h, ctypes.byref(g), ctypes.c_void_p(words.data_ptr())) == 0
                assert lib.psm_grid_counts_dev(th._h, ctypes.byref(g), ctypes.c_void_p(cells.data_ptr())) == 0
            psm._torch_ordered(ctx, dev, launch)     # side -> the context's stream (both launches, in order) -> side
        for _ in range(2):
            words.fill_(0x55)
            cells.fill_(7)
            graph.replay()
            torch.cuda.synchronize()
            _same(words.cpu().numpy().view(np.uint64), vg.bricks, "replayed surface")
            _same(cells.cpu().numpy().view(U), count, "replayed counts")
    finally:
        th.close()
    torch.cuda.synchronize()


def test_grid_refusals_launch_nothing(psm, ctx):
    """a call before the build, invalid grids, misaligned and NULL outputs and samples = 2 are refused on the host: the outputs
    keep what they held"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(4)
    th.loadTriangles(tri.reshape(1, 9))
    good = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
    hw, hc = ctx.buf_alloc(8 * 8 + 16), ctx.buf_alloc(4 * 512 + 16)
    try:
        ctx.buf_upload(hw, np.full(10, 0x7777777777777777, np.uint64))
        ctx.buf_upload(hc, np.full(516, 77, U))
        pw, pc = ctx.buf_ptr(hw)[0], ctx.buf_ptr(hc)[0]

        def surface(grid=good, p=pw):
            return lib.psm_grid_surface_dev(th._h, ctypes.byref(grid) if grid is not None else None, ctypes.c_void_p(p))

        def counts(grid=good, p=pc):
            return lib.psm_grid_counts_dev(th._h, ctypes.byref(grid) if grid is not None else None, ctypes.c_void_p(p))

        def solid(samples=3, grid=good, p=pw):
            return lib.psm_grid_solid_dev(th._h, ctypes.byref(grid) if grid is not None else None, ctypes.c_uint32(samples), ctypes.c_void_p(p))

        for call in (surface, counts, solid):
            assert call() == -5 and b"grid query before build" in lib.psm_last_error(ctx._h)      # PSM_ERR_STATE
        th.build()
        bad = []
        for field, k, value in (("dims", 0, 0), ("dims", 2, (1 << 20) + 1), ("cell", 1, 0.0), ("cell", 0, -1.0), ("cell", 2, np.nan),
                                ("cell", 1, np.inf), ("origin", 0, np.inf), ("origin", 2, np.nan), ("cell", 1, 1e38)):
            g = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
            getattr(g, field)[k] = value                               # (the last one: the last voxel's hi, -2 + 8e38, is not finite)
            bad.append(g)
        huge = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
        huge.dims[:] = [1 << 20, 1 << 20, 8]                           # 2^37 bricks
        huge.cell[:] = [1e-3, 1e-3, 1e-3]
        for g in bad + [huge]:
            assert lib.psm_grid_brick_count(ctypes.byref(g)) == 0
            for call in (surface, counts, solid):
                assert call(grid=g) == -1 and b"invalid grid" in lib.psm_last_error(ctx._h)
        for call in (surface, counts, solid):
            assert call(grid=None) == -1 and call(p=None) == -1
        assert surface(p=pw + 4) == -1 and b"bricks not 8-byte aligned" in lib.psm_last_error(ctx._h)
        assert solid(p=pw + 4) == -1 and counts(p=pc + 2) == -1 and b"counts not 4-byte aligned" in lib.psm_last_error(ctx._h)
        for s in (0, 2, 4, 6):
            assert solid(samples=s) == -1 and b"samples must be 1, 3 or 5" in lib.psm_last_error(ctx._h)
        ctx.sync()
        assert (ctx.buf_download(hw, np.uint64, 10) == 0x7777777777777777).all() and (ctx.buf_download(hc, U, 516) == 77).all()
        with pytest.raises(psm.PsmError):
            th.voxelize((-2, -2, -2), 0.5, (8, 8, 8), solid=True, samples=2)
        with pytest.raises(ValueError):
            th.voxelCounts((-2, -2, -2), 0.0, (8, 8, 8))
        # and the same buffers are fine: 8 words and 512 counts are written, nothing past them
        assert surface() == 0 and counts(p=pc + 4) == 0
        ctx.sync()
        words, cells = ctx.buf_download(hw, np.uint64, 10), ctx.buf_download(hc, U, 516)
        assert (words[8:] == 0x7777777777777777).all() and cells[0] == 77 and (cells[513:] == 77).all()
        _same(words[:8].reshape(2, 2, 2), th.voxelize((-2, -2, -2), 0.5, (8, 8, 8)).bricks, "the raw call")
        assert words[:8].any() and (cells[1:513] <= 1).all() and cells[1:513].sum() > 4
    finally:
        ctx.buf_free(hw)
        ctx.buf_free(hc)
        th.close()


def test_grid_header_layer(psm, ctx, tmp_path):
    """psm::TriangleHierarchy::voxelize / voxelizeSolid / voxelCounts (tests/cpp/grid_query_host.cpp, a process of its own): the
    same bricks and counts as Python's"""
    exe = str(tmp_path / "grid_query_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "grid_query_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    tris = IQ.icosphere(2)
    grid = ((-1.2, -1.1, -1.3), (0.21, 0.2, 0.24), (11, 12, 10))
    g = psm._grid(*grid)
    inp, out = str(tmp_path / "grid.in"), str(tmp_path / "grid.out")
    with open(inp, "wb") as f:
        f.write(struct.pack("<i", tris.shape[0]))
        f.write(tris.astype("<f4").tobytes())
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
    th = _hier(psm, ctx, tris)
    try:
        _same(surface, th.voxelize(*grid).bricks, "the header layer's voxelize")
        _same(solid, th.voxelize(*grid, solid=True, samples=3).bricks, "the header layer's voxelizeSolid")
        _same(cells, th.voxelCounts(*grid), "the header layer's voxelCounts")
        assert surface.any() and (solid != surface).any()
    finally:
        th.close()
