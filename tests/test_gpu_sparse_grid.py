"""The sparse grids on the GPU (psm_grid_sparse_*_dev, grid_sparse.hip; TriangleHierarchy.sparseVoxelize /
sparseDistanceField). The answer is defined by the dense calls, so the yardstick of every case is the merged
th.voxelize / th.distanceField of the same grid, rmax and samples: `ids` must be the ascending bricks where the dense answer is
non-empty, and slot i the dense answer of brick ids[i] (tests/sparse_grid_model.py states "dense -> sparse"). Every comparison
is exact: dist is compared through a uint32 view. Each listing is run with and without the coarse pass (PSM_SPARSE_COARSE)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import grid_query_model as GQ
import inside_query_model as IQ
import sparse_grid_model as SG
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
SOUP_GRID = ((-3.0, -3.0, -3.0), 0.2, (30, 30, 30))
PLANE_GRID = ((0.0, 0.0, 0.0), 1.0, (4, 4, 12))


def _hier(psm, ctx, tris, opt=None):
    tris = np.ascontiguousarray(tris, F).reshape(-1, 9)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(max(tris.shape[0], 1))
    th.loadTriangles(tris)
    th.build(opt)
    return th


def _bounds_grid(tris, dims, grow=0.0):
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


class _coarse:
    """the listing's coarse pass forced on / off (the knob is read at each call)"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.before = os.environ.get("PSM_SPARSE_COARSE")
        os.environ["PSM_SPARSE_COARSE"] = "1" if self.on else "0"

    def __exit__(self, *exc):
        if self.before is None:
            del os.environ["PSM_SPARSE_COARSE"]
        else:
            os.environ["PSM_SPARSE_COARSE"] = self.before


def check_distance(psm, th, grid, rmax, signed=False, samples=3):
    """sparseDistanceField against distanceField, with and without the coarse pass and the ids; returns the sparse grid"""
    dense = th.distanceField(*grid, rmax=rmax, signed=signed, samples=samples)
    ids, dist, tri = SG.distance_list(dense.dist, dense.tri)
    for on in (True, False):
        with _coarse(on):
            got = th.sparseDistanceField(*grid, rmax, signed=signed, samples=samples)
        what = "%s field, coarse %s" % ("signed" if signed else "plain", on)
        assert got.ids.dtype == U and got.dist.dtype == F and got.tri.dtype == np.int32 and got.dims == tuple(grid[2])
        _same(got.ids, ids, what + ": ids")
        _same(got.dist, dist, what + ": dist")
        _same(got.tri, tri, what + ": tri")
    alone = th.sparseDistanceField(*grid, rmax, signed=signed, samples=samples, nearest=False)
    assert alone.tri is None
    _same(alone.ids, ids, "ids without the triangles")
    _same(alone.dist, dist, "dist without the triangles")
    back = got.dense()
    _same(back.dist, dense.dist, "dense() dist")
    _same(back.tri, dense.tri, "dense() tri")
    assert len(got) == ids.size and (got.tri >= 0).any(axis=(1, 2, 3)).all()
    return got


def check_surface(psm, th, grid):
    dense = th.voxelize(*grid)
    ids, words = SG.surface_list(dense.bricks)
    for on in (True, False):
        with _coarse(on):
            got = th.sparseVoxelize(*grid)
        assert got.ids.dtype == U and got.words.dtype == np.uint64 and got.dims == tuple(grid[2])
        _same(got.ids, ids, "surface ids, coarse %s" % on)
        _same(got.words, words, "surface words, coarse %s" % on)
    _same(got.dense().bricks, dense.bricks, "dense() bricks")
    assert (got.words != 0).all()
    return got


def raw_list(psm, ctx, th, grid, rmax, capacity, sentinel=0xABCDEF01):
    """one raw listing call (rmax None: the surface's) into `capacity` pre-filled slots: (the slots, *d_count)"""
    lib = psm.lib()
    g = psm._grid(*grid)
    h_ids, h_count = ctx.buf_alloc(4 * capacity + 16), ctx.buf_alloc(16)
    try:
        ctx.buf_upload(h_ids, np.full(capacity + 4, sentinel, U))
        ctx.buf_upload(h_count, np.full(4, sentinel, U))
        p_ids = ctypes.c_void_p(ctx.buf_ptr(h_ids)[0]) if capacity else None
        p_count = ctypes.c_void_p(ctx.buf_ptr(h_count)[0])
        if rmax is None:
            rc = lib.psm_grid_sparse_surface_bricks_dev(th._h, ctypes.byref(g), ctypes.c_uint32(capacity), p_ids, p_count)
        else:
            rc = lib.psm_grid_sparse_distance_bricks_dev(th._h, ctypes.byref(g), ctypes.c_float(rmax), ctypes.c_uint32(capacity), p_ids, p_count)
        assert rc == 0, lib.psm_last_error(ctx._h)
        ctx.sync()
        count = ctx.buf_download(h_count, U, 4)
        assert (count[1:] == sentinel).all()
        return ctx.buf_download(h_ids, U, capacity + 4), int(count[0])
    finally:
        ctx.buf_free(h_ids)
        ctx.buf_free(h_count)


@pytest.fixture(scope="module")
def soup():
    rng = np.random.RandomState(41)
    c = rng.uniform(-1, 1, (300, 1, 3))
    return (c + rng.uniform(-0.15, 0.15, (300, 3, 3))).astype(F)


def test_sparse_soup_in_a_larger_grid(psm, ctx, soup):
    """8 bricks an axis, the last partial; brick 0 holds centres <= -2.3 and the soup lies >= -1.15: the outer bricks are empty
    by arithmetic"""
    th = _hier(psm, ctx, soup)
    try:
        for signed in (False, True):
            got = check_distance(psm, th, SOUP_GRID, 0.25, signed=signed, samples=3)
            n = len(got)
            assert 0 < n < 512 and 0 not in got.ids and 511 not in got.ids
            if signed:
                assert np.signbit(got.dist).any()
        _, count = raw_list(psm, ctx, th, SOUP_GRID, 0.25, 0)
        assert count == n
        surf = check_surface(psm, th, SOUP_GRID)
        assert 0 < len(surf) <= n                                    # (the surface lies within the band)
        _, count = raw_list(psm, ctx, th, SOUP_GRID, None, 0)
        assert count == len(surf)
        xyz = got.coords()
        assert xyz.shape == (n, 3) and np.array_equal((xyz[:, 2] * 8 + xyz[:, 1]) * 8 + xyz[:, 0], got.ids) and xyz.min() >= 1 and xyz.max() <= 6
    finally:
        th.close()


@pytest.mark.parametrize("dims", [(5, 7, 9), (1, 1, 1), (4, 4, 4), (3, 1, 130)], ids=lambda d: "x".join(map(str, d)))
def test_sparse_partial_bricks(psm, ctx, soup, dims):
    th = _hier(psm, ctx, soup)
    try:
        grid = _bounds_grid(soup, dims)
        bricks = int(np.prod(SG.brick_shape(dims)))
        every = check_distance(psm, th, grid, np.inf)               # rmax = inf: every brick listed, dense() is the dense field
        assert every.ids.tolist() == list(range(bricks))
        outside = 64 * bricks - dims[0] * dims[1] * dims[2]
        assert int((every.tri < 0).sum()) == outside and int((every.dist.view(U) == INF_BITS).sum()) == outside
        check_distance(psm, th, grid, 0.25)
        check_distance(psm, th, grid, 0.25, signed=True)
        zero = check_distance(psm, th, grid, 0.0)                   # rmax = 0: a centre on a triangle, or nothing
        assert len(zero) == 0 and zero.dist.shape == (0, 4, 4, 4)
        check_surface(psm, th, grid)
    finally:
        th.close()


def test_sparse_closed_at_rmax(psm, ctx):
    """tests/test_sparse_grid_cpu.py establishes the dense answer's shape by the models: rmax = 4.5 reaches the lowest layer of
    brick 1 exactly, the float below it does not; a triangle in the face two bricks share is in both"""
    plane = np.array([[[-8, -8, 0], [24, -8, 0], [-8, 24, 0]]], F)
    th = _hier(psm, ctx, plane)
    try:
        got = check_distance(psm, th, PLANE_GRID, 4.5)
        assert got.ids.tolist() == [0, 1]
        lanes = got.dist[1].reshape(64)
        assert (lanes[:16] == 4.5).all() and (lanes[16:].view(U) == INF_BITS).all() and np.isfinite(got.dist[0]).all()
        below = check_distance(psm, th, PLANE_GRID, float(np.nextafter(F(4.5), F(0))))
        assert below.ids.tolist() == [0]
        assert check_surface(psm, th, PLANE_GRID).ids.tolist() == [0]
    finally:
        th.close()
    th = _hier(psm, ctx, plane + F([0, 0, 4]))
    try:
        surf = check_surface(psm, th, PLANE_GRID)
        assert surf.ids.tolist() == [0, 1] and surf.words.tolist() == [0xFFFF << 48, 0xFFFF]
    finally:
        th.close()


def test_sparse_lattice_ties_and_zeros(psm, ctx):
    """all arithmetic exact: triangles on the 1/8 lattice, centres at distance exactly 0 and exactly rmax"""
    tris = GQ.lattice_soup(31, 500)
    th = _hier(psm, ctx, tris)
    try:
        for grid in GQ.LATTICE_GRIDS:
            got = check_distance(psm, th, grid, 0.25)
            assert (got.dist == 0).any() and (got.tri < 0).any()
            check_distance(psm, th, grid, 0.125)
            check_distance(psm, th, grid, 0.0)
            check_surface(psm, th, grid)
    finally:
        th.close()


def test_sparse_more_candidates_than_workgroups(psm, ctx, scenes):
    """13 824 bricks, all candidates with rmax = inf: the waves stride over the list under the cap; and a narrow band over the
    same grid, where the coarse pass leaves a list whose count only the device knows"""
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3)
    dims = (96, 96, 96)
    assert (96 // 4) ** 3 > GRID_CAP
    th = _hier(psm, ctx, tris)
    try:
        grid = _bounds_grid(tris, dims, 0.01)
        every = check_distance(psm, th, grid, np.inf)
        assert len(every) == 13824
        band = check_distance(psm, th, grid, 2 * max(grid[1]))
        assert GRID_CAP // 8 < len(band) < 13824
        surf = check_surface(psm, th, grid)
        assert 0 < len(surf) <= len(band)
    finally:
        th.close()


def test_sparse_scan_boundaries(psm, ctx, soup):
    """brick counts that are no multiple of the scan's 1 024 entries nor of 64: 17 x 9 x 11 = 1 683 bricks, and 1 025"""
    th = _hier(psm, ctx, soup)
    try:
        for dims in ((66, 34, 43), (4 * 1025, 2, 3)):
            bricks = int(np.prod(SG.brick_shape(dims)))
            assert bricks % 1024 and bricks % 64 and bricks > 1024
            grid = _bounds_grid(soup, dims, 0.3)
            check_distance(psm, th, grid, np.inf)
            band = check_distance(psm, th, grid, 0.1)
            assert 0 < len(band) < bricks
            check_surface(psm, th, grid)
    finally:
        th.close()


def test_sparse_capacity(psm, ctx, soup):
    """count-only with NULL ids; capacity < count gives the prefix and the slots past it keep what they held; capacity > count
    leaves the slots past the count alone"""
    th = _hier(psm, ctx, soup)
    try:
        for rmax in (0.25, None, np.inf):
            for on in (True, False):
                with _coarse(on):
                    slots, count = raw_list(psm, ctx, th, SOUP_GRID, rmax, 0)
                    assert 4 < count <= 512 and (slots == 0xABCDEF01).all()
                    full, again = raw_list(psm, ctx, th, SOUP_GRID, rmax, count + 3)
                    assert again == count and (full[count:] == 0xABCDEF01).all() and (np.diff(full[:count].astype(np.int64)) > 0).all()
                    part, again = raw_list(psm, ctx, th, SOUP_GRID, rmax, count - 4)
                    assert again == count and (part[count - 4:] == 0xABCDEF01).all()
                    _same(part[:count - 4], full[:count - 4], "the prefix")
                    one, again = raw_list(psm, ctx, th, SOUP_GRID, rmax, 1)
                    assert again == count and one[0] == full[0] and (one[1:] == 0xABCDEF01).all()
    finally:
        th.close()


def test_sparse_caller_lists(psm, ctx, soup):
    """reversed, with duplicates, with ids at and above the brick count (empty slots), and n = 0"""
    th = _hier(psm, ctx, soup)
    try:
        grid = SOUP_GRID
        dense = th.distanceField(*grid, rmax=0.25)
        sdense = th.distanceField(*grid, rmax=0.25, signed=True, samples=3)
        words = th.voxelize(*grid).bricks.reshape(-1)
        listed = th.sparseDistanceField(*grid, 0.25).ids
        ids = np.concatenate([listed[::-1], listed[:5], listed[:5], [512, 513, 1 << 31, 0xFFFFFFFF, 0, 511]]).astype(U)
        d_all, t_all = SG.bricked_fast(dense.dist, F(np.inf)), SG.bricked_fast(dense.tri, np.int32(-1))
        got = th.sparseDistanceField(*grid, 0.25, bricks=ids)
        _same(got.ids, ids, "the caller's ids")
        _same(got.dist, SG.slots(ids, d_all, F(np.inf)), "the caller's list: dist")
        _same(got.tri, SG.slots(ids, t_all, -1), "the caller's list: tri")
        assert (got.tri[-6:] == -1).all() and (got.dist[-6:].view(U) == INF_BITS).all()
        sgot = th.sparseDistanceField(*grid, 0.25, signed=True, samples=3, bricks=ids, nearest=False)
        assert sgot.tri is None
        _same(sgot.dist, SG.slots(ids, SG.bricked_fast(sdense.dist, F(np.inf)), F(np.inf)), "the caller's list: signed dist")
        wgot = th.sparseVoxelize(*grid, bricks=ids)
        _same(wgot.words, SG.slots(ids, words, 0), "the caller's list: words")
        assert (wgot.words[-6:] == 0).all() and (wgot.words != 0).any()
        _same(got.dense().dist, dense.dist, "dense() of a list with duplicates and strangers")
        for empty in (np.zeros(0, U), []):
            none = th.sparseDistanceField(*grid, 0.25, bricks=empty)
            assert none.ids.shape == (0,) and none.dist.shape == none.tri.shape == (0, 4, 4, 4)
            assert th.sparseVoxelize(*grid, bricks=empty).words.shape == (0,)
            assert th.sparseDistanceField(*grid, 0.25, signed=True, bricks=empty).dist.shape == (0, 4, 4, 4)
        # the raw calls with n = 0 launch nothing and need no list
        lib, g = psm.lib(), psm._grid(*grid)
        h = ctx.buf_alloc(1024)
        try:
            p = ctypes.c_void_p(ctx.buf_ptr(h)[0])
            assert lib.psm_grid_sparse_surface_dev(th._h, ctypes.byref(g), None, ctypes.c_uint32(0), p) == 0
            assert lib.psm_grid_sparse_distance_dev(th._h, ctypes.byref(g), ctypes.c_float(0.25), None, ctypes.c_uint32(0), p, None) == 0
            assert lib.psm_grid_sparse_signed_distance_dev(th._h, ctypes.byref(g), ctypes.c_float(0.25), ctypes.c_uint32(3), None, ctypes.c_uint32(0), p, None) == 0
        finally:
            ctx.buf_free(h)
    finally:
        th.close()


def test_sparse_signed_list_of_more_than_one_slab(psm, ctx):
    """a caller's list of 40 000 slots: more than the 32 768 bricks whose centres and records the scratch holds at a time"""
    tris = IQ.icosphere(2)
    grid = ((-1.2, -1.2, -1.2), 0.1, (24, 24, 24))
    th = _hier(psm, ctx, tris)
    try:
        dense = th.distanceField(*grid, rmax=0.3, signed=True, samples=1)
        ids = (np.arange(40000, dtype=np.int64) * 7 % 216).astype(U)
        got = th.sparseDistanceField(*grid, 0.3, signed=True, samples=1, bricks=ids)
        _same(got.dist, SG.slots(ids, SG.bricked_fast(dense.dist, F(np.inf)), F(np.inf)), "signed dist over two slabs")
        _same(got.tri, SG.slots(ids, SG.bricked_fast(dense.tri, np.int32(-1)), -1), "tri over two slabs")
        assert np.signbit(got.dist[32768:]).any() and (got.tri[32768:] >= 0).any()
    finally:
        th.close()


def test_sparse_tiny_hierarchies_and_refit(psm, ctx, scenes):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    degenerate = np.repeat(tri[:, :1], 3, axis=1)                    # three equal vertices: the build keeps no leaf
    grid = ((-0.5, -1.5, -1.5), 0.6, (5, 5, 5))
    for tris, leaves in ((np.concatenate([degenerate] * 4), 0), (np.concatenate([degenerate, tri, degenerate]), 1)):
        th = _hier(psm, ctx, tris)
        try:
            assert th.info().leaf_count == leaves
            for rmax in (np.inf, 0.7):
                got = check_distance(psm, th, grid, rmax)
                check_distance(psm, th, grid, rmax, signed=True)
                assert len(got) == (0 if leaves == 0 else (8 if rmax == np.inf else len(got))) and (leaves == 0 or len(got) > 0)
            assert (len(check_surface(psm, th, grid)) > 0) == (leaves == 1)
            assert raw_list(psm, ctx, th, grid, np.inf, 0)[1] == (0 if leaves == 0 else 8)
        finally:
            th.close()
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3).copy()
    th = _hier(psm, ctx, tris)
    try:
        grid = _bounds_grid(tris, (21, 21, 21), 0.05)
        rmax = 1.5 * max(grid[1])
        before = check_distance(psm, th, grid, rmax)
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
        after = check_distance(psm, th, grid, rmax)                   # the refitted boxes and the moved triangles are used
        check_surface(psm, th, grid)
        assert 0 < len(after) < 216 and (len(after) != len(before) or (before.dist.view(U) != after.dist.view(U)).any())
    finally:
        th.close()


ROT_SCALE = np.array([[np.cos(0.3), 0, np.sin(0.3), 0.5], [0, 1.3, 0, -1.0], [-np.sin(0.3), 0, np.cos(0.3), 2.0], [0, 0, 0, 1]])
SHEAR = np.array([[1, 0.6, 0, 0.2], [0, 1, -0.4, 0], [0.3, 0, 1, -1], [0, 0, 0, 1]])


@pytest.mark.parametrize("opt", [ROT_SCALE, SHEAR], ids=["rotate_scale", "shear"])
def test_sparse_optimisation_matrix(psm, ctx, opt):
    """a full 3 x 3 part in the build's transform: the coarse pass's interval and bound under the sum form and the max form"""
    rng = np.random.RandomState(35)
    c = rng.uniform(-1, 1, (1500, 1, 3)) * [1.0, 0.3, 2.0]
    tris = (c + rng.uniform(-0.08, 0.08, (1500, 3, 3))).astype(F)
    th = _hier(psm, ctx, tris, opt)
    try:
        grid = _bounds_grid(tris, (30, 30, 30), 0.6)
        bricks = 512
        for rmax in (0.0, 0.05, 0.3):
            assert len(check_distance(psm, th, grid, rmax)) < bricks
        assert 0 < len(check_surface(psm, th, grid)) < bricks
    finally:
        th.close()


def test_sparse_refusals_launch_nothing(psm, ctx):
    """before the build PSM_ERR_STATE, after the dense calls' refusals in their order; then the NULL list and the outputs
    untouched"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(4)
    th.loadTriangles(tri.reshape(1, 9))
    good = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
    bad = psm._grid((-2, -2, -2), 0.5, (8, 8, 8))
    bad.cell[1] = 0.0
    huge = psm._grid((0, 0, 0), 1e-3, (4096, 4096, 4096))            # 2^30 bricks: a valid grid, above the sparse cap
    h_out, h_ids = ctx.buf_alloc(4 * 1024 + 16), ctx.buf_alloc(64)
    try:
        ctx.buf_upload(h_out, np.full(1028, 77.0, F))
        ctx.buf_upload(h_ids, np.arange(16, dtype=U))
        po, pi = ctx.buf_ptr(h_out)[0], ctx.buf_ptr(h_ids)[0]

        def ptr(p):
            return ctypes.c_void_p(p) if p is not None else None

        def lists(dist):
            def call(grid=good, rmax=1.0, capacity=8, ids=po, count=po + 512):
                g = ctypes.byref(grid) if grid is not None else None
                if dist:
                    return lib.psm_grid_sparse_distance_bricks_dev(th._h, g, ctypes.c_float(rmax), ctypes.c_uint32(capacity), ptr(ids), ptr(count))
                return lib.psm_grid_sparse_surface_bricks_dev(th._h, g, ctypes.c_uint32(capacity), ptr(ids), ptr(count))
            return call

        def fills(kind):
            def call(grid=good, rmax=1.0, samples=3, ids=pi, n=2, out=po, tri=None):
                g = ctypes.byref(grid) if grid is not None else None
                if kind == "surface":
                    return lib.psm_grid_sparse_surface_dev(th._h, g, ptr(ids), ctypes.c_uint32(n), ptr(out))
                if kind == "distance":
                    return lib.psm_grid_sparse_distance_dev(th._h, g, ctypes.c_float(rmax), ptr(ids), ctypes.c_uint32(n), ptr(out), ptr(tri))
                return lib.psm_grid_sparse_signed_distance_dev(th._h, g, ctypes.c_float(rmax), ctypes.c_uint32(samples), ptr(ids), ctypes.c_uint32(n), ptr(out), ptr(tri))
            return call

        def said(text):
            return text in lib.psm_last_error(ctx._h)

        calls = [(lists(False), b"psm_grid_sparse_surface_bricks_dev", "count", False), (lists(True), b"psm_grid_sparse_distance_bricks_dev", "count", True),
                 (fills("surface"), b"psm_grid_sparse_surface_dev", "out", False), (fills("distance"), b"psm_grid_sparse_distance_dev", "out", True),
                 (fills("signed"), b"psm_grid_sparse_signed_distance_dev", "out", True)]
        for built in (False, True):
            for call, name, out, has_rmax in calls:
                assert call(grid=None, **{out: po + 2}) == -1 and said(name + b": NULL pointer")
                assert call(grid=bad, **{out: None}) == -1 and said(name + b": NULL pointer")
                assert call(grid=bad, **{out: po + 2}) == -1 and said(name + b": invalid grid: cell must be finite and > 0")
                assert call(**{out: po + 2}) == -1 and said(b"-byte aligned")
                assert call(ids=pi + 1) == -1 and said(b"-byte aligned")
                if has_rmax:
                    for rmax in (np.nan, -1.0, -np.inf):
                        assert call(rmax=rmax, ids=None) == -1 and said(name + b": rmax must be >= 0")
                if not built:
                    assert call(ids=None) == -5 and said(b"grid query before build")            # PSM_ERR_STATE: before the NULL list
                    assert call(grid=huge) == -5
                else:
                    assert call(ids=None) == -1 and said(name + b": NULL pointer")
                    assert call(grid=huge) == -4 and said(name + b": more than 2^27 bricks")       # PSM_ERR_CAPACITY
            if not built:
                assert fills("signed")(samples=2) == -1 and said(b"psm_grid_sparse_signed_distance_dev: samples must be 1, 3 or 5")
                th.build()
        assert fills("signed")(samples=4) == -1 and said(b"samples must be 1, 3 or 5")
        ctx.sync()
        assert (ctx.buf_download(h_out, F, 1028) == 77.0).all()
        with pytest.raises(psm.PsmError):
            th.sparseDistanceField((-2, -2, -2), 0.5, (8, 8, 8), 1.0, signed=True, samples=2)
        with pytest.raises(ValueError):
            th.sparseVoxelize((-2, -2, -2), 0.0, (8, 8, 8))
        with pytest.raises(ValueError):
            th.sparseDistanceField((-2, -2, -2), 0.5, (8, 8, 8), np.nan)
        with pytest.raises(ValueError):
            th.sparseVoxelize((-2, -2, -2), 0.5, (8, 8, 8), bricks=np.array([-1]))
        # and the same buffers are fine: 2 x 64 entries are written, nothing past them
        assert fills("distance")(out=po + 4, rmax=np.inf) == 0
        ctx.sync()
        dist = ctx.buf_download(h_out, F, 1028)
        assert dist[0] == 77.0 and (dist[129:] == 77.0).all() and np.isfinite(dist[1:129]).all()
    finally:
        ctx.buf_free(h_out)
        ctx.buf_free(h_ids)
        th.close()


def test_sparse_torch_side_stream_and_graph(psm, ctx, scenes):
    if torch is None:
        pytest.skip("torch is not installed")
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3)
    grid = _bounds_grid(tris, (41, 38, 43), 0.02)
    rmax = 1.5 * max(grid[1])
    th = _hier(psm, ctx, tris)
    try:
        plain = th.sparseDistanceField(*grid, rmax)
        signed = th.sparseDistanceField(*grid, rmax, signed=True, samples=3)
        surf = th.sparseVoxelize(*grid)
        n = len(plain)
        assert 0 < n < 11 * 10 * 11
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            tplain = th.sparseDistanceField(*grid, rmax, as_torch=True)
            tsigned = th.sparseDistanceField(*grid, rmax, signed=True, samples=3, as_torch=True)
            tsurf = th.sparseVoxelize(*grid, as_torch=True)
            tlist = th.sparseDistanceField(*grid, rmax, bricks=tplain.ids.flip(0), nearest=False, as_torch=True)
            agree = torch.equal(tplain.dist.abs(), tsigned.dist.abs()) and torch.equal(tlist.dist.flip(0), tplain.dist)   # torch ops on the results, no host synchronisation before them
            tdense = tplain.dense()
            bufs = [x.cpu() for x in (tplain.ids, tplain.dist, tplain.tri, tsigned.dist, tsurf.ids, tsurf.words, tdense.dist, tdense.tri, tplain.coords())]
        assert agree and tplain.dist.device == dev and tplain.dist.dtype == torch.float32 and tplain.tri.dtype == torch.int32 and tlist.tri is None
        assert tuple(tplain.dist.shape) == (n, 4, 4, 4) and tplain.ids.dtype == torch.int32 and tsurf.words.dtype == torch.int64
        _same(bufs[0].numpy().view(U), plain.ids, "torch ids")
        _same(bufs[1].numpy(), plain.dist, "torch dist")
        _same(bufs[2].numpy(), plain.tri, "torch tri")
        _same(bufs[3].numpy(), signed.dist, "torch signed dist")
        _same(bufs[4].numpy().view(U), surf.ids, "torch surface ids")
        _same(bufs[5].numpy().view(np.uint64), surf.words, "torch words")
        dense = th.distanceField(*grid, rmax=rmax)
        _same(bufs[6].numpy(), dense.dist, "torch dense() dist")
        _same(bufs[7].numpy(), dense.tri, "torch dense() tri")
        _same(bufs[8].numpy(), plain.coords(), "torch coords")
        # a numpy list with torch outputs
        mixed = th.sparseVoxelize(*grid, bricks=surf.ids, as_torch=True)
        _same(mixed.words.cpu().numpy().view(np.uint64), surf.words, "a numpy list, torch words")
        # the listing and the unsigned fill make no host synchronisation and, after the warm calls above, allocate nothing:
        # captured together, replayed twice into pre-filled buffers
        lib = psm.lib()
        g = psm._grid(*grid)
        ids = torch.zeros(n + 2, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        dist = torch.zeros((n, 64), dtype=torch.float32, device=dev)
        tri = torch.zeros((n, 64), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            def launch():
                assert lib.psm_grid_sparse_distance_bricks_dev(th._h, ctypes.byref(g), ctypes.c_float(rmax), ctypes.c_uint32(n + 2),
                                                               ctypes.c_void_p(ids.data_ptr()), ctypes.c_void_p(count.data_ptr())) == 0
                assert lib.psm_grid_sparse_distance_dev(th._h, ctypes.byref(g), ctypes.c_float(rmax), ctypes.c_void_p(ids.data_ptr()), ctypes.c_uint32(n),
                                                        ctypes.c_void_p(dist.data_ptr()), ctypes.c_void_p(tri.data_ptr())) == 0
            psm._torch_ordered(ctx, dev, launch)     # side -> the context's stream -> side
        for _ in range(2):
            ids.fill_(-7)
            count.fill_(-7)
            dist.fill_(-7.0)
            tri.fill_(7)
            graph.replay()
            torch.cuda.synchronize()
            assert int(count.cpu()[0]) == n and (ids.cpu().numpy()[n:] == -7).all()
            _same(ids.cpu().numpy()[:n].view(U), plain.ids, "replayed ids")
            _same(dist.cpu().numpy().reshape(n, 4, 4, 4), plain.dist, "replayed dist")
            _same(tri.cpu().numpy().reshape(n, 4, 4, 4), plain.tri, "replayed tri")
    finally:
        th.close()
    torch.cuda.synchronize()


def test_sparse_header_layer(psm, ctx, tmp_path):
    """psm::TriangleHierarchy::sparseVoxelize / sparseDistanceField / sparseSignedDistanceField (tests/cpp/sparse_grid_host.cpp, a
    process of its own): the same bytes as Python's"""
    exe = str(tmp_path / "sparse_grid_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "sparse_grid_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    tris = IQ.icosphere(2)
    grid = ((-2.2, -2.1, -2.3), (0.21, 0.2, 0.24), (21, 22, 19))
    g = psm._grid(*grid)
    rmax = 0.3
    inp, out = str(tmp_path / "sparse.in"), str(tmp_path / "sparse.out")
    with open(inp, "wb") as f:
        f.write(struct.pack("<i", tris.shape[0]))
        f.write(tris.astype("<f4").tobytes())
        f.write(bytes(g))
        f.write(struct.pack("<fI", rmax, 3))
    subprocess.check_call([exe, inp, out], timeout=120)
    raw = open(out, "rb").read()
    at = 0

    def take(dtype, count, shape=None):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a.reshape(shape) if shape else a

    th = _hier(psm, ctx, tris)
    try:
        r32 = float(F(rmax))
        surf, plain = th.sparseVoxelize(*grid), th.sparseDistanceField(*grid, r32)
        signed = th.sparseDistanceField(*grid, r32, signed=True, samples=3)
        n = int(take(np.uint64, 1)[0])
        _same(take(U, n), surf.ids, "the header layer's surface ids")
        _same(take(np.uint64, n), surf.words, "the header layer's words")
        n = int(take(np.uint64, 1)[0])
        _same(take(U, n), plain.ids, "the header layer's ids")
        _same(take(F, 64 * n, (n, 4, 4, 4)), plain.dist, "the header layer's sparseDistanceField")
        _same(take(np.int32, 64 * n, (n, 4, 4, 4)), plain.tri, "the header layer's triangles")
        n = int(take(np.uint64, 1)[0])
        _same(take(U, n), plain.ids, "the header layer's ids, no triangles asked")
        _same(take(F, 64 * n, (n, 4, 4, 4)), plain.dist, "the header layer's sparseDistanceField without ids")
        n = int(take(np.uint64, 1)[0])
        _same(take(U, n), signed.ids, "the header layer's signed ids")
        _same(take(F, 64 * n, (n, 4, 4, 4)), signed.dist, "the header layer's sparseSignedDistanceField")
        _same(take(np.int32, 64 * n, (n, 4, 4, 4)), signed.tri, "the header layer's signed triangles")
        assert at == len(raw) and 0 < len(surf) <= len(plain) < 6 * 6 * 5 and np.signbit(signed.dist).any()
    finally:
        th.close()
