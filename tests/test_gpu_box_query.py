"""The box queries on the GPU (psm_bvh_box_overlaps_dev / psm_bvh_box_count_dev / psm_bvh_box_triangles_dev, box.hip;
TriangleHierarchy.boxOverlaps / boxCount / boxTriangles). The yardstick is tests/box_query_model.py: box_tri in
numpy float32 by brute force over the hierarchy's leaves. Every comparison is exact on every box, and in every case the three
queries are also held against one another: overlaps == (count > 0), triangles.count == min(k, count), rows are prefixes."""
import ctypes
import os
import re

import numpy as np
import pytest

import box_query_model as BQ
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
KS = (1, 2, 3, 8, 16)


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
    assert a.shape == b.shape, what
    bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, "%s: %d differ, first %d: %s against %s" % (what, bad.size, bad[0], a[bad[0]], b[bad[0]])


def check_boxes(psm, th, tris, lo, hi, ks=KS):
    """the three queries against the model (computed once at the largest k: its rows are prefixes, test_box_query_cpu) and
    against one another; returns the model's flag, full count and rows at the largest k"""
    lo, hi = np.ascontiguousarray(lo, F).reshape(-1, 3), np.ascontiguousarray(hi, F).reshape(-1, 3)
    n = lo.shape[0]
    flag, count, rows, _ = BQ.query(tris, _leaves(psm, th), lo, hi, max(ks))
    got_flag, got_count = th.boxOverlaps(lo, hi), th.boxCount(lo, hi)
    assert got_flag.shape == (n,) and got_flag.dtype == np.bool_ and got_count.shape == (n,) and got_count.dtype == U
    _same(got_flag, flag, "boxOverlaps")
    _same(got_count, count, "boxCount")
    assert np.array_equal(got_flag, got_count > 0)
    widest = None
    for k in sorted(ks, reverse=True):
        got = th.boxTriangles(lo, hi, k)
        assert got.tri.shape == (n, k) and got.tri.dtype == np.int32 and got.count.shape == (n,) and got.count.dtype == U
        _same(got.tri, rows[:, :k], "boxTriangles k = %d" % k)
        _same(got.count, np.minimum(got_count, U(k)), "boxTriangles count against boxCount, k = %d" % k)
        assert np.array_equal(got.tri >= 0, np.arange(k)[None] < got.count[:, None])
        if widest is None:
            widest = got.tri
        _same(got.tri, widest[:, :k], "boxTriangles k = %d is a prefix of k = %d" % (k, max(ks)))
    return flag, count, rows


def lattice_soup(seed, count):
    """triangles with vertices on the 1/8 lattice of [-1, 1]^3, each vertex within a step of one lattice point"""
    rng = np.random.RandomState(seed)
    a = rng.randint(-8, 9, (count, 1, 3))
    a[count // 2:] = rng.randint(0, 5, (count - count // 2, 1, 3))   # half of them crowd one octant: cells with more than 16
    return (np.clip(a + rng.randint(-1, 2, (count, 3, 3)), -8, 8) / 8.0).astype(F)


def test_box_lattice_soup(psm, ctx):
    """all arithmetic exact: the cells of an 8^3 grid of [-1, 1]^3, and the same cells shifted by half a cell along one, two and
    three axes, so that they meet the lattice triangles at faces, edges and corners"""
    tris = lattice_soup(31, 500)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3)
    cells = (g / 4.0 - 1.0).astype(F)
    los = [cells] + [(cells + F(0.125) * F(s)).astype(F) for s in ([1, 0, 0], [0, 1, 1], [1, 1, 1])]
    lo = np.concatenate(los)
    hi = (lo + F(0.25)).astype(F)
    th = _hier(psm, ctx, tris)
    try:
        flag, count, _ = check_boxes(psm, th, tris, lo, hi)
        assert flag.sum() > 1000 and (~flag).sum() > 20 and (count > 16).any()
        # two cells sharing a face both count a triangle lying in that face
        face = np.array([[[0, 0, 0], [0, 0.25, 0], [0, 0, 0.25]]], F)
        th2 = _hier(psm, ctx, face)
        try:
            f2, c2, r2 = check_boxes(psm, th2, face, F([[-0.25, 0, 0], [0, 0, 0], [0.25, 0, 0]]), F([[0, 0.25, 0.25], [0.25, 0.25, 0.25], [0.5, 0.25, 0.25]]))
            assert list(c2) == [1, 1, 0] and list(r2[:, 0]) == [0, 0, -1]
        finally:
            th2.close()
    finally:
        th.close()


def test_box_random_soup(psm, ctx):
    rng = np.random.RandomState(32)
    c = rng.uniform(-1, 1, (2000, 1, 3))
    tris = (c + rng.uniform(-0.1, 0.1, (2000, 3, 3))).astype(F)
    n = 4096
    centre = rng.uniform(-1.1, 1.1, (n, 3))
    half = 10.0 ** rng.uniform(-3.5, -0.5, (n, 1)) * rng.uniform(0.3, 1.0, (n, 3))      # sizes over three decades
    lo, hi = (centre - half).astype(F), (centre + half).astype(F)
    lo[0, 0], hi[1, 1], lo[2, 2], hi[3, 0] = np.nan, np.nan, np.inf, np.inf
    lo[4, 1], hi[5, 2] = -np.inf, -np.inf
    lo[6, 0], hi[6, 0] = 0.5, 0.25                                                      # lo > hi on one axis
    lo[7], hi[7] = -np.inf, np.inf
    pts = tris.reshape(-1, 3)
    lo[8:40] = hi[8:40] = tris[rng.choice(2000, 32), 0]                                  # point boxes on a v0: L = H = 0, they count
    lo[40:56] = hi[40:56] = pts[rng.choice(pts.shape[0], 16)]                            # ... on any vertex (off v0 rounding may miss)
    w = rng.uniform(0, 1, (16, 3, 1))
    w /= w.sum(axis=1, keepdims=True)
    lo[56:72] = hi[56:72] = (tris[rng.choice(2000, 16)] * w).sum(axis=1).astype(F)      # ... and near interiors
    lo[72], hi[72] = pts.min(0) - F(1), pts.max(0) + F(1)                                # one box around everything
    th = _hier(psm, ctx, tris)
    try:
        leaves = np.sort(_leaves(psm, th))
        flag, count, rows = check_boxes(psm, th, tris, lo, hi)
        assert (count[:8] == 0).all() and (count[8:40] >= 1).all()
        assert count[72] == leaves.size and list(rows[72]) == list(leaves[:16])
        assert (count[73:] == 0).sum() > 100 and ((count[73:] > 0) & (count[73:] < 16)).sum() > 100 and (count[73:] > 16).sum() > 20
    finally:
        th.close()


def test_box_tiny_hierarchies(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    rng = np.random.RandomState(4)
    centre = rng.uniform(-0.5, 2.0, (200, 3))
    half = rng.uniform(0.0, 0.8, (200, 3))
    lo, hi = (centre - half).astype(F), (centre + half).astype(F)
    lo[0], hi[0] = -4, 4
    degenerate = np.repeat(tri[:, :1], 3, axis=1)                    # three equal vertices: the build keeps no leaf
    for tris, leaves in ((np.concatenate([degenerate] * 4), 0), (np.concatenate([degenerate, tri, degenerate]), 1),
                         (np.concatenate([tri, degenerate, tri + F([0.5, 0, 0])]), 2),
                         (np.concatenate([tri, tri + F([0.25, 0, 0]), degenerate, tri + F([0.5, 0, 0])]), 3)):
        th = _hier(psm, ctx, tris)
        try:
            assert th.info().leaf_count == leaves
            _, count, rows = check_boxes(psm, th, tris, lo, hi, (1, 16))
            assert count.max() == leaves == count[0] and (leaves == 0 or count.min() == 0)
            if leaves == 1:
                assert rows[0, 0] == 1                                # the lone leaf, by its load-order id
        finally:
            th.close()


def test_box_deep_fixture(psm, ctx):
    """the stack spills past its LDS part (while the id list is in use)"""
    tris, o, d = Q.deep_fixture()
    th = _hier(psm, ctx, tris)
    try:
        rng = np.random.RandomState(33)
        centre = (o + d * np.linspace(0.4, 1.6, o.shape[0]).astype(F)[:, None]).astype(np.float64)
        half = 10.0 ** rng.uniform(-3, 0, (o.shape[0], 1)) * rng.uniform(0.2, 1.0, (o.shape[0], 3))
        lo, hi = (centre - half).astype(F), (centre + half).astype(F)
        pts = tris.reshape(-1, 3)
        lo[0], hi[0] = pts.min(0), pts.max(0)                        # every leaf is reached: the deepest too
        _, count, _ = check_boxes(psm, th, tris, lo, hi, (4, 16))
        assert count[0] == th.info().leaf_count and (count > 0).sum() > o.shape[0] // 4
    finally:
        th.close()


@pytest.mark.parametrize("n", [1, 63, 65, GRID_CAP * 64 + 65])
def test_box_batch_sizes(psm, ctx, n):
    """the last size takes a second trip of the grid-stride loop: the count and the list must start empty again"""
    rng = np.random.RandomState(34)
    c = rng.uniform(-1, 1, (64, 1, 3))
    tris = (c + rng.uniform(-0.3, 0.3, (64, 3, 3))).astype(F)
    rng = np.random.RandomState(n % 1000)
    centre = rng.uniform(-1.2, 1.2, (n, 3)).astype(F)
    half = rng.uniform(0.0, 0.5, (n, 3)).astype(F)
    th = _hier(psm, ctx, tris)
    try:
        _, count, _ = check_boxes(psm, th, tris, centre - half, centre + half, (2,))
        if n > 64:
            assert len(np.unique(count)) > 2 and len(np.unique(count[-65:])) > 2
    finally:
        th.close()


# the optimisation matrices of test_gpu_point_query.py: the fit transform's 3 x 3 part is full, the prune's row sums matter
ROT_SCALE = np.array([[np.cos(0.3), 0, np.sin(0.3), 0.5], [0, 1.3, 0, -1.0], [-np.sin(0.3), 0, np.cos(0.3), 2.0], [0, 0, 0, 1]])
SHEAR = np.array([[1, 0.6, 0, 0.2], [0, 1, -0.4, 0], [0.3, 0, 1, -1], [0, 0, 0, 1]])


@pytest.mark.parametrize("opt", [ROT_SCALE, SHEAR], ids=["rotate_scale", "shear"])
def test_box_optimisation_matrix(psm, ctx, opt):
    rng = np.random.RandomState(35)
    c = rng.uniform(-1, 1, (1500, 1, 3)) * [1.0, 0.3, 2.0]
    tris = (c + rng.uniform(-0.08, 0.08, (1500, 3, 3))).astype(F)
    n = 3000
    centre = rng.uniform(-1.1, 1.1, (n, 3)) * [1.0, 0.3, 2.0]
    half = 10.0 ** rng.uniform(-3, -0.3, (n, 1)) * rng.uniform(0.2, 1.0, (n, 3))
    lo, hi = (centre - half).astype(F), (centre + half).astype(F)
    pts = tris.reshape(-1, 3)
    lo[:64] = hi[:64] = tris[rng.choice(1500, 64), 0]                # point boxes on a v0 (they count): the tightest case for the prune
    hi[32:64] += F(1e-3)
    lo[64:128] = hi[64:128] = pts[rng.choice(pts.shape[0], 64)]      # ... and on any vertex (off v0 rounding may miss: the model says)
    th = _hier(psm, ctx, tris, opt)
    try:
        assert np.abs(np.array(th.info().transform).reshape(4, 4)[:3, :3] - np.diag(np.diag(np.array(th.info().transform).reshape(4, 4)[:3, :3]))).max() > 0.01
        _, count, _ = check_boxes(psm, th, tris, lo, hi, (3, 16))
        assert (count[:64] >= 1).all() and (count == 0).sum() > 100 and (count > 16).sum() > 20
    finally:
        th.close()


def test_box_after_refit(psm, ctx, scenes):
    sc = scenes.cornell()
    tris = sc["tris"].reshape(-1, 3, 3).copy()
    th = _hier(psm, ctx, tris)
    try:
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
        centre = np.concatenate([rng.uniform(blo, bhi, (960, 3)), moved[k].mean(axis=1).repeat(8, axis=0)])
        half = rng.uniform(0.0, 0.15, (1024, 3)) * (bhi - blo)
        _, count, rows = check_boxes(psm, th, moved, (centre - half).astype(F), (centre + half).astype(F), (4, 16))
        assert np.isin(rows, k).any() and (count > 0).sum() > 200
    finally:
        th.close()


def test_box_torch_tensors_on_a_side_stream(psm, ctx, scenes):
    if torch is None:
        pytest.skip("torch is not installed")
    sc = scenes.cornell()
    tris = sc["tris"].reshape(-1, 3, 3)
    rng = np.random.RandomState(6)
    blo, bhi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    centre = rng.uniform(blo, bhi, (4099, 3))
    half = rng.uniform(0.0, 0.1, (4099, 3)) * (bhi - blo)
    lo, hi = (centre - half).astype(F), (centre + half).astype(F)
    th = _hier(psm, ctx, tris)
    try:
        flag, count, lists = th.boxOverlaps(lo, hi), th.boxCount(lo, hi), th.boxTriangles(lo, hi, 5)
        assert flag.any() and not flag.all()
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            tlo, thi = (torch.from_numpy(x).to(dev, non_blocking=True) for x in (lo, hi))
            gflag, gcount, glists = th.boxOverlaps(tlo, thi), th.boxCount(tlo, thi), th.boxTriangles(tlo, thi, 5)
            bufs = [x.cpu() for x in (gflag, gcount, glists.tri, glists.count)]   # (on the side stream: in order)
        assert gflag.device == dev and gflag.dtype == torch.bool and gcount.dtype == torch.int32
        assert glists.tri.shape == (4099, 5) and glists.tri.dtype == torch.int32 and glists.count.dtype == torch.int32
        _same(bufs[0].numpy(), flag, "torch boxOverlaps")
        _same(bufs[1].numpy().view(U), count, "torch boxCount")
        _same(bufs[2].numpy(), lists.tri, "torch boxTriangles")
        _same(bufs[3].numpy().view(U), lists.count, "torch boxTriangles count")
    finally:
        th.close()


def test_box_refusals_launch_nothing(psm, ctx):
    """a call before the build, k = 0, k = 17, NULL and misaligned pointers are refused on the host: the outputs keep what they held"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(4)
    th.loadTriangles(tri.reshape(1, 9))
    n = 4
    hin, hout, hcnt = ctx.buf_alloc(32 * n), ctx.buf_alloc(4 * 17 * n), ctx.buf_alloc(4 * n + 16)
    try:
        boxes = np.zeros((n, 8), F)
        boxes[:, 0:3], boxes[:, 4:7] = -2.0, 2.0
        ctx.buf_upload(hin, boxes)
        ctx.buf_upload(hout, np.full(17 * n, 7, np.int32))
        ctx.buf_upload(hcnt, np.full(n + 4, 77, U))
        pin, pout, pcnt = (ctypes.c_void_p(ctx.buf_ptr(h)[0]) for h in (hin, hout, hcnt))
        size = ctypes.c_size_t(n)

        def tris_call(k, p_in=pin, p_out=pout, p_cnt=pcnt, count=size):
            return lib.psm_bvh_box_triangles_dev(th._h, p_in, count, ctypes.c_uint32(k), p_out, p_cnt)

        def flat_call(fn, p_in=pin, p_out=pcnt, count=size):
            return fn(th._h, p_in, count, p_out)
        for fn in (lib.psm_bvh_box_overlaps_dev, lib.psm_bvh_box_count_dev):
            assert flat_call(fn) == -5                                # before the build: PSM_ERR_STATE
            assert b"box query before build" in lib.psm_last_error(ctx._h)
            assert flat_call(fn, count=ctypes.c_size_t(0)) == 0      # n = 0 is answered first, as for every query
        assert tris_call(4) == -5 and b"box query before build" in lib.psm_last_error(ctx._h)
        th.build()
        for k in (0, 17, 1 << 31):
            assert tris_call(k) == -1
            assert b"k must be 1 .. 16" in lib.psm_last_error(ctx._h)
        assert tris_call(4, p_out=None) == -1 and tris_call(4, p_cnt=None) == -1 and tris_call(4, p_in=None) == -1
        assert tris_call(4, p_in=ctypes.c_void_p(pin.value + 4)) == -1 and b"boxes not 16-byte aligned" in lib.psm_last_error(ctx._h)
        assert tris_call(4, p_out=ctypes.c_void_p(pout.value + 2)) == -1 and b"tris not 4-byte aligned" in lib.psm_last_error(ctx._h)
        assert tris_call(4, p_cnt=ctypes.c_void_p(pcnt.value + 2)) == -1 and b"counts not 4-byte aligned" in lib.psm_last_error(ctx._h)
        for fn in (lib.psm_bvh_box_overlaps_dev, lib.psm_bvh_box_count_dev):
            assert flat_call(fn, p_in=None) == -1 and flat_call(fn, p_out=None) == -1
            assert flat_call(fn, p_in=ctypes.c_void_p(pin.value + 8)) == -1
        assert flat_call(lib.psm_bvh_box_count_dev, p_out=ctypes.c_void_p(pcnt.value + 2)) == -1
        ctx.sync()
        assert (ctx.buf_download(hout, np.int32, 17 * n) == 7).all() and (ctx.buf_download(hcnt, U, n + 4) == 77).all()
        for k in (0, 17):
            with pytest.raises(psm.PsmError):
                th.boxTriangles(boxes[:, 0:3], boxes[:, 4:7], k)
        assert tris_call(16) == 0                                      # and the same buffers are fine at k = 16
        ctx.sync()
        assert (ctx.buf_download(hcnt, U, n) == 1).all()
        rows = ctx.buf_download(hout, np.int32, 17 * n)
        assert (rows[:16 * n].reshape(n, 16) == [0] + [-1] * 15).all() and (rows[16 * n:] == 7).all()
    finally:
        for h in (hin, hout, hcnt):
            ctx.buf_free(h)
        th.close()
