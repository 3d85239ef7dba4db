"""The triangle queries on the GPU (psm_bvh_tri_overlaps_dev / psm_bvh_tri_count_dev / psm_bvh_tri_triangles_dev, tri.hip;
TriangleHierarchy.triOverlaps / triCount / triTriangles). The yardstick is tests/tri_query_model.py: tri_tri in
numpy float32 by brute force over the hierarchy's leaves. Every comparison is exact on every query, and in every case the three
queries are also held against one another: overlaps == (count > 0), triangles.count == min(k, count), rows are prefixes."""
import ctypes
import os
import re

import numpy as np
import pytest

import query_model as Q
import tri_query_model as TQ
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


def check_tris(psm, th, tris, q, ks=KS):
    """the three queries against the model (computed once at the largest k: its rows are prefixes, test_tri_query_cpu) and
    against one another; returns the model's flag, full count and rows at the largest k"""
    q = np.ascontiguousarray(q, F).reshape(-1, 3, 3)
    n = q.shape[0]
    flag, count, rows, _ = TQ.query(tris, _leaves(psm, th), q, max(ks))
    got_flag, got_count = th.triOverlaps(q), th.triCount(q.reshape(n, 9))     # (either shape of the argument)
    assert got_flag.shape == (n,) and got_flag.dtype == np.bool_ and got_count.shape == (n,) and got_count.dtype == U
    _same(got_flag, flag, "triOverlaps")
    _same(got_count, count, "triCount")
    assert np.array_equal(got_flag, got_count > 0)
    widest = None
    for k in sorted(ks, reverse=True):
        got = th.triTriangles(q, k)
        assert got.tri.shape == (n, k) and got.tri.dtype == np.int32 and got.count.shape == (n,) and got.count.dtype == U
        _same(got.tri, rows[:, :k], "triTriangles k = %d" % k)
        _same(got.count, np.minimum(got_count, U(k)), "triTriangles count against triCount, k = %d" % k)
        assert np.array_equal(got.tri >= 0, np.arange(k)[None] < got.count[:, None])
        if widest is None:
            widest = got.tri
        _same(got.tri, widest[:, :k], "triTriangles k = %d is a prefix of k = %d" % (k, max(ks)))
    return flag, count, rows


def lattice_soup(seed, count):
    """triangles with vertices on the 1/8 lattice of [-1, 1]^3, each vertex within a step of one lattice point"""
    rng = np.random.RandomState(seed)
    a = rng.randint(-8, 9, (count, 1, 3))
    a[count // 2:] = rng.randint(0, 5, (count - count // 2, 1, 3))   # half of them crowd one octant: queries that meet more than 16
    return (np.clip(a + rng.randint(-1, 2, (count, 3, 3)), -8, 8) / 8.0).astype(F)


def test_tri_lattice_soup(psm, ctx):
    """all arithmetic exact: lattice queries of three sizes, copies of the stored triangles, and their coplanar neighbours (a
    copy moved along one of its own edges, and one mirrored over an edge)"""
    tris = lattice_soup(41, 500)
    rng = np.random.RandomState(42)
    a = rng.randint(-8, 9, (1400, 1, 3))
    q = [np.clip(a + rng.randint(-1, 2, (1400, 3, 3)) * rng.randint(1, 4, (1400, 1, 1)), -8, 8) / 8.0]
    src = rng.choice(500, 200)
    pick = tris[src].astype(np.float64)
    q.append(pick)                                                           # the stored triangles themselves
    q.append(pick + (pick[:, 1:2] - pick[:, 0:1]))                           # moved along the edge v0 v1: coplanar, touching at v1
    q.append(np.stack([pick[:, 0], pick[:, 1], pick[:, 0] + pick[:, 1] - pick[:, 2]], axis=1))   # mirrored over the midpoint of v0 v1
    q = np.concatenate(q).astype(F)
    th = _hier(psm, ctx, tris)
    try:
        flag, count, _ = check_tris(psm, th, tris, q)
        assert q.shape[0] == 2000 and flag.sum() > 1000 and (~flag).sum() > 20 and (count > 16).any()
        kept = np.tile(np.isin(src, _leaves(psm, th)), 3)                    # (a triangle with three equal vertices is no leaf)
        assert kept.sum() > 550 and (count[1400:][kept] >= 1).all()          # exact arithmetic: each meets the triangle it came from
        # two stored triangles sharing an edge: a query lying in that edge meets both; one a step off meets neither
        pair = np.array([[[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]], [[0, 0, 0], [0.5, 0, 0], [0, 0, 0.5]]], F)
        th2 = _hier(psm, ctx, pair)
        try:
            qq = F([[[0.125, 0, 0], [0.25, 0, 0], [0.375, 0, 0]], [[0.125, -0.125, 0], [0.25, -0.125, -0.125], [0.375, -0.125, 0]],
                    [[0.125, 0.125, 0], [0.125, 0.125, 0], [0.125, 0.125, 0]]])
            f2, c2, r2 = check_tris(psm, th2, pair, qq)
            assert list(c2) == [2, 0, 1] and list(r2[0, :2]) == [0, 1] and r2[2, 0] == 0
        finally:
            th2.close()
    finally:
        th.close()


def test_tri_random_soup(psm, ctx):
    rng = np.random.RandomState(43)
    c = rng.uniform(-1, 1, (2000, 1, 3))
    tris = (c + rng.uniform(-0.1, 0.1, (2000, 3, 3))).astype(F)
    n = 4096
    centre = rng.uniform(-1.1, 1.1, (n, 1, 3))
    q = (centre + rng.uniform(-1, 1, (n, 3, 3)) * 10.0 ** rng.uniform(-2.7, 0.3, (n, 1, 1))).astype(F)   # sizes over three decades
    q[0, 0, 0], q[1, 1, 1], q[2, 2, 2], q[3, 0, 1] = np.nan, np.nan, np.inf, -np.inf
    q[4], q[5, 1] = np.inf, -np.inf
    q[6, :, 0] = np.nan
    pts = tris.reshape(-1, 3)
    q[8:40] = tris[rng.choice(2000, 32), 0][:, None, :]                                   # point queries on a v0: A = B = C = 0, they count
    q[40:56] = pts[rng.choice(pts.shape[0], 16)][:, None, :]                              # ... on any vertex (off v0 rounding may miss)
    w = rng.uniform(0, 1, (16, 3, 1))
    w /= w.sum(axis=1, keepdims=True)
    q[56:72] = (tris[rng.choice(2000, 16)] * w).sum(axis=1).astype(F)[:, None, :]         # ... and near interiors
    pick = tris[rng.choice(2000, 48)]
    q[72:88] = np.stack([pick[:16, 0], pick[:16, 0], pick[:16, 1]], axis=1)               # segment queries: an edge itself
    mid = ((pick[16:32, 0] + pick[16:32, 1]) * F(0.5)).astype(F)
    q[88:104] = np.stack([mid, mid, (mid + rng.uniform(-0.2, 0.2, (16, 3))).astype(F)], axis=1)        # ... from a point of an edge
    inner = pick[32:48].mean(axis=1).astype(F)
    q[104:120] = np.stack([(inner - F(0.1)).astype(F), (inner + F(0.1)).astype(F), (inner + F(0.1)).astype(F)], axis=1)   # ... through an interior
    q[120] = [[-3, -3, -0.01], [3, -3, 0.02], [0, 4, 0.0]]                                 # one huge triangle cutting the whole soup
    q[128:640] = tris[:512]                                                               # the mesh's own first 512 triangles
    th = _hier(psm, ctx, tris)
    try:
        leaves = _leaves(psm, th)
        flag, count, rows = check_tris(psm, th, tris, q)
        assert (count[:7] == 0).all() and (count[8:40] >= 1).all() and count[120] > 16
        # a stored triangle as the query meets itself where the stored edges are fl(v1 - v0), fl(v2 - v0): what the model says
        own = np.isin(np.arange(512), leaves)
        v0, e1, e2 = (x[:512] for x in TQ._split(tris))
        itself = TQ.tri_tri(v0, e1, e2, tris[:512, 0], tris[:512, 1], tris[:512, 2])
        print("stored triangles that meet themselves under the model: %d of %d" % (itself[own].sum(), own.sum()))
        if itself[own].all():
            assert (count[128:640][own] >= 1).all()
        assert (count[640:] == 0).sum() > 100 and ((count[640:] > 0) & (count[640:] < 16)).sum() > 100 and (count[640:] > 16).sum() > 20
    finally:
        th.close()


def test_tri_tiny_hierarchies(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    rng = np.random.RandomState(44)
    q = (rng.uniform(-0.5, 2.0, (200, 1, 3)) + rng.uniform(-0.8, 0.8, (200, 3, 3))).astype(F)
    q[0] = [[-4, -0.5, -0.25], [4, -0.5, -0.25], [4, 0.5, 0.5]]      # through all of them
    degenerate = np.repeat(tri[:, :1], 3, axis=1)                    # three equal vertices: the build keeps no leaf
    for tris, leaves in ((np.concatenate([degenerate] * 4), 0), (np.concatenate([degenerate, tri, degenerate]), 1),
                         (np.concatenate([tri, degenerate, tri + F([0.5, 0, 0])]), 2),
                         (np.concatenate([tri, tri + F([0.25, 0, 0]), degenerate, tri + F([0.5, 0, 0])]), 3)):
        th = _hier(psm, ctx, tris)
        try:
            assert th.info().leaf_count == leaves
            _, count, rows = check_tris(psm, th, tris, q, (1, 16))
            assert count.max() == leaves == count[0] and (leaves == 0 or count.min() == 0)
            if leaves == 1:
                assert rows[0, 0] == 1                                # the lone leaf, by its load-order id
        finally:
            th.close()


def test_tri_deep_fixture(psm, ctx):
    """the stack spills past its LDS part (while the id list is in use)"""
    tris, o, d = Q.deep_fixture()
    th = _hier(psm, ctx, tris)
    try:
        rng = np.random.RandomState(45)
        centre = (o + d * np.linspace(0.4, 1.6, o.shape[0]).astype(F)[:, None]).astype(np.float64)
        q = (centre[:, None, :] + rng.uniform(-1, 1, (o.shape[0], 3, 3)) * 10.0 ** rng.uniform(-3, 0, (o.shape[0], 1, 1))).astype(F)
        q[0] = [[-1, -3, -1.5], [3, -3, -1.5], [1, 3, 1.5]]           # a sheet along the row of clusters whose box holds every leaf: all are reached
        _, count, _ = check_tris(psm, th, tris, q, (4, 16))
        assert count[0] > 100 and (count > 0).sum() > o.shape[0] // 4
        assert TQ._unit_pass(*TQ._split(tris), q[0, 0], q[0, 1], q[0, 2]).all()   # its bounding box holds every leaf
    finally:
        th.close()


@pytest.mark.parametrize("n", [1, 63, 65, GRID_CAP * 64 + 65])
def test_tri_batch_sizes(psm, ctx, n):
    """the last size takes a second trip of the grid-stride loop: the count and the list must start empty again"""
    rng = np.random.RandomState(46)
    c = rng.uniform(-1, 1, (16, 1, 3))
    tris = (c + rng.uniform(-0.6, 0.6, (16, 3, 3))).astype(F)
    rng = np.random.RandomState(n % 1000)
    q = (rng.uniform(-1.2, 1.2, (n, 1, 3)) + rng.uniform(-1.0, 1.0, (n, 3, 3))).astype(F)
    th = _hier(psm, ctx, tris)
    try:
        _, count, _ = check_tris(psm, th, tris, q, (2,))
        if n > 64:
            assert len(np.unique(count)) > 2 and len(np.unique(count[-65:])) > 2
    finally:
        th.close()


# the optimisation matrices of test_gpu_point_query.py: the fit transform's 3 x 3 part is full, the prune's row sums matter
ROT_SCALE = np.array([[np.cos(0.3), 0, np.sin(0.3), 0.5], [0, 1.3, 0, -1.0], [-np.sin(0.3), 0, np.cos(0.3), 2.0], [0, 0, 0, 1]])
SHEAR = np.array([[1, 0.6, 0, 0.2], [0, 1, -0.4, 0], [0.3, 0, 1, -1], [0, 0, 0, 1]])


@pytest.mark.parametrize("opt", [ROT_SCALE, SHEAR], ids=["rotate_scale", "shear"])
def test_tri_optimisation_matrix(psm, ctx, opt):
    rng = np.random.RandomState(47)
    c = rng.uniform(-1, 1, (1500, 1, 3)) * [1.0, 0.3, 2.0]
    tris = (c + rng.uniform(-0.08, 0.08, (1500, 3, 3))).astype(F)
    n = 3000
    centre = rng.uniform(-1.1, 1.1, (n, 1, 3)) * [1.0, 0.3, 2.0]
    q = (centre + rng.uniform(-1, 1, (n, 3, 3)) * 10.0 ** rng.uniform(-2.7, 0.3, (n, 1, 1))).astype(F)
    pts = tris.reshape(-1, 3)
    v = tris[rng.choice(1500, 64), 0]
    q[:32] = v[:32, None, :]                                          # point queries on a v0 (they count): the tightest case for the prune
    q[32:64, 0] = v[32:]                                              # ... and queries touching at a v0 with a vertex, reaching anywhere
    q[64:128, 1] = pts[rng.choice(pts.shape[0], 64)]                  # ... at any vertex (off v0 rounding may miss: the model says)
    th = _hier(psm, ctx, tris, opt)
    try:
        M = np.array(th.info().transform).reshape(4, 4)[:3, :3]
        assert np.abs(M - np.diag(np.diag(M))).max() > 0.01
        _, count, _ = check_tris(psm, th, tris, q, (3, 16))
        assert (count[:64] >= 1).all() and (count == 0).sum() > 100 and (count > 16).sum() > 20
    finally:
        th.close()


def test_tri_after_refit(psm, ctx, scenes):
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
        q = (centre[:, None, :] + rng.uniform(-0.15, 0.15, (1024, 3, 3)) * (bhi - blo)).astype(F)
        _, count, rows = check_tris(psm, th, moved, q, (4, 16))
        assert np.isin(rows, k).any() and (count > 0).sum() > 200
    finally:
        th.close()


def test_tri_torch_tensors_on_a_side_stream(psm, ctx, scenes):
    if torch is None:
        pytest.skip("torch is not installed")
    sc = scenes.cornell()
    tris = sc["tris"].reshape(-1, 3, 3)
    rng = np.random.RandomState(6)
    blo, bhi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    q = (rng.uniform(blo, bhi, (4099, 1, 3)) + rng.uniform(-0.1, 0.1, (4099, 3, 3)) * (bhi - blo)).astype(F)
    th = _hier(psm, ctx, tris)
    try:
        flag, count, lists = th.triOverlaps(q), th.triCount(q), th.triTriangles(q, 5)
        assert flag.any() and not flag.all()
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            tq = torch.from_numpy(q).to(dev, non_blocking=True)
            gflag, gcount, glists = th.triOverlaps(tq), th.triCount(tq.reshape(-1, 9)), th.triTriangles(tq, 5)
            bufs = [x.cpu() for x in (gflag, gcount, glists.tri, glists.count)]   # (on the side stream: in order)
        assert gflag.device == dev and gflag.dtype == torch.bool and gcount.dtype == torch.int32
        assert glists.tri.shape == (4099, 5) and glists.tri.dtype == torch.int32 and glists.count.dtype == torch.int32
        _same(bufs[0].numpy(), flag, "torch triOverlaps")
        _same(bufs[1].numpy().view(U), count, "torch triCount")
        _same(bufs[2].numpy(), lists.tri, "torch triTriangles")
        _same(bufs[3].numpy().view(U), lists.count, "torch triTriangles count")
    finally:
        th.close()


def test_tri_refusals_launch_nothing(psm, ctx):
    """a call before the build, k = 0, k = 17, NULL and misaligned pointers are refused on the host: the outputs keep what they held"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(4)
    th.loadTriangles(tri.reshape(1, 9))
    n = 4
    hin, hout, hcnt = ctx.buf_alloc(48 * n + 16), ctx.buf_alloc(4 * 17 * n), ctx.buf_alloc(4 * n + 16)
    try:
        recs = np.zeros((n + 1, 12), F)
        recs[:n] = [0, 0, -2, 0, 2, 0, 2, 0, 2, 1, 2, 0]              # a triangle through the stored one
        ctx.buf_upload(hin, recs[:n])
        ctx.buf_upload(hout, np.full(17 * n, 7, np.int32))
        ctx.buf_upload(hcnt, np.full(n + 4, 77, U))
        pin, pout, pcnt = (ctypes.c_void_p(ctx.buf_ptr(h)[0]) for h in (hin, hout, hcnt))
        size = ctypes.c_size_t(n)

        def tris_call(k, p_in=pin, p_out=pout, p_cnt=pcnt, count=size):
            return lib.psm_bvh_tri_triangles_dev(th._h, p_in, count, ctypes.c_uint32(k), p_out, p_cnt)

        def flat_call(fn, p_in=pin, p_out=pcnt, count=size):
            return fn(th._h, p_in, count, p_out)
        for fn in (lib.psm_bvh_tri_overlaps_dev, lib.psm_bvh_tri_count_dev):
            assert flat_call(fn) == -5                                # before the build: PSM_ERR_STATE
            assert b"triangle query before build" in lib.psm_last_error(ctx._h)
            assert flat_call(fn, count=ctypes.c_size_t(0)) == 0      # n = 0 is answered first, as for every query
        assert tris_call(4) == -5 and b"triangle query before build" in lib.psm_last_error(ctx._h)
        th.build()
        for k in (0, 17, 1 << 31):
            assert tris_call(k) == -1
            assert b"k must be 1 .. 16" in lib.psm_last_error(ctx._h)
        assert tris_call(4, p_out=None) == -1 and tris_call(4, p_cnt=None) == -1 and tris_call(4, p_in=None) == -1
        assert tris_call(4, p_in=ctypes.c_void_p(pin.value + 4)) == -1 and b"triangles not 16-byte aligned" in lib.psm_last_error(ctx._h)
        assert tris_call(4, p_out=ctypes.c_void_p(pout.value + 2)) == -1 and b"tris not 4-byte aligned" in lib.psm_last_error(ctx._h)
        assert tris_call(4, p_cnt=ctypes.c_void_p(pcnt.value + 2)) == -1 and b"counts not 4-byte aligned" in lib.psm_last_error(ctx._h)
        for fn in (lib.psm_bvh_tri_overlaps_dev, lib.psm_bvh_tri_count_dev):
            assert flat_call(fn, p_in=None) == -1 and flat_call(fn, p_out=None) == -1
            assert flat_call(fn, p_in=ctypes.c_void_p(pin.value + 8)) == -1
        assert flat_call(lib.psm_bvh_tri_count_dev, p_out=ctypes.c_void_p(pcnt.value + 2)) == -1
        ctx.sync()
        assert (ctx.buf_download(hout, np.int32, 17 * n) == 7).all() and (ctx.buf_download(hcnt, U, n + 4) == 77).all()
        for k in (0, 17):
            with pytest.raises(psm.PsmError):
                th.triTriangles(recs[:n].reshape(n, 3, 4)[:, :, :3], k)
        assert tris_call(16) == 0                                      # and the same buffers are fine at k = 16
        ctx.sync()
        assert (ctx.buf_download(hcnt, U, n) == 1).all()
        rows = ctx.buf_download(hout, np.int32, 17 * n)
        assert (rows[:16 * n].reshape(n, 16) == [0] + [-1] * 15).all() and (rows[16 * n:] == 7).all()
    finally:
        for h in (hin, hout, hcnt):
            ctx.buf_free(h)
        th.close()
