"""The sphere sweeps on the GPU (psm_bvh_sweep_sphere_dev / psm_bvh_sweep_occluded_dev, sweep.hip; TriangleHierarchy.sweepSphere /
sweepOccluded). The yardstick is tests/sweep_query_model.py: sweep_tri in numpy float32 by brute force over the
hierarchy's leaves. Every comparison is exact on every sweep -- t, u, v bit for bit, and tri -- and in every case the queries
are also held against one another: sweepOccluded == isfinite(sweepSphere.t), and t == 0 exactly where within(origin, radius)
counts a triangle."""
import ctypes
import os
import re

import numpy as np
import pytest

import query_model as Q
import sweep_query_model as SQ
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


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, "%s: %d differ, first %d: %s against %s" % (what, bad.size, bad[0], a[bad[0]], b[bad[0]])


def check_sweeps(psm, th, tris, o, d, r, tmax=np.inf):
    """both queries against the model and against one another and the within query; returns the model's records [n, 4]"""
    o, d = np.ascontiguousarray(o, F).reshape(-1, 3), np.ascontiguousarray(d, F).reshape(-1, 3)
    n = o.shape[0]
    r, tm = (np.broadcast_to(np.asarray(x, F), (n,)).astype(F) for x in (r, tmax))
    want, occluded = SQ.query(tris, _leaves(psm, th), o, d, r, tm)
    got, flag = th.sweepSphere(o, d, r, tm), th.sweepOccluded(o, d, r, tm)
    assert got.buffer.shape == (n, 4) and got.buffer.dtype == F and got.tri.dtype == np.int32
    assert flag.shape == (n,) and flag.dtype == np.bool_
    _same(got.buffer.view(U), want.view(U), "sweepSphere (u, v, t, tri as bits)")
    _same(flag, occluded, "sweepOccluded")
    assert np.array_equal(flag, np.isfinite(got.t)) and np.array_equal(flag, got.tri >= 0)
    valid = SQ.sweep_valid(o, Q.normalize3(d), r, tm)
    with np.errstate(invalid="ignore"):
        rq = np.where(r >= 0, r, F(-1))                      # (a NaN radius: within misses on a negative one as well)
    _same(got.t == 0, th.within(np.where(np.isfinite(o), o, F(0)), rq) & valid & np.isfinite(o).all(axis=1), "t == 0 against within")
    return want


def check_closed(th, o, d, r, tmax, want):
    """every hit again with tmax = t (the same record) and with the float before t (a miss; a t = 0 hit unchanged)"""
    n = want.shape[0]
    r, tm = (np.broadcast_to(np.asarray(x, F), (n,)).astype(F) for x in (r, tmax))
    t, hit = want[:, 2], np.isfinite(want[:, 2])
    at = th.sweepSphere(o, d, r, np.where(hit, t, tm))
    _same(at.buffer.view(U), want.view(U), "tmax = t")
    before = th.sweepSphere(o, d, r, np.where(hit & (t > 0), np.nextafter(t, F(0)), np.where(hit, t, tm)))
    gone = hit & (t > 0)
    assert gone.sum() > 0 and np.isinf(before.t[gone]).all() and (before.tri[gone] == -1).all()
    _same(before.buffer[~gone].view(U), want[~gone].view(U), "tmax = the float before t, t = 0 hits and misses")


def check_from_contact(psm, th, tris, o, d, r, want, most=512):
    """hits with t > 0 issued again from where they ended, fl(o + t d), along the same direction: the sphere rests on a triangle
    within rounding of its radius and moves into it, so it must touch at once -- by the start test or by a feature at t = 0 or a
    rounding later (1e-3: coordinates of a few units, down to a cosine of 1e-4 between the path and the contact normal) -- and
    equal the model bit for bit as everything else"""
    n = want.shape[0]
    r = np.broadcast_to(np.asarray(r, F), (n,)).astype(F)
    k = np.nonzero(np.isfinite(want[:, 2]) & (want[:, 2] > 0) & (r > 0))[0][:most]   # (radius 0 is a ray: from the surface it may start behind it)
    dn = Q.normalize3(np.ascontiguousarray(d, F)[k])
    o2 = (np.ascontiguousarray(o, F)[k] + want[k, 2:3] * dn).astype(F)
    got = th.sweepSphere(o2, dn, r[k])
    again, _ = SQ.query(tris, _leaves(psm, th), o2, dn, r[k])
    _same(got.buffer.view(U), again.view(U), "re-issued from the contact")
    assert k.size > 100 and np.isfinite(got.t).all() and got.t.max() <= 1e-3 and (got.t == 0).sum() > k.size // 4


def lattice_soup(seed, count):
    """triangles with vertices on the 1/8 lattice of [-1, 1]^3, each vertex within a step of one lattice point"""
    rng = np.random.RandomState(seed)
    a = rng.randint(-8, 9, (count, 1, 3))
    a[count // 2:] = rng.randint(0, 5, (count - count // 2, 1, 3))   # half of them crowd one octant
    return (np.clip(a + rng.randint(-1, 2, (count, 3, 3)), -8, 8) / 8.0).astype(F)


def test_sweep_lattice_soup(psm, ctx):
    """sweeps from lattice points along the axes and diagonals, radii multiples of 1/16: many contacts are exact, ties happen"""
    tris = lattice_soup(41, 500)
    rng = np.random.RandomState(42)
    n = 2048
    o = (rng.randint(-12, 13, (n, 3)) / 8.0).astype(F)
    dirs = np.concatenate([np.eye(3), -np.eye(3), [[1, 1, 0], [0, -1, 1], [1, 0, -1], [1, 1, 1], [-1, 1, -1], [-1, -1, -1]]]).astype(F)
    d = dirs[rng.randint(0, dirs.shape[0], n)]
    r = (rng.randint(0, 9, n) / 16.0).astype(F)
    th = _hier(psm, ctx, tris)
    try:
        want = check_sweeps(psm, th, tris, o, d, r)
        t = want[:, 2]
        assert np.isfinite(t).sum() > 1000 and np.isinf(t).sum() > 50 and (t == 0).sum() > 50
        assert (np.isfinite(t) & (r == 0)).sum() > 10                  # radius 0 finds lattice triangles
        check_closed(th, o, d, r, np.inf, want)
        check_from_contact(psm, th, tris, o, d, r, want)
    finally:
        th.close()


def test_sweep_random_soup(psm, ctx):
    rng = np.random.RandomState(43)
    c = rng.uniform(-1, 1, (2000, 1, 3))
    tris = (c + rng.uniform(-0.1, 0.1, (2000, 3, 3))).astype(F)
    n = 2048
    o = rng.uniform(-1.6, 1.6, (n, 3)).astype(F)
    d = (rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(F)      # any length: normalised inside
    r = (10.0 ** rng.uniform(-3.5, -0.5, n)).astype(F)                                # radii over three decades
    tm = np.full(n, np.inf, F)
    tm[:1024] = rng.uniform(0, 2, 1024)
    o[0, 0], d[1, 1], o[2, 2], d[3, 0], d[4] = np.nan, np.nan, np.inf, -np.inf, 0
    r[5], r[6], r[7], tm[8], tm[9] = np.nan, -0.5, np.inf, np.nan, -1.0
    r[10:74] = 0
    tm[74:138] = 0
    o[138:202] = tris[rng.choice(2000, 64)].mean(axis=1)                               # origins inside the soup: t = 0
    tm[170:202] = np.inf
    r[138:202] = np.maximum(r[138:202], F(1e-3))
    th = _hier(psm, ctx, tris)
    try:
        want = check_sweeps(psm, th, tris, o, d, r, tm)
        t, tri = want[:, 2], want.view(np.int32)[:, 3]
        assert np.isinf(t[:10]).all() and (tri[:10] == -1).all()
        assert (t[138:202] == 0).all() and (tri[138:202] >= 0).all()
        assert np.isfinite(t[10:74]).any() and (t[74:138][np.isfinite(t[74:138])] == 0).all()
        assert np.isfinite(t[1024:]).sum() > 300 and np.isinf(t[1024:]).sum() > 100 and (np.isfinite(t[202:1024]) & (t[202:1024] > 0)).sum() > 50
        check_closed(th, o, d, r, tm, want)
        check_from_contact(psm, th, tris, o, d, r, want)
    finally:
        th.close()


def test_sweep_tiny_hierarchies(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    rng = np.random.RandomState(44)
    o = rng.uniform(-1.5, 3.0, (200, 3)).astype(F)
    d = (np.array([1.25, 0, 0]) - o + rng.uniform(-1.5, 1.5, (200, 3))).astype(F)
    r = rng.uniform(0.0, 0.6, 200).astype(F)
    o[0], d[0], r[0] = [-1, 0, 0], [1, 0, 0], 0.25
    degenerate = np.repeat(tri[:, :1], 3, axis=1)                    # three equal vertices: the build keeps no leaf
    for tris, leaves in ((np.concatenate([degenerate] * 4), 0), (np.concatenate([degenerate, tri, degenerate]), 1),
                         (np.concatenate([tri, degenerate, tri + F([0.5, 0, 0])]), 2),
                         (np.concatenate([tri, tri + F([0.25, 0, 0]), degenerate, tri + F([0.5, 0, 0])]), 3)):
        th = _hier(psm, ctx, tris)
        try:
            assert th.info().leaf_count == leaves
            want = check_sweeps(psm, th, tris, o, d, r)
            if leaves == 0:
                assert np.isinf(want[:, 2]).all()
            else:
                assert want[0, 2] == 1.75 and want.view(np.int32)[0, 3] == (1 if leaves == 1 else 0)   # the first wall, by its load-order id
                assert 20 < np.isfinite(want[:, 2]).sum() < 200
        finally:
            th.close()


def test_sweep_deep_fixture(psm, ctx):
    """the stack spills past its LDS part; one sweep's radius reaches every leaf: all tie at t = 0 and the lowest id wins"""
    tris, o, d = Q.deep_fixture()
    th = _hier(psm, ctx, tris)
    try:
        rng = np.random.RandomState(45)
        n = o.shape[0]
        r = (10.0 ** rng.uniform(-4, -1, n)).astype(F)
        o2 = (o + rng.uniform(-0.02, 0.02, (n, 3))).astype(F)
        pts = tris.reshape(-1, 3)
        o2[0], r[0] = pts.mean(0), 2 * np.abs(pts).max() + 1             # every leaf is reached: the deepest too
        tm = np.full(n, np.inf, F)
        tm[1::4] = rng.uniform(0.01, 1.0, tm[1::4].size)
        want = check_sweeps(psm, th, tris, o2, d, r, tm)
        t, tri = want[:, 2], want.view(np.int32)[:, 3]
        assert t[0] == 0 and tri[0] == np.sort(_leaves(psm, th))[0]
        assert np.isfinite(t).sum() > n // 2 and len(np.unique(tri)) > 10
    finally:
        th.close()


@pytest.mark.parametrize("n", [1, 63, 65, GRID_CAP * 64 + 65])
def test_sweep_batch_sizes(psm, ctx, n):
    """the last size takes a second trip of the grid-stride loop: the best so far must start at tmax again"""
    rng = np.random.RandomState(46)
    c = rng.uniform(-1, 1, (6, 1, 3))                                 # (few triangles: the yardstick is n x 6 pairs)
    tris = (c + rng.uniform(-0.5, 0.5, (6, 3, 3))).astype(F)
    rng = np.random.RandomState(n % 1000)
    o = rng.uniform(-2, 2, (n, 3)).astype(F)
    d = (rng.uniform(-0.8, 0.8, (n, 3)) - o).astype(F)
    r = rng.uniform(0.0, 0.3, n).astype(F)
    tm = np.where(rng.uniform(size=n) < 0.5, rng.uniform(0, 3, n), np.inf).astype(F)
    th = _hier(psm, ctx, tris)
    try:
        want = check_sweeps(psm, th, tris, o, d, r, tm)
        if n > 64:
            tri = want.view(np.int32)[:, 3]
            assert len(np.unique(tri)) == 7 and len(np.unique(tri[-65:])) > 4 and (tri[-65:] == -1).any()
    finally:
        th.close()


# the optimisation matrices of test_gpu_point_query.py: the fit transform's 3 x 3 part is full, the prune's row sums matter
ROT_SCALE = np.array([[np.cos(0.3), 0, np.sin(0.3), 0.5], [0, 1.3, 0, -1.0], [-np.sin(0.3), 0, np.cos(0.3), 2.0], [0, 0, 0, 1]])
SHEAR = np.array([[1, 0.6, 0, 0.2], [0, 1, -0.4, 0], [0.3, 0, 1, -1], [0, 0, 0, 1]])


@pytest.mark.parametrize("opt", [ROT_SCALE, SHEAR], ids=["rotate_scale", "shear"])
def test_sweep_optimisation_matrix(psm, ctx, opt):
    rng = np.random.RandomState(47)
    c = rng.uniform(-1, 1, (1500, 1, 3)) * [1.0, 0.3, 2.0]
    tris = (c + rng.uniform(-0.08, 0.08, (1500, 3, 3))).astype(F)
    n = 2048
    o = (rng.uniform(-1.4, 1.4, (n, 3)) * [1.0, 0.3, 2.0]).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)
    r = (10.0 ** rng.uniform(-3, -0.7, n)).astype(F)
    # the tightest case for the prune: sweeps that pass a vertex at the radius, give or take a few ulps
    k = rng.choice(1500, 256)
    q = tris[k, rng.randint(0, 3, 256)].astype(np.float64)
    dd = d[:256].astype(np.float64)
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    perp = np.cross(dd, rng.normal(size=(256, 3)))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    o[:256] = (q + perp * r[:256, None] - dd * rng.uniform(0.2, 1.5, (256, 1))).astype(F)
    r[:256] = (r[:256] + rng.randint(-8, 9, 256) * np.spacing(r[:256])).astype(F)
    th = _hier(psm, ctx, tris, opt)
    try:
        m = np.array(th.info().transform).reshape(4, 4)[:3, :3]
        assert np.abs(m - np.diag(np.diag(m))).max() > 0.01
        want = check_sweeps(psm, th, tris, o, d, r)
        assert np.isfinite(want[:, 2]).sum() > 500 and np.isinf(want[:, 2]).sum() > 300
    finally:
        th.close()


def test_sweep_after_refit(psm, ctx, scenes):
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
        n = 1024
        o = rng.uniform(blo, bhi, (n, 3)).astype(F)
        target = np.concatenate([rng.uniform(blo, bhi, (n - 256, 3)), moved[k].mean(axis=1).repeat(32, axis=0)])
        r = (rng.uniform(0.001, 0.05, n) * (bhi - blo).max()).astype(F)
        want = check_sweeps(psm, th, moved, o, (target - o).astype(F), r)
        assert np.isin(want.view(np.int32)[:, 3], k).any() and np.isfinite(want[:, 2]).sum() > 800
    finally:
        th.close()


def test_sweep_torch_tensors_on_a_side_stream(psm, ctx, scenes):
    if torch is None:
        pytest.skip("torch is not installed")
    sc = scenes.cornell()
    tris = sc["tris"].reshape(-1, 3, 3)
    rng = np.random.RandomState(6)
    blo, bhi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    n = 4099
    o = rng.uniform(blo, bhi, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)
    r = (rng.uniform(0.0, 0.05, n) * (bhi - blo).max()).astype(F)
    tm = np.where(rng.uniform(size=n) < 0.5, rng.uniform(0, 1, n) * (bhi - blo).max(), np.inf).astype(F)
    th = _hier(psm, ctx, tris)
    try:
        hits, flag = th.sweepSphere(o, d, r, tm), th.sweepOccluded(o, d, r, tm)
        scalar = th.sweepSphere(o, d, 0.01, 2.5)
        assert flag.any() and not flag.all()
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            to, td, tr, tt = (torch.from_numpy(x).to(dev, non_blocking=True) for x in (o, d, r, tm))
            ghits, gflag, gscalar = th.sweepSphere(to, td, tr, tt), th.sweepOccluded(to, td, tr, tt), th.sweepSphere(to, td, 0.01, 2.5)
            bufs = [x.cpu() for x in (ghits.buffer, gflag, gscalar.buffer)]   # (on the side stream: in order)
        assert ghits.buffer.device == dev and ghits.buffer.shape == (n, 4) and ghits.tri.dtype == torch.int32
        assert gflag.device == dev and gflag.dtype == torch.bool
        _same(bufs[0].numpy().view(U), hits.buffer.view(U), "torch sweepSphere")
        _same(bufs[1].numpy(), flag, "torch sweepOccluded")
        _same(bufs[2].numpy().view(U), scalar.buffer.view(U), "torch sweepSphere, scalar radius and tmax")
    finally:
        th.close()


def test_sweep_refusals_launch_nothing(psm, ctx):
    """a call before the build, NULL and misaligned pointers are refused on the host: the outputs keep what they held"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(4)
    th.loadTriangles(tri.reshape(1, 9))
    n = 4
    hin, hout, hbyte = ctx.buf_alloc(32 * n + 32), ctx.buf_alloc(16 * n + 32), ctx.buf_alloc(16)
    try:
        sweeps = np.zeros((n, 8), F)
        sweeps[:, 0:4], sweeps[:, 4:8] = [-1, 0, 0, 0.25], [1, 0, 0, np.inf]
        ctx.buf_upload(hin, np.concatenate([sweeps.reshape(-1), np.zeros(8, F)]))
        ctx.buf_upload(hout, np.full(4 * n + 8, 7, np.int32))
        ctx.buf_upload(hbyte, np.full(16, 77, np.uint8))
        pin, pout, pbyte = (ctypes.c_void_p(ctx.buf_ptr(h)[0]) for h in (hin, hout, hbyte))
        size = ctypes.c_size_t(n)

        def hits_call(p_in=pin, p_out=pout, count=size):
            return lib.psm_bvh_sweep_sphere_dev(th._h, p_in, count, p_out)

        def flag_call(p_in=pin, p_out=pbyte, count=size):
            return lib.psm_bvh_sweep_occluded_dev(th._h, p_in, count, p_out)
        for call in (hits_call, flag_call):
            assert call() == -5                                        # before the build: PSM_ERR_STATE
            assert b"sweep query before build" in lib.psm_last_error(ctx._h)
            assert call(count=ctypes.c_size_t(0)) == 0                # n = 0 is answered first, as for every query
        th.build()
        for call in (hits_call, flag_call):
            assert call(p_in=None) == -1 and b"NULL pointer" in lib.psm_last_error(ctx._h)
            assert call(p_out=None) == -1 and b"NULL pointer" in lib.psm_last_error(ctx._h)
        assert hits_call(p_in=ctypes.c_void_p(pin.value + 4)) == -1 and b"sweeps or hits not 16-byte aligned" in lib.psm_last_error(ctx._h)
        assert hits_call(p_out=ctypes.c_void_p(pout.value + 8)) == -1 and b"sweeps or hits not 16-byte aligned" in lib.psm_last_error(ctx._h)
        assert flag_call(p_in=ctypes.c_void_p(pin.value + 8)) == -1 and b"sweeps not 16-byte aligned" in lib.psm_last_error(ctx._h)
        ctx.sync()
        assert (ctx.buf_download(hout, np.int32, 4 * n + 8) == 7).all() and (ctx.buf_download(hbyte, np.uint8, 16) == 77).all()
        assert hits_call() == 0 and flag_call(p_out=ctypes.c_void_p(pbyte.value + 1)) == 0      # a byte per query: any address
        ctx.sync()
        out = ctx.buf_download(hout, np.int32, 4 * n + 8)
        rec = out[:4 * n].reshape(n, 4)
        assert (rec.view(F)[:, :3] == [0.25, 0.5, 1.75]).all() and (rec[:, 3] == 0).all() and (out[4 * n:] == 7).all()
        assert list(ctx.buf_download(hbyte, np.uint8, 16)) == [77] + [1] * n + [77] * (15 - n)
    finally:
        for h in (hin, hout, hbyte):
            ctx.buf_free(h)
        th.close()
