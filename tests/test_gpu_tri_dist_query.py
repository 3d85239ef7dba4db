"""The clearance queries on the GPU (psm_bvh_tri_closest_dev / psm_bvh_tri_within_dev, tri_dist.hip;
TriangleHierarchy.triClosest / triWithin). The yardstick is tests/tri_dist_query_model.py: tri_dist in numpy
float32 by brute force over the hierarchy's leaves. Every record is compared bit for bit on every query, and in every case the
two queries are held against each other and against the triangle queries: triWithin == (triClosest.tri >= 0), triOverlaps
implies dist == 0, triWithin(q, 0) is at least triOverlaps(q). The sizes keep a case's brute force at about 1.5 M pairs."""
import ctypes
import os
import re

import numpy as np
import pytest

import query_model as Q
import tri_dist_query_model as TD
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


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    ab, bb = (x.view(U) if x.dtype == F else x for x in (a, b))
    bad = np.nonzero((ab != bb).reshape(a.shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, "%s: %d differ, first %d: %s against %s" % (what, bad.size, bad[0], a[bad[0]], b[bad[0]])


def check_clearance(psm, th, tris, q, rmax=np.inf):
    """triClosest and triWithin against the model and against each other and the triangle queries; returns the model's
    records [n, 8]"""
    q = np.ascontiguousarray(q, F).reshape(-1, 3, 3)
    n = q.shape[0]
    want, want_in = TD.query(tris, _leaves(psm, th), q, rmax)
    got, got_in = th.triClosest(q, rmax), th.triWithin(q.reshape(n, 9), rmax)     # (either shape of the argument)
    assert got.buffer.shape == (n, 8) and got.buffer.dtype == F and got_in.shape == (n,) and got_in.dtype == np.bool_
    _same_bits(got.buffer, want, "triClosest")
    _same_bits(got_in, want_in, "triWithin")
    assert np.array_equal(got_in, got.tri >= 0)
    assert not got.buffer[:, 6:].any() and not got.buffer[got.tri < 0][:, [0, 1, 4, 5]].any() and np.isinf(got.dist[got.tri < 0]).all()
    meets = th.triOverlaps(q)
    with np.errstate(invalid="ignore"):
        allowed = TD.query_valid(q, np.broadcast_to(np.asarray(rmax, F), (n,)))
    assert (got.dist[meets & allowed] == 0).all() and (got.tri[meets & allowed] >= 0).all()
    at0 = th.triWithin(q, 0.0)
    assert at0[meets].all()
    return want


def lattice_soup(seed, count):
    """triangles with vertices on the 1/8 lattice of [-1, 1]^3, each vertex within a step of one lattice point"""
    rng = np.random.RandomState(seed)
    a = rng.randint(-8, 9, (count, 1, 3))
    return (np.clip(a + rng.randint(-1, 2, (count, 3, 3)), -8, 8) / 8.0).astype(F)


def test_clearance_lattice_soup(psm, ctx):
    """a 500-triangle lattice soup against 2 000 lattice queries, copies of stored triangles and their coplanar neighbours
    among them, rmax from +inf, 0 and a few lattice distances"""
    tris = lattice_soup(51, 500)
    rng = np.random.RandomState(52)
    a = rng.randint(-12, 13, (1400, 1, 3))                                   # (a part of them outside the soup's cube)
    q = [(a + rng.randint(-1, 2, (1400, 3, 3)) * rng.randint(1, 3, (1400, 1, 1))) / 8.0]
    src = rng.choice(500, 200)
    pick = tris[src].astype(np.float64)
    q.append(pick)                                                           # the stored triangles themselves
    q.append(pick + (pick[:, 1:2] - pick[:, 0:1]))                           # moved along the edge v0 v1: coplanar, touching at v1
    q.append(np.stack([pick[:, 0], pick[:, 1], pick[:, 0] + pick[:, 1] - pick[:, 2]], axis=1))   # mirrored over the midpoint of v0 v1
    q = np.concatenate(q).astype(F)
    rmax = rng.choice(F([np.inf, np.inf, 0.0, 0.125, 0.25, 0.5]), q.shape[0])
    th = _hier(psm, ctx, tris)
    try:
        want = check_clearance(psm, th, tris, q, rmax)
        tri, dist = want.view(np.int32)[:, 3], want[:, 2]
        assert q.shape[0] == 2000 and (tri < 0).sum() > 20 and (dist == 0).sum() > 300 and ((dist > 0) & (tri >= 0)).sum() > 300
        kept = np.tile(np.isin(src, _leaves(psm, th)), 3)                    # (a triangle with three equal vertices is no leaf)
        assert kept.sum() > 550 and (dist[1400:][kept] == 0).all()           # exact arithmetic: each meets the triangle it came from
        check_clearance(psm, th, tris, q[:600])                              # and all of them without a limit
    finally:
        th.close()


def _random_soup_queries(rng, tris, n):
    T = tris.shape[0]
    centre = rng.uniform(-1.1, 1.1, (n, 1, 3))
    q = (centre + rng.uniform(-1, 1, (n, 3, 3)) * 10.0 ** rng.uniform(-2.7, 0.3, (n, 1, 1))).astype(F)   # sizes over three decades
    rmax = np.where(rng.uniform(size=n) < 0.5, np.inf, 10.0 ** rng.uniform(-2.5, 0, n)).astype(F)
    q[0, 0, 0], q[1, 1, 1], q[2, 2, 2], q[3, 0, 1] = np.nan, np.nan, np.inf, -np.inf
    q[4], q[5, 1] = np.inf, -np.inf
    q[6, :, 0] = np.nan
    rmax[8:16] = F([np.nan, -1.0, -np.inf, -0.0, 0.0, np.inf, -1e-30, np.nan])
    pts = tris.reshape(-1, 3)
    q[16:48] = tris[rng.choice(T, 32), 0][:, None, :]                                     # point queries on a v0
    q[48:64] = pts[rng.choice(pts.shape[0], 16)][:, None, :]                              # ... on any vertex
    w = rng.uniform(0, 1, (16, 3, 1))
    w /= w.sum(axis=1, keepdims=True)
    q[64:80] = (tris[rng.choice(T, 16)] * w).sum(axis=1).astype(F)[:, None, :]            # ... and near interiors
    pick = tris[rng.choice(T, 48)]
    q[80:96] = np.stack([pick[:16, 0], pick[:16, 0], pick[:16, 1]], axis=1)               # segment queries: an edge itself
    mid = ((pick[16:32, 0] + pick[16:32, 1]) * F(0.5)).astype(F)
    q[96:112] = np.stack([mid, mid, (mid + rng.uniform(-0.2, 0.2, (16, 3))).astype(F)], axis=1)        # ... from a point of an edge
    inner = pick[32:48].mean(axis=1).astype(F)
    q[112:128] = np.stack([(inner - F(0.1)).astype(F), (inner + F(0.1)).astype(F), (inner + F(0.1)).astype(F)], axis=1)   # ... through an interior
    q[128] = [[-3, -3, -0.01], [3, -3, 0.02], [0, 4, 0.0]]                                 # one huge triangle cutting the whole soup
    rmax[16:129] = np.inf
    q[136:392] = tris[:256]                                                               # the mesh's own first 256 triangles
    rmax[136:392] = np.where(np.arange(256) % 2 == 0, np.inf, 0.0)
    far = rng.normal(size=(64, 1, 3))
    q[392:456] = (far / np.linalg.norm(far, axis=2, keepdims=True) * 10.0 ** rng.uniform(1, 4, (64, 1, 1))
                  + rng.uniform(-1, 1, (64, 3, 3))).astype(F)                             # far outside the scene: the bound's slow case
    rmax[392:456] = np.inf
    return q, rmax


def test_clearance_random_soup(psm, ctx):
    rng = np.random.RandomState(53)
    c = rng.uniform(-1, 1, (1000, 1, 3))
    tris = (c + rng.uniform(-0.1, 0.1, (1000, 3, 3))).astype(F)
    q, rmax = _random_soup_queries(rng, tris, 1024)
    th = _hier(psm, ctx, tris)
    try:
        want = check_clearance(psm, th, tris, q, rmax)
        tri, dist = want.view(np.int32)[:, 3], want[:, 2]
        assert (tri[:7] < 0).all() and (tri[[8, 9, 10, 14, 15]] < 0).all() and tri[13] >= 0
        assert (tri[16:129] >= 0).all() and dist[128] == 0 and (dist[16:48] == 0).all()
        own = np.isin(np.arange(256), _leaves(psm, th))
        assert (dist[136:392][own] == 0).all() and own.sum() > 250            # a stored triangle is at distance 0 of the mesh
        assert (tri[392:456] >= 0).all() and (dist[392:456] > 5).all()
        assert (tri[456:] < 0).sum() > 50 and (dist[456:] == 0).sum() > 50 and ((dist[456:] > 0) & (tri[456:] >= 0)).sum() > 100
        # the two points reproduce the distance: one rounding of each coordinate apart from the kernel's own relative ones
        hit = (tri >= 0) & np.isfinite(q.reshape(-1, 9)).all(axis=1) & (dist > 0) & (np.arange(1024) < 392)
        pm, pq = TD.points_of(tris, q, want)
        again = np.linalg.norm(pm[hit].astype(np.float64) - pq[hit], axis=1)
        assert np.abs(again - dist[hit]).max() <= 1e-5
    finally:
        th.close()


def test_clearance_tiny_hierarchies(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    rng = np.random.RandomState(54)
    q = (rng.uniform(-0.5, 2.0, (200, 1, 3)) + rng.uniform(-0.8, 0.8, (200, 3, 3))).astype(F)
    rmax = rng.choice(F([np.inf, 0.0, 0.3, 1.0]), 200)
    q[0], rmax[0] = [[-4, -0.5, -0.25], [4, -0.5, -0.25], [4, 0.5, 0.5]], 0.0      # through all of them
    degenerate = np.repeat(tri[:, :1], 3, axis=1)                    # three equal vertices: the build keeps no leaf
    for tris, leaves in ((np.concatenate([degenerate] * 4), 0), (np.concatenate([degenerate, tri, degenerate]), 1),
                         (np.concatenate([tri, degenerate, tri + F([0.5, 0, 0])]), 2),
                         (np.concatenate([tri, tri + F([0.25, 0, 0]), degenerate, tri + F([0.5, 0, 0])]), 3)):
        th = _hier(psm, ctx, tris)
        try:
            assert th.info().leaf_count == leaves
            want = check_clearance(psm, th, tris, q, rmax)
            tri_id = want.view(np.int32)[:, 3]
            if leaves == 0:
                assert (tri_id < 0).all()
            else:
                assert want[0, 2] == 0 and tri_id[0] == (1 if leaves == 1 else 0) and (tri_id < 0).any()
                assert (tri_id[rmax == np.inf] >= 0).all()
        finally:
            th.close()


def test_clearance_deep_fixture(psm, ctx):
    """the stack spills past its LDS part"""
    tris, o, d = Q.deep_fixture()
    th = _hier(psm, ctx, tris)
    try:
        rng = np.random.RandomState(55)
        n = o.shape[0]
        centre = (o + d * np.linspace(0.4, 1.6, n).astype(F)[:, None]).astype(np.float64)
        q = (centre[:, None, :] + rng.uniform(-1, 1, (n, 3, 3)) * 10.0 ** rng.uniform(-3, 0, (n, 1, 1))).astype(F)
        q[0] = [[-1, -3, -1.5], [3, -3, -1.5], [1, 3, 1.5]]           # a sheet along the row of clusters
        q[1:33] += F([0, 0.5, 0])                                     # beside the row: every cluster is a candidate for a while
        want = check_clearance(psm, th, tris, q)
        assert (want.view(np.int32)[:, 3] >= 0).all() and want[0, 2] == 0 and (want[1:33, 2] > 0).all()
    finally:
        th.close()


@pytest.mark.parametrize("n", [1, 63, 65, GRID_CAP * 64 + 65])
def test_clearance_batch_sizes(psm, ctx, n):
    """the last size takes a second trip of the grid-stride loop: the best and the record must start afresh per query"""
    tris = F([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 1], [1, 0, 1], [0, 1, 1.5]], [[2, 0, 0], [2, 1, 0], [2, 0, 1]]])
    rng = np.random.RandomState(n % 1000)
    q = (rng.uniform(-1.2, 2.4, (n, 1, 3)) + rng.uniform(-0.5, 0.5, (n, 3, 3))).astype(F)
    rmax = rng.choice(F([np.inf, 0.25, 0.5, 0.0]), n)
    th = _hier(psm, ctx, tris)
    try:
        want = check_clearance(psm, th, tris, q, rmax)
        if n > 64:
            tri = want.view(np.int32)[:, 3]
            assert len(np.unique(tri)) == 4 and len(np.unique(tri[-65:])) >= 3
    finally:
        th.close()


# the optimisation matrices of test_gpu_point_query.py: a rotation with a scale takes the sum form of the bound, a shear the max form
ROT_SCALE = np.array([[np.cos(0.3), 0, np.sin(0.3), 0.5], [0, 1.3, 0, -1.0], [-np.sin(0.3), 0, np.cos(0.3), 2.0], [0, 0, 0, 1]])
SHEAR = np.array([[1, 0.6, 0, 0.2], [0, 1, -0.4, 0], [0.3, 0, 1, -1], [0, 0, 0, 1]])


@pytest.mark.parametrize("opt", [ROT_SCALE, SHEAR], ids=["rotate_scale", "shear"])
def test_clearance_optimisation_matrix(psm, ctx, opt):
    rng = np.random.RandomState(57)
    c = rng.uniform(-1, 1, (1000, 1, 3)) * [1.0, 0.3, 2.0]
    tris = (c + rng.uniform(-0.08, 0.08, (1000, 3, 3))).astype(F)
    n = 1024
    centre = rng.uniform(-1.3, 1.3, (n, 1, 3)) * [1.0, 0.5, 2.0]
    q = (centre + rng.uniform(-1, 1, (n, 3, 3)) * 10.0 ** rng.uniform(-2.7, 0, (n, 1, 1))).astype(F)
    rmax = np.where(rng.uniform(size=n) < 0.5, np.inf, 10.0 ** rng.uniform(-2.5, 0, n)).astype(F)
    v = tris[rng.choice(1000, 64), 0]
    q[:32] = v[:32, None, :]                                          # point queries on a v0: distance 0, the tightest case for the prune
    q[32:64, 0] = v[32:]                                              # ... and queries touching at a v0 with a vertex
    rmax[:64] = 0.0
    th = _hier(psm, ctx, tris, opt)
    try:
        M = np.array(th.info().transform, F).reshape(4, 4)
        assert np.abs(M[:3, :3] - np.diag(np.diag(M[:3, :3]))).max() > 0.01
        assert TD.point_bound(M)[2] == (opt is ROT_SCALE)             # the sum form for the rotation, the max form for the shear
        want = check_clearance(psm, th, tris, q, rmax)
        tri = want.view(np.int32)[:, 3]
        assert (tri[:64] >= 0).all() and (tri < 0).sum() > 50 and (want[tri >= 0][:, 2] > 0).sum() > 300
    finally:
        th.close()


def test_clearance_after_refit(psm, ctx, scenes):
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
        q = (centre[:, None, :] + rng.uniform(-0.05, 0.05, (1024, 3, 3)) * (bhi - blo)).astype(F)
        want = check_clearance(psm, th, moved, q)
        tri = want.view(np.int32)[:, 3]
        assert (tri >= 0).all() and np.isin(tri, k).any() and (want[:, 2] > 0).sum() > 200
    finally:
        th.close()


def test_clearance_torch_tensors_on_a_side_stream(psm, ctx, scenes):
    if torch is None:
        pytest.skip("torch is not installed")
    sc = scenes.cornell()
    tris = sc["tris"].reshape(-1, 3, 3)
    rng = np.random.RandomState(6)
    blo, bhi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    q = (rng.uniform(blo, bhi, (4099, 1, 3)) + rng.uniform(-0.05, 0.05, (4099, 3, 3)) * (bhi - blo)).astype(F)
    rmax = rng.choice(F([np.inf, 0.05, 0.2]), 4099) * F((bhi - blo).max())
    th = _hier(psm, ctx, tris)
    try:
        hits, flag, flag1 = th.triClosest(q, rmax), th.triWithin(q, rmax), th.triWithin(q, 0.01)
        assert flag.any() and not flag.all() and (hits.dist[flag] > 0).any()
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            tq = torch.from_numpy(q).to(dev, non_blocking=True)
            tr = torch.from_numpy(rmax).to(dev, non_blocking=True)
            ghits, gflag, gflag1 = th.triClosest(tq, tr), th.triWithin(tq.reshape(-1, 9), tr), th.triWithin(tq, 0.01)
            pm, pq = ghits.points(torch.from_numpy(np.ascontiguousarray(tris, F)).to(dev), tq)
            bufs = [x.cpu() for x in (ghits.buffer, gflag, gflag1, ghits.tri, pm, pq)]   # (on the side stream: in order)
        assert ghits.buffer.device == dev and ghits.buffer.shape == (4099, 8) and gflag.dtype == torch.bool and ghits.tri.dtype == torch.int32
        _same_bits(bufs[0].numpy(), hits.buffer, "torch triClosest")
        _same_bits(bufs[1].numpy(), flag, "torch triWithin")
        _same_bits(bufs[2].numpy(), flag1, "torch triWithin, a scalar radius")
        _same_bits(bufs[3].numpy(), hits.tri, "torch triClosest tri")
        npm, npq = hits.points(np.ascontiguousarray(tris, F), q)
        found = hits.tri >= 0
        assert np.array_equal(bufs[4].numpy()[found], npm[found]) and np.array_equal(bufs[5].numpy()[found], npq[found])
        assert np.isnan(npm[~found]).all() and np.isnan(bufs[4].numpy()[~found]).all()
        apart = found & (hits.dist > 0)                 # (at dist == 0 the points are where the boundaries come closest)
        gap = np.linalg.norm(npm[apart].astype(np.float64) - npq[apart], axis=1)
        assert apart.sum() > 1000 and np.abs(gap - hits.dist[apart]).max() <= 1e-5 * (bhi - blo).max()
    finally:
        th.close()


def test_clearance_refusals_launch_nothing(psm, ctx):
    """a call before the build, NULL and misaligned pointers are refused on the host: the outputs keep what they held"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(4)
    th.loadTriangles(tri.reshape(1, 9))
    n = 4
    hin, hout, hflag = ctx.buf_alloc(48 * n + 16), ctx.buf_alloc(32 * n + 32), ctx.buf_alloc(n + 16)
    try:
        recs = np.zeros((n, 12), F)
        recs[:] = [0, 0, -2, np.inf, 2, 0, 2, 0, 2, 1, 2, 0]              # a triangle through the stored one, no limit
        recs[1:, 0] = [-1, -2, -3]                                       # ... and moved off it along x
        recs[1:, 4] -= [1, 2, 3]
        recs[1:, 8] -= [1, 2, 3]
        ctx.buf_upload(hin, recs)
        ctx.buf_upload(hout, np.full(8 * n + 8, 7, F))
        ctx.buf_upload(hflag, np.full(n + 16, 77, np.uint8))
        pin, pout, pflag = (ctypes.c_void_p(ctx.buf_ptr(h)[0]) for h in (hin, hout, hflag))
        size = ctypes.c_size_t(n)

        def call(fn, p_out, p_in=pin, count=size):
            return fn(th._h, p_in, count, p_out)
        for fn, out in ((lib.psm_bvh_tri_closest_dev, pout), (lib.psm_bvh_tri_within_dev, pflag)):
            assert call(fn, out) == -5                                   # before the build: PSM_ERR_STATE
            assert b"clearance query before build" in lib.psm_last_error(ctx._h)
            assert call(fn, out, count=ctypes.c_size_t(0)) == 0          # n = 0 is answered first, as for every query
        th.build()
        for fn, out in ((lib.psm_bvh_tri_closest_dev, pout), (lib.psm_bvh_tri_within_dev, pflag)):
            assert call(fn, None) == -1 and b"NULL pointer" in lib.psm_last_error(ctx._h)
            assert call(fn, out, p_in=None) == -1
            assert call(fn, out, p_in=ctypes.c_void_p(pin.value + 8)) == -1 and b"not 16-byte aligned" in lib.psm_last_error(ctx._h)
        assert call(lib.psm_bvh_tri_closest_dev, ctypes.c_void_p(pout.value + 8)) == -1
        assert b"psm_bvh_tri_closest_dev: triangles or hits not 16-byte aligned" in lib.psm_last_error(ctx._h)
        ctx.sync()
        assert (ctx.buf_download(hout, F, 8 * n + 8) == 7).all() and (ctx.buf_download(hflag, np.uint8, n + 16) == 77).all()
        assert call(lib.psm_bvh_tri_closest_dev, pout) == 0 and call(lib.psm_bvh_tri_within_dev, pflag) == 0   # the same buffers are fine
        ctx.sync()
        got = ctx.buf_download(hout, F, 8 * n + 8)
        want, _ = TD.query(tri, [0], recs.reshape(n, 3, 4)[:, :, :3], recs[:, 3])
        _same_bits(got[:8 * n].reshape(n, 8), want, "the C ABI's records")
        assert (got[8 * n:] == 7).all() and want[0, 2] == 0 and (want[1:, 2] > 0).all()
        flags = ctx.buf_download(hflag, np.uint8, n + 16)
        assert (flags[:n] == 1).all() and (flags[n:] == 77).all()
    finally:
        for h in (hin, hout, hflag):
            ctx.buf_free(h)
        th.close()
