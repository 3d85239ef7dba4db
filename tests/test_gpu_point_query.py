"""The point queries on the GPU (psm_bvh_closest_point_dev / psm_bvh_within_dev, query.hip; TriangleHierarchy.closestPoint /
within). The yardstick is tests/point_query_model.py: Ericson's closest point with its guards over the hierarchy's leaves
(PSM_BVH_LEAF_TRI), dist <= rmax, closest = smallest d2 then lowest id. Every comparison is bit for bit on every point unless a
test says otherwise."""
import ctypes

import numpy as np
import pytest

import point_query_model as PQ
import query_model as Q
from test_gpu_fuzz import fuzz_case

try:   # (imported before the library loads its HIP runtime, as tests/test_gpu_query.py)
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32


def _hier(psm, ctx, tris, opt=None):
    tris = np.ascontiguousarray(tris, F).reshape(-1, 9)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(max(tris.shape[0], 1))
    th.loadTriangles(tris)
    th.build(opt)
    return th


def _leaves(psm, th):
    return th.download(psm.BVH_LEAF_TRI, np.int32, th.info().leaf_count)


def _check(psm, th, tris, p, rmax=np.inf):
    """closest point and within equal the model; within is exactly `found`"""
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    rm = np.broadcast_to(np.asarray(rmax, F), (p.shape[0],)).copy()
    got = th.closestPoint(p, rm)
    win = th.within(p, rm)
    exp, ew = PQ.query(tris, _leaves(psm, th), p, rm)
    bad = np.nonzero((got.buffer.view(np.uint32) != exp.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:4], got.buffer[bad[:4]], exp[bad[:4]], p[bad[:4]], rm[bad[:4]])
    assert np.array_equal(win, ew), np.nonzero(win != ew)[0][:8]
    assert np.array_equal(got.tri >= 0, ew)
    return got


def _points(rng, tris, n):
    """surface samples, near the surface (noise of 1 % of the diagonal), far away, on vertices, inside the box; NaN / inf"""
    t = np.asarray(tris, F).reshape(-1, 3, 3)
    lo, hi = t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0)
    diag = float(np.linalg.norm(hi - lo)) or 1.0
    k = n // 5
    pick = t[rng.randint(0, t.shape[0], 2 * k)]
    w = rng.dirichlet([1, 1, 1], 2 * k).astype(F)
    surf = np.einsum("ij,ijk->ik", w, pick).astype(F)
    near = surf[k:] + rng.normal(0, 0.01 * diag, (k, 3)).astype(F)
    far = ((lo + hi) / 2 + rng.normal(0, 2 * diag, (k, 3))).astype(F)
    vert = t.reshape(-1, 3)[rng.randint(0, 3 * t.shape[0], k)]
    box = rng.uniform(lo, hi, (n - 4 * k, 3)).astype(F)
    p = np.concatenate([surf[:k], near, far, vert, box]).astype(F)
    p[-1] = [np.nan, 0, 0]
    p[-2] = [0, np.inf, 0]
    p[-3] = [0, 0, -np.inf]
    return p


def _radii(rng, n, scale):
    """per-point rmax: plain, zero, -0, negative, NaN, +inf"""
    r = rng.uniform(0, scale, n).astype(F)
    k = n // 8
    r[:k] = np.inf
    r[k:k + 4] = 0
    r[k + 4] = -0.0
    r[k + 5:k + 8] = -1
    r[k + 8:k + 10] = np.nan
    return r


def _with_degenerates(rng, tris):
    """a few triangles made collinear or zero-area (two equal vertices; all three equal: not a leaf)"""
    t = np.array(tris, F).reshape(-1, 3, 3)
    if t.shape[0] < 8:
        return t
    idx = rng.choice(t.shape[0], max(4, t.shape[0] // 16), replace=False)
    for j, i in enumerate(idx):
        if j % 3 == 0:
            t[i, 2] = t[i, 0] + F(0.5) * (t[i, 1] - t[i, 0])
        elif j % 3 == 1:
            t[i, 1] = t[i, 0]
        else:
            t[i, 1] = t[i, 2] = t[i, 0]
    return t


def _scene_cases(psm, ctx, tris, seed, n=768):
    th = _hier(psm, ctx, tris)
    try:
        rng = np.random.RandomState(seed)
        p = _points(rng, tris, n)
        got = _check(psm, th, tris, p)
        diag = float(np.linalg.norm(tris.reshape(-1, 3).max(0) - tris.reshape(-1, 3).min(0)))
        _check(psm, th, tris, p, _radii(rng, n, 0.05 * diag))
        # rmax = the model's own distance is found, the float below it is not
        ok = got.tri >= 0
        r = np.where(ok, got.t, F(1)).astype(F)
        again = _check(psm, th, tris, p, r)
        assert np.array_equal(again.tri[ok], got.tri[ok])
        below = _check(psm, th, tris, p, np.where(ok, np.nextafter(r, F(0)), F(1)).astype(F))
        assert (below.tri[ok & (got.t > 0)] == -1).all()
    finally:
        th.close()


def test_point_query_cornell(psm, ctx, scenes):
    _scene_cases(psm, ctx, scenes.cornell()["tris"].reshape(-1, 3, 3), 1)


def test_point_query_sponza_like(psm, ctx, scenes):
    _scene_cases(psm, ctx, scenes.sponza_like(30011)["tris"].reshape(-1, 3, 3), 2, n=512)


@pytest.mark.parametrize("seed", range(8))
def test_point_query_fuzz_soups(psm, ctx, seed):
    tris, _, _, _ = fuzz_case(seed)
    if seed % 2 == 0:
        tris = _with_degenerates(np.random.RandomState(seed), tris)
    _scene_cases(psm, ctx, tris, 100 + seed, n=256)


def test_point_query_ties_across_subtrees(psm, ctx):
    """A coplanar grid, triangles in shuffled order: points above shared vertices and edge midpoints have a bit-equal d2 on
    several triangles, usually in different subtrees; the lowest id wins."""
    rng = np.random.RandomState(7)
    g = 48
    i, j = np.meshgrid(np.arange(g, dtype=F), np.arange(g, dtype=F), indexing="ij")
    a = np.stack([i, j, np.zeros_like(i)], -1).reshape(-1, 3)
    b, c, d = a + F([1, 0, 0]), a + F([0, 1, 0]), a + F([1, 1, 0])
    tris = np.concatenate([np.stack([a, b, d], 1), np.stack([a, d, c], 1)]).astype(F)
    tris = tris[rng.permutation(tris.shape[0])]
    th = _hier(psm, ctx, tris)
    try:
        vi = rng.randint(1, g, (600, 2)).astype(F)
        p = np.concatenate([np.c_[vi, np.full(600, 1.0, F)],                            # above interior vertices
                            np.c_[vi[:, 0] + F(0.5), vi[:, 1], np.full(600, 0.5, F)],  # above edge midpoints
                            np.c_[vi, np.zeros(600, F)]]).astype(F)                     # on the vertices
        got = _check(psm, th, tris, p)
        exp_d2 = PQ.closest_on_tris(*(x[None] for x in PQ._split(tris)), p[:, None, :])[2]
        ties = (exp_d2 == exp_d2.min(axis=1, keepdims=True)).sum(axis=1)
        assert (ties > 1).mean() > 0.9
        assert np.array_equal(got.tri, np.argmax(exp_d2 == exp_d2.min(axis=1, keepdims=True), axis=1))
    finally:
        th.close()


ROT_SCALE = np.array([[np.cos(0.3), 0, np.sin(0.3), 0.5], [0, 1.3, 0, -1.0], [-np.sin(0.3), 0, np.cos(0.3), 2.0], [0, 0, 0, 1]])
SHEAR = np.array([[1, 0.6, 0, 0.2], [0, 1, -0.4, 0], [0.3, 0, 1, -1], [0, 0, 0, 1]])


@pytest.mark.parametrize("opt", [None, ROT_SCALE, SHEAR], ids=["identity", "rotate_scale", "shear"])
def test_point_query_optimisation_matrix(psm, ctx, scenes, opt):
    tris = scenes.sponza_like(30011)["tris"].reshape(-1, 3, 3)
    th = _hier(psm, ctx, tris, opt)
    try:
        rng = np.random.RandomState(11)
        p = _points(rng, tris, 512)
        _check(psm, th, tris, p)
        _check(psm, th, tris, p, _radii(rng, 512, 1.0))
    finally:
        th.close()


def test_point_query_deep_fixture(psm, ctx):
    """points near the origin of the deep fixture: the walk holds more than 16 pending subtrees, the rest spill"""
    tris, _, _ = Q.deep_fixture()
    th = _hier(psm, ctx, tris)
    try:
        rng = np.random.RandomState(12)
        p = np.concatenate([rng.normal(0, 1e-3, (256, 3)), np.c_[rng.uniform(-0.5, 1.2, 256), rng.normal(0, 0.05, (256, 2))]])
        _check(psm, th, tris, p.astype(F))
    finally:
        th.close()


def test_point_query_tiny_hierarchies(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    rng = np.random.RandomState(4)
    p = rng.uniform(-1, 3, (200, 3)).astype(F)
    degenerate = np.repeat(tri[:, :1], 3, axis=1)
    for tris, leaves in ((np.concatenate([degenerate] * 4), 0), (np.concatenate([degenerate, tri, degenerate]), 1),
                         (np.concatenate([tri, degenerate, tri + F([0.5, 0, 0])]), 2)):
        th = _hier(psm, ctx, tris)
        try:
            assert th.info().leaf_count == leaves
            got = _check(psm, th, tris, p)
            _check(psm, th, tris, p, _radii(rng, 200, 2.0))
            assert (got.tri >= 0).any() == (leaves > 0)
        finally:
            th.close()


def test_point_query_before_build_is_a_state_error(psm, ctx):
    th = psm.TriangleHierarchy(ctx)
    th.allocate(4)
    th.loadTriangles(np.eye(3, dtype=F).reshape(1, 9))
    try:
        lib = psm.lib()
        h = ctx.buf_alloc(64)
        p = ctx.buf_ptr(h)[0]
        assert lib.psm_bvh_closest_point_dev(th._h, ctypes.c_void_p(p), ctypes.c_size_t(1), ctypes.c_void_p(p)) == -5
        assert lib.psm_bvh_within_dev(th._h, ctypes.c_void_p(p), ctypes.c_size_t(1), ctypes.c_void_p(p)) == -5
        assert lib.psm_bvh_closest_point_dev(th._h, ctypes.c_void_p(p), ctypes.c_size_t(0), ctypes.c_void_p(p)) == 0
        assert lib.psm_bvh_closest_point_dev(th._h, ctypes.c_void_p(p + 4), ctypes.c_size_t(1), ctypes.c_void_p(p)) == -1
        assert lib.psm_bvh_closest_point_dev(th._h, ctypes.c_void_p(p), ctypes.c_size_t(1), ctypes.c_void_p(p + 4)) == -1
        assert lib.psm_bvh_within_dev(th._h, None, ctypes.c_size_t(1), ctypes.c_void_p(p)) == -1
        assert lib.psm_bvh_within_dev(th._h, ctypes.c_void_p(p), ctypes.c_size_t(1), None) == -1
        assert lib.psm_last_error(ctx._h).decode() == "psm_bvh_within_dev: NULL pointer"
        # the ray queries keep their own texts beside the point queries'
        assert lib.psm_bvh_intersect_dev(th._h, ctypes.c_void_p(p + 4), ctypes.c_size_t(1), ctypes.c_void_p(p)) == -1
        assert lib.psm_last_error(ctx._h).decode() == "psm_bvh_intersect_dev: rays or hits not 16-byte aligned"
        assert lib.psm_bvh_occluded_dev(th._h, ctypes.c_void_p(p + 4), ctypes.c_size_t(1), ctypes.c_void_p(p)) == -1
        assert lib.psm_last_error(ctx._h).decode() == "psm_bvh_occluded_dev: rays not 16-byte aligned"
        assert lib.psm_bvh_within_dev(th._h, ctypes.c_void_p(p + 4), ctypes.c_size_t(1), ctypes.c_void_p(p)) == -1
        assert lib.psm_last_error(ctx._h).decode() == "psm_bvh_within_dev: points not 16-byte aligned"
        ctx.buf_free(h)
    finally:
        th.close()


def test_point_query_after_refit(psm, ctx, scenes):
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3).copy()
    th = _hier(psm, ctx, tris)
    try:
        lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
        moved = tris.copy()
        rng = np.random.RandomState(9)
        k = rng.choice(tris.shape[0], 8, replace=False)
        c = moved[k].mean(axis=1, keepdims=True)
        moved[k] = (c + (moved[k] - c) * F(0.5) + rng.uniform(-0.3, 0.3, (8, 1, 3)).astype(F)).astype(F)
        moved = np.clip(moved, lo, hi).astype(F)
        th.clearTribuffer()
        th.loadTriangles(moved.reshape(-1, 9))
        th.refit()
        p = np.concatenate([_points(rng, moved, 400), moved[k].mean(axis=1)]).astype(F)
        got = _check(psm, th, moved, p)
        assert np.isin(got.tri, k).any()
    finally:
        th.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 100003])
def test_point_query_batch_sizes(psm, ctx, scenes, n):
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3)
    th = _hier(psm, ctx, tris)
    try:
        p = np.random.RandomState(n).uniform(-1, 1, (n, 3)).astype(F) * F(600)
        got = _check(psm, th, tris, p, F(100))
        assert len(got) == n
    finally:
        th.close()


def test_point_query_within_is_closest_found(psm, ctx, scenes):
    tris = scenes.sponza_like(30011)["tris"].reshape(-1, 3, 3)
    th = _hier(psm, ctx, tris)
    try:
        rng = np.random.RandomState(13)
        p = _points(rng, tris, 200000)
        for r in (F(0), F(0.01), F(0.3), _radii(rng, p.shape[0], 2.0)):
            assert np.array_equal(th.within(p, r), th.closestPoint(p, rmax=r).tri >= 0)
    finally:
        th.close()


def test_point_query_torch_tensors(psm, ctx, scenes):
    if torch is None:
        pytest.skip("torch is not installed")
    tris = scenes.sponza_like(30011)["tris"].reshape(-1, 3, 3)
    rng = np.random.RandomState(6)
    p = _points(rng, tris, 4099)
    r = _radii(rng, p.shape[0], 1.0)
    own = psm.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        for c in (own, ctx):     # a context on torch's current stream, and one with its own stream
            th = _hier(psm, c, tris)
            try:
                ref = th.closestPoint(p, r)
                ref_w = th.within(p, r)
                dev = torch.device("cuda", 0)
                tp, tr = torch.from_numpy(p).to(dev), torch.from_numpy(r).to(dev)
                got = th.closestPoint(tp, tr)
                w = th.within(tp, tr)
                w_scalar = th.within(tp, 0.5)
                assert got.buffer.device == dev and got.buffer.shape == (p.shape[0], 4) and w.dtype == torch.bool
                assert np.array_equal(got.buffer.cpu().numpy().view(np.uint32), ref.buffer.view(np.uint32))
                assert np.array_equal(w.cpu().numpy(), ref_w)
                assert np.array_equal(w_scalar.cpu().numpy(), th.within(p, 0.5))
            finally:
                th.close()
    finally:
        own.close()


def test_point_and_ray_queries_interleaved(psm, ctx, scenes):
    """ray and point queries on one context, one after the other without a synchronisation between them: they share the
    stack's spill area; every result equals its model"""
    tris, _, _ = Q.deep_fixture()
    th = _hier(psm, ctx, tris)
    try:
        _, o, d = Q.deep_fixture(rays=512)
        rng = np.random.RandomState(14)
        p = rng.normal(0, 1e-3, (512, 3)).astype(F)
        leaves = _leaves(psm, th)
        rays = np.zeros((512, 8), F)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 0, d, np.inf
        pts = np.zeros((512, 4), F)
        pts[:, 0:3], pts[:, 3] = p, np.inf
        hr, hp, h1, h2, h3 = (ctx.buf_alloc(n) for n in (rays.nbytes, pts.nbytes, 16 * 512, 16 * 512, 512))
        ctx.buf_upload(hr, rays)
        ctx.buf_upload(hp, pts)
        lib = psm.lib()
        ptr = [ctypes.c_void_p(ctx.buf_ptr(h)[0]) for h in (hr, hp, h1, h2, h3)]
        n = ctypes.c_size_t(512)
        for _ in range(3):
            assert lib.psm_bvh_intersect_dev(th._h, ptr[0], n, ptr[2]) == 0
            assert lib.psm_bvh_closest_point_dev(th._h, ptr[1], n, ptr[3]) == 0
            assert lib.psm_bvh_within_dev(th._h, ptr[1], n, ptr[4]) == 0
        ray_hits = ctx.buf_download(h1, F, 4 * 512).reshape(512, 4)
        pt_hits = ctx.buf_download(h2, F, 4 * 512).reshape(512, 4)
        win = ctx.buf_download(h3, np.uint8, 512)
        for h in (hr, hp, h1, h2, h3):
            ctx.buf_free(h)
        exp_r, _ = Q.query(tris, leaves, o, d)
        exp_p, exp_w = PQ.query(tris, leaves, p)
        assert np.array_equal(ray_hits.view(np.uint32), exp_r.view(np.uint32))
        assert np.array_equal(pt_hits.view(np.uint32), exp_p.view(np.uint32))
        assert np.array_equal(win.astype(bool), exp_w)
    finally:
        th.close()


def test_point_query_16m_points(psm, ctx, scenes):
    tris = scenes.sponza_like(30011)["tris"].reshape(-1, 3, 3)
    th = _hier(psm, ctx, tris)
    try:
        n = 1 << 24
        rng = np.random.RandomState(16)
        lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
        p = rng.uniform(lo, hi, (n, 3)).astype(F)
        got = th.closestPoint(p)
        assert (got.tri >= 0).all()
        r = F(0.05)
        win = th.within(p, r)
        assert np.array_equal(win, got.t <= r)
        s = rng.choice(n, 2048, replace=False)
        exp, _ = PQ.query(tris, _leaves(psm, th), p[s])
        assert np.array_equal(got.buffer[s].view(np.uint32), exp.view(np.uint32))
    finally:
        th.close()
