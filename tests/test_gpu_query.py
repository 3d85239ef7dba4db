"""The ray queries on the GPU (psm_bvh_intersect_dev / psm_bvh_occluded_dev, query.hip; TriangleHierarchy.intersect / occluded).
The yardstick is tests/query_model.py: the unclamped triangle test over the hierarchy's leaves (PSM_BVH_LEAF_TRI), the window
tmin <= t <= tmax, closest = smallest t then lowest id. Every comparison is bit for bit on every ray unless a test says otherwise."""
import ctypes
import importlib

import numpy as np
import pytest

import query_model as Q
from test_gpu_fuzz import fuzz_case

try:   # (imported before the library loads its HIP runtime: torch's wheel carries a runtime of its own, which finds no device when
    import torch   # it comes second into a process)
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32


def _hier(psm, ctx, tris):
    tris = np.ascontiguousarray(tris, F).reshape(-1, 9)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(max(tris.shape[0], 1))
    th.loadTriangles(tris)
    th.build()
    return th


def _leaves(psm, th):
    return th.download(psm.BVH_LEAF_TRI, np.int32, th.info().leaf_count)


def _check(psm, th, tris, o, d, tmin=0.0, tmax=np.inf):
    """closest and any hit equal the model; occluded with tmax = the closest t (where one was found) is exactly `found`"""
    o = np.ascontiguousarray(o, F).reshape(-1, 3)
    d = np.ascontiguousarray(d, F).reshape(-1, 3)
    n = o.shape[0]
    lo = np.broadcast_to(np.asarray(tmin, F), (n,)).copy()
    hi = np.broadcast_to(np.asarray(tmax, F), (n,)).copy()
    got = th.intersect(o, d, lo, hi)
    occ = th.occluded(o, d, lo, hi)
    exp, anyh = Q.query(tris, _leaves(psm, th), o, d, lo, hi)
    bad = np.nonzero((got.buffer.view(np.uint32) != exp.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:4], got.buffer[bad[:4]], exp[bad[:4]], o[bad[:4]], d[bad[:4]])
    assert np.array_equal(occ, anyh), np.nonzero(occ != anyh)[0][:8]
    found = got.tri >= 0
    assert np.array_equal(found, anyh)
    occ2 = th.occluded(o, d, lo, np.where(found, got.t, hi))
    assert np.array_equal(occ2, found)
    return got, exp


def _camera_rays(oracle, scenes, sc, w, h, time=7):
    cam = scenes.camera_matrices(sc["eye"], sc["view"], w, h)
    rays, *_ = oracle.camera(oracle.make_cfg(w, h), cam[0], cam[1], time)
    return rays["origin"].copy(), rays["direct"].copy()


def _random_rays(rng, tris, n, outside=False):
    p = tris.reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    ext = hi - lo
    o = rng.uniform(lo, hi, (n, 3)).astype(F)
    if outside:   # from a shell around the box, pointing at a point inside it
        u = rng.normal(size=(n, 3)).astype(F)
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        o = ((lo + hi) * F(0.5) + u * ext.max() * F(1.5)).astype(F)
        d = (rng.uniform(lo, hi, (n, 3)) - o).astype(F)
    else:
        d = rng.normal(size=(n, 3)).astype(F)
    return o, d


def _windows(rng, exact_t, n):
    """random per-ray windows: plain, tmin = tmax = an exact hit t, tmin > tmax, negative tmin, NaN"""
    tmin = rng.uniform(-2, 2, n).astype(F)
    tmax = (tmin + rng.uniform(0, 5, n)).astype(F)
    k = n // 5
    hit = np.isfinite(exact_t)
    idx = np.nonzero(hit)[0][:k]
    tmin[idx] = exact_t[idx]
    tmax[idx] = exact_t[idx]
    tmin[k:2 * k], tmax[k:2 * k] = tmax[k:2 * k] + F(1), tmin[k:2 * k]              # empty windows
    tmin[2 * k:3 * k] = -np.inf
    tmax[3 * k:3 * k + 3] = np.inf
    tmin[3 * k + 3] = np.nan
    tmax[3 * k + 4] = np.nan
    return tmin, tmax


def _nonfinite(o, d):
    o, d = o.copy(), d.copy()
    d[0] = [np.nan, 0, 1]
    d[1] = [np.inf, 0, 0]
    d[2] = 0
    o[3] = [np.nan, 0, 0]
    o[4] = [-np.inf, 0, 0]
    d[5] = [1e-30, 0, 0]
    d[6] = [0, -0.0, 1]
    d[7] = [-0.0, 1, -0.0]
    return o, d


def _scene_cases(psm, ctx, oracle, scenes, tris, o, d, seed):
    th = _hier(psm, ctx, tris)
    try:
        rng = np.random.RandomState(seed)
        got, _ = _check(psm, th, tris, o, d)
        _check(psm, th, tris, *_random_rays(rng, tris, 512))
        _check(psm, th, tris, *_random_rays(rng, tris, 512, outside=True))
        tmin, tmax = _windows(rng, got.t.copy(), o.shape[0])
        _check(psm, th, tris, o, d, tmin, tmax)
        _check(psm, th, tris, *_nonfinite(o[:64], d[:64]))
    finally:
        th.close()


def test_query_cornell(psm, ctx, oracle, scenes):
    sc = scenes.cornell()
    tris = sc["tris"].reshape(-1, 3, 3)
    o, d = _camera_rays(oracle, scenes, sc, 64, 48)
    _scene_cases(psm, ctx, oracle, scenes, tris, o, d, 1)


def test_query_sponza_like(psm, ctx, oracle, scenes):
    sc = scenes.sponza_like(30011)
    tris = sc["tris"].reshape(-1, 3, 3)
    o, d = _camera_rays(oracle, scenes, sc, 48, 27)
    _scene_cases(psm, ctx, oracle, scenes, tris, o, d, 2)


@pytest.mark.parametrize("seed", range(8))
def test_query_fuzz_soups(psm, ctx, seed):
    tris, o, d, tags = fuzz_case(seed)
    o, d = o[:256], d[:256]
    th = _hier(psm, ctx, tris)
    try:
        rng = np.random.RandomState(seed)
        got, _ = _check(psm, th, tris, o, d)
        _check(psm, th, tris, *_random_rays(rng, tris, 256, outside=True))
        tmin, tmax = _windows(rng, got.t.copy(), o.shape[0])
        _check(psm, th, tris, o, d, tmin, tmax)
    finally:
        th.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 100003])
def test_query_batch_sizes(psm, ctx, scenes, n):
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3)
    th = _hier(psm, ctx, tris)
    try:
        o, d = _random_rays(np.random.RandomState(n), tris, n)
        got, _ = _check(psm, th, tris, o, d)
        assert len(got) == n
    finally:
        th.close()


def test_query_deep_fixture_pipeline_drops(psm, ctx):
    """The pipeline's 16-entry stack drops subtrees on this hierarchy; the query answers exactly."""
    tris, o, d = Q.deep_fixture()
    th = _hier(psm, ctx, tris)
    try:
        _check(psm, th, tris, o, d)
        n = o.shape[0]
        rays = np.zeros(n, psm.RAY_DT)
        rays["origin"], rays["direct"], rays["color"] = o, d, 1.0
        rays["bitfield"] = 1 | (3 << 8)
        rays["texel"] = np.arange(n)
        rt = psm.Pipeline(ctx)
        rt.resizeBuffers(16, 16)
        rt.upload_rays(rays)
        ctx.stats_enable(False, True)
        ctx.stats_reset()
        rt.intersection(th)
        st = ctx.stats()
        ctx.stats_enable(False, False)
        rt.close()
        assert st.stack_drops > 0
    finally:
        th.close()


def _lessF_inf_limit():
    """the largest t with lessF(t, INF) = (INF - t) >= PZERO in float arithmetic"""
    t = F(Q.INF - Q.PZERO)
    while not (F(Q.INF - t) >= Q.PZERO):
        t = np.nextafter(t, F(-np.inf))
    while F(Q.INF - np.nextafter(t, F(np.inf))) >= Q.PZERO:
        t = np.nextafter(t, F(np.inf))
    return t


def test_query_agrees_with_pipeline_sponza(psm, ctx, scenes, oracle):
    """Full sponza_like, 256 x 144 camera rays, window = the pipeline's t acceptance (greaterEqualF(t, 0), lessF(t, INF)): where the
    pipeline's chain has one entry, the ray had no stack drop and the head's |det| >= 1e-6, (t, u, v, tri) is the chain head bit for
    bit. A ray whose chain is empty misses -- unless its stack dropped a subtree or the query's hit has |det| < 1e-6 (the clamp)."""
    sc = scenes.sponza_like()
    tris = np.ascontiguousarray(sc["tris"], F).reshape(-1, 3, 3)
    th = _hier(psm, ctx, tris)
    rt = psm.Pipeline(ctx, seed=7)
    try:
        w, h = 256, 144
        rt.resizeBuffers(w, h)
        rt.resize(w, h)
        rt.camera(sc["eye"], sc["view"])
        rays = rt.download_rays()
        n = rays.shape[0]
        ctx.stats_enable(False, True)
        ctx.stats_reset()
        rt.intersection(th)
        st = ctx.stats()
        ctx.stats_enable(False, False)
        heads, counts = rt.download_hits(n)
        o, d = rays["origin"].copy(), rays["direct"].copy()
        tmin = np.nextafter(-Q.PZERO, F(np.inf))
        got = th.intersect(o, d, tmin, _lessF_inf_limit())
        dropped = np.zeros(n, bool)
        if st.stack_drops:
            ob = oracle.build_scene(tris)
            for i in range(n):
                _, _, c = oracle.traverse(ob["nodes"], tris, ob["M"], o[i:i + 1], d[i:i + 1], want_hits=False)
                dropped[i] = c.stack_drops > 0
        head = heads[:, 0]
        tri = np.where(counts > 0, head["tri"], -1)
        dn = Q.normalize3(d)

        def det_of(k):
            tk = tris[np.maximum(k, 0)]
            return np.abs(Q.dot3(tk[:, 1] - tk[:, 0], Q.cross3(dn, tk[:, 2] - tk[:, 0])))

        one = (counts == 1) & ~dropped & (det_of(tri) >= F(1e-6))
        assert one.sum() > n // 4
        for name, a, b in (("t", got.t, head["t"]), ("u", got.u, head["u"]), ("v", got.v, head["v"])):
            bad = np.nonzero(one & (a.view(np.uint32) != np.ascontiguousarray(b, F).view(np.uint32)))[0]
            assert bad.size == 0, (name, bad[:8])
        assert np.array_equal(got.tri[one], tri[one])
        empty = counts == 0
        explained = dropped | (det_of(got.tri) < F(1e-6))
        assert not (empty & (got.tri >= 0) & ~explained).any()
    finally:
        rt.close()
        th.close()


def test_query_tiny_hierarchies(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    rng = np.random.RandomState(4)
    o = rng.uniform(-0.5, 0.5, (200, 3)).astype(F)
    d = (np.float32([2, 0, 0]) + rng.uniform(-1, 1, (200, 3)).astype(F) - o).astype(F)
    degenerate = np.repeat(tri[:, :1], 3, axis=1)                    # three equal vertices: the build keeps no leaf
    for tris, leaves in ((np.concatenate([degenerate] * 4), 0), (np.concatenate([degenerate, tri, degenerate]), 1),
                         (np.concatenate([tri, degenerate, tri + F([0.5, 0, 0])]), 2)):
        th = _hier(psm, ctx, tris)
        try:
            assert th.info().leaf_count == leaves
            got, _ = _check(psm, th, tris, o, d)
            assert (got.tri >= 0).any() == (leaves > 0)
        finally:
            th.close()


def test_query_before_build_is_a_state_error(psm, ctx):
    th = psm.TriangleHierarchy(ctx)
    th.allocate(4)
    th.loadTriangles(np.eye(3, dtype=F).reshape(1, 9))
    try:
        lib = psm.lib()
        h = ctx.buf_alloc(64)
        p = ctx.buf_ptr(h)[0]
        assert lib.psm_bvh_intersect_dev(th._h, ctypes.c_void_p(p), ctypes.c_size_t(1), ctypes.c_void_p(p)) == -5
        assert lib.psm_bvh_occluded_dev(th._h, ctypes.c_void_p(p), ctypes.c_size_t(1), ctypes.c_void_p(p)) == -5
        assert lib.psm_bvh_intersect_dev(th._h, ctypes.c_void_p(p), ctypes.c_size_t(0), ctypes.c_void_p(p)) == 0
        assert lib.psm_bvh_intersect_dev(th._h, ctypes.c_void_p(p + 4), ctypes.c_size_t(1), ctypes.c_void_p(p)) == -1
        assert lib.psm_bvh_occluded_dev(th._h, None, ctypes.c_size_t(1), ctypes.c_void_p(p)) == -1
        ctx.buf_free(h)
    finally:
        th.close()


def test_query_after_refit(psm, ctx, oracle, scenes):
    sc = scenes.cornell()
    tris = sc["tris"].reshape(-1, 3, 3).copy()
    th = _hier(psm, ctx, tris)
    try:
        lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
        moved = tris.copy()
        rng = np.random.RandomState(9)
        k = rng.choice(tris.shape[0], 8, replace=False)
        c = moved[k].mean(axis=1, keepdims=True)
        moved[k] = (c + (moved[k] - c) * F(0.5) + rng.uniform(-0.3, 0.3, (8, 1, 3)).astype(F)).astype(F)
        moved = np.clip(moved, lo, hi).astype(F)                    # within the build's bounds
        th.clearTribuffer()
        th.loadTriangles(moved.reshape(-1, 9))
        th.refit()
        o, d = _camera_rays(oracle, scenes, sc, 64, 48)
        got, _ = _check(psm, th, moved, o, d)
        assert np.isin(got.tri, k).any()
    finally:
        th.close()


def test_query_torch_tensors(psm, ctx, scenes):
    if torch is None:
        pytest.skip("torch is not installed")
    sc = scenes.sponza_like(30011)
    tris = sc["tris"].reshape(-1, 3, 3)
    rng = np.random.RandomState(6)
    o, d = _random_rays(rng, tris, 4099)
    tmin = rng.uniform(-1, 0.5, o.shape[0]).astype(F)
    own = psm.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        for c in (own, ctx):     # a context on torch's current stream, and one with its own stream
            th = _hier(psm, c, tris)
            try:
                ref = th.intersect(o, d, tmin)
                ref_occ = th.occluded(o, d, tmin)
                dev = torch.device("cuda", 0)
                to, td, tt = (torch.from_numpy(x).to(dev) for x in (o, d, tmin))
                got = th.intersect(to, td, tt)
                occ = th.occluded(to, td, tt)
                assert got.buffer.device == dev and got.buffer.shape == (o.shape[0], 4) and occ.dtype == torch.bool
                assert np.array_equal(got.buffer.cpu().numpy().view(np.uint32), ref.buffer.view(np.uint32))
                assert np.array_equal(got.tri.cpu().numpy(), ref.tri)
                assert np.array_equal(occ.cpu().numpy(), ref_occ)
            finally:
                th.close()
    finally:
        own.close()


def test_query_16m_rays(psm, ctx, scenes):
    sc = scenes.sponza_like(30011)
    tris = sc["tris"].reshape(-1, 3, 3)
    th = _hier(psm, ctx, tris)
    try:
        n = 1 << 24
        rng = np.random.RandomState(16)
        o, d = _random_rays(rng, tris, n)
        got = th.intersect(o, d)
        occ = th.occluded(o, d)
        assert np.array_equal(occ, got.tri >= 0)
        s = rng.choice(n, 4096, replace=False)
        exp, _ = Q.query(tris, _leaves(psm, th), o[s], d[s])
        assert np.array_equal(got.buffer[s].view(np.uint32), exp.view(np.uint32))
    finally:
        th.close()
