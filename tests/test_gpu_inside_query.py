"""The hit-count, inside / outside and signed-distance queries on the GPU (psm_bvh_count_hits_dev / psm_bvh_inside_dev /
psm_bvh_signed_distance_dev, query.hip; TriangleHierarchy.countHits / inside / signedDistance). The yardstick is
tests/inside_query_model.py over the hierarchy's leaves (PSM_BVH_LEAF_TRI). Every comparison is exact on every query: counts are
integers, votes booleans, and the signed hits are compared by their float bits."""
import ctypes
import functools

import numpy as np
import pytest

import inside_query_model as IQ
import query_model as Q
from test_gpu_fuzz import fuzz_case
from test_gpu_query import _camera_rays, _nonfinite, _random_rays, _windows

try:   # (imported before the library loads its HIP runtime, as tests/test_gpu_query.py)
    import torch
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


def _check_count(psm, th, tris, o, d, tmin=0.0, tmax=np.inf):
    """the count equals the model's, and count > 0 is occluded() of the same rays"""
    o = np.ascontiguousarray(o, F).reshape(-1, 3)
    d = np.ascontiguousarray(d, F).reshape(-1, 3)
    n = o.shape[0]
    lo = np.broadcast_to(np.asarray(tmin, F), (n,)).copy()
    hi = np.broadcast_to(np.asarray(tmax, F), (n,)).copy()
    got = th.countHits(o, d, lo, hi)
    exp = IQ.count(tris, _leaves(psm, th), o, d, lo, hi)
    assert got.dtype == np.uint32 and got.shape == (n,)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (bad.size, bad[:4], got[bad[:4]], exp[bad[:4]], o[bad[:4]], d[bad[:4]], lo[bad[:4]], hi[bad[:4]])
    assert np.array_equal(got > 0, th.occluded(o, d, lo, hi))
    return got


def _check_points(psm, th, tris, p, rmax=np.inf, samples=(1, 3, 5)):
    """inside and signedDistance equal the model for every sample count; the signed hits are closestPoint's but for t's sign"""
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    rm = np.broadcast_to(np.asarray(rmax, F), (p.shape[0],)).copy()
    leaves = _leaves(psm, th)
    par = IQ.parities(tris, leaves, p, max(samples))
    plain = th.closestPoint(p, rm)
    found = plain.tri >= 0
    out = {}
    for s in samples:
        exp_in = IQ.vote(par, s)
        got_in = th.inside(p, s)
        assert got_in.dtype == np.bool_ and np.array_equal(got_in, exp_in), (s, np.nonzero(got_in != exp_in)[0][:8])
        sd = th.signedDistance(p, rm, s)
        exp = plain.buffer.copy()
        exp.view(np.uint32)[found & exp_in, 2] |= np.uint32(0x80000000)
        bad = np.nonzero((sd.buffer.view(np.uint32) != exp.view(np.uint32)).any(axis=1))[0]
        assert bad.size == 0, (s, bad.size, bad[:4], sd.buffer[bad[:4]], exp[bad[:4]], p[bad[:4]], rm[bad[:4]])
        miss = sd.buffer[~found]
        assert np.isposinf(miss[:, 2]).all() and (miss.view(np.int32)[:, 3] == -1).all() and not miss[:, :2].any()
        out[s] = got_in
    # ... and the model's own statement of the signed distance (point_query_model's hits with the sign) on the first 2048
    s, k = samples[-1], min(p.shape[0], 2048)
    exp = IQ.signed_distance(tris, leaves, p[:k], rm[:k], s)
    assert np.array_equal(th.signedDistance(p[:k], rm[:k], s).buffer.view(np.uint32), exp.view(np.uint32))
    return out


def _scene_points(rng, tris, n):
    """uniform in the scene's box grown by a tenth, on the surface, at vertices; NaN / inf"""
    t = np.asarray(tris, F).reshape(-1, 3, 3)
    lo, hi = t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0)
    ext = hi - lo
    k = n // 4
    w = rng.dirichlet([1, 1, 1], k).astype(F)
    surf = np.einsum("ij,ijk->ik", w, t[rng.randint(0, t.shape[0], k)]).astype(F)
    vert = t.reshape(-1, 3)[rng.randint(0, 3 * t.shape[0], k)]
    box = rng.uniform(lo - 0.1 * ext, hi + 0.1 * ext, (n - 2 * k, 3)).astype(F)
    p = np.concatenate([surf, vert, box]).astype(F)
    p[-1] = [np.nan, 0, 0]
    p[-2] = [0, np.inf, 0]
    p[-3] = [0, 0, -np.inf]
    return p


def _count_cases(psm, ctx, tris, o, d, seed):
    th = _hier(psm, ctx, tris)
    try:
        rng = np.random.RandomState(seed)
        _check_count(psm, th, tris, o, d)
        _check_count(psm, th, tris, o, d, -np.inf, np.inf)
        _check_count(psm, th, tris, *_random_rays(rng, tris, 512))
        _check_count(psm, th, tris, *_random_rays(rng, tris, 512, outside=True))
        exact_t = th.intersect(o, d).t.copy()
        tmin, tmax = _windows(rng, exact_t, o.shape[0])
        _check_count(psm, th, tris, o, d, tmin, tmax)
        # a window shrunk to the closest hit's own t still holds it
        hit = np.isfinite(exact_t)
        assert (th.countHits(o[hit], d[hit], exact_t[hit], exact_t[hit]) >= 1).all()
        got = _check_count(psm, th, tris, *_nonfinite(o[:64], d[:64]))
        assert not got[:6].any()
    finally:
        th.close()


def test_count_cornell(psm, ctx, oracle, scenes):
    sc = scenes.cornell()
    o, d = _camera_rays(oracle, scenes, sc, 64, 48)
    _count_cases(psm, ctx, sc["tris"].reshape(-1, 3, 3), o, d, 1)


def test_count_sponza_like(psm, ctx, oracle, scenes):
    sc = scenes.sponza_like(30011)
    o, d = _camera_rays(oracle, scenes, sc, 48, 27)
    _count_cases(psm, ctx, sc["tris"].reshape(-1, 3, 3), o, d, 2)


@pytest.mark.parametrize("seed", range(8))
def test_count_fuzz_soups(psm, ctx, seed):
    tris, o, d, _ = fuzz_case(seed)
    _count_cases(psm, ctx, tris, o[:256], d[:256], 100 + seed)


def test_count_deep_fixture(psm, ctx):
    """deeper than the 16 stack entries kept in LDS: every crossing is still counted (the rays run through all the clusters)"""
    tris, o, d = Q.deep_fixture()
    th = _hier(psm, ctx, tris)
    try:
        got = _check_count(psm, th, tris, o, d)
        assert got.max() >= 8
        _check_count(psm, th, tris, o, d, 0.25, 1.0)
        rng = np.random.RandomState(12)
        _check_points(psm, th, tris, rng.normal(0, 1e-3, (256, 3)).astype(F), samples=(3,))
    finally:
        th.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 100003])
def test_inside_query_batch_sizes(psm, ctx, scenes, n):
    tris = scenes.cornell()["tris"].reshape(-1, 3, 3)
    th = _hier(psm, ctx, tris)
    try:
        rng = np.random.RandomState(n)
        o, d = _random_rays(rng, tris, n)
        got = _check_count(psm, th, tris, o, d)
        assert len(got) == n
        ins = _check_points(psm, th, tris, o, F(150), samples=(3,))
        assert len(ins[3]) == n and len(th.signedDistance(o, F(150))) == n
    finally:
        th.close()


def test_inside_query_tiny_hierarchies(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    rng = np.random.RandomState(4)
    o = rng.uniform(-0.5, 0.5, (200, 3)).astype(F)
    d = (np.float32([2, 0, 0]) + rng.uniform(-1, 1, (200, 3)).astype(F) - o).astype(F)
    p = np.concatenate([o, o + F([1.5, 0, 0])])
    degenerate = np.repeat(tri[:, :1], 3, axis=1)                    # three equal vertices: the build keeps no leaf
    for tris, leaves in ((np.concatenate([degenerate] * 4), 0), (np.concatenate([degenerate, tri, degenerate]), 1),
                         (np.concatenate([tri, degenerate, tri + F([0.5, 0, 0])]), 2)):
        th = _hier(psm, ctx, tris)
        try:
            assert th.info().leaf_count == leaves
            got = _check_count(psm, th, tris, o, d)
            assert got.max() <= leaves and (got.max() > 0) == (leaves > 0)
            _check_points(psm, th, tris, p)   # (an open surface: the model's answer, whatever it means)
        finally:
            th.close()


def test_inside_query_before_build_and_host_checks(psm, ctx):
    th = psm.TriangleHierarchy(ctx)
    th.allocate(4)
    th.loadTriangles(np.eye(3, dtype=F).reshape(1, 9))
    try:
        lib = psm.lib()
        h = ctx.buf_alloc(64)
        p = ctx.buf_ptr(h)[0]
        P, one, three = ctypes.c_void_p, ctypes.c_size_t(1), ctypes.c_uint32(3)
        assert lib.psm_bvh_count_hits_dev(th._h, P(p), one, P(p)) == -5
        assert lib.psm_last_error(ctx._h).decode() == "ray query before build"
        assert lib.psm_bvh_inside_dev(th._h, P(p), one, three, P(p)) == -5
        assert lib.psm_bvh_signed_distance_dev(th._h, P(p), one, three, P(p)) == -5
        assert lib.psm_last_error(ctx._h).decode() == "point query before build"
        for fn in (lib.psm_bvh_inside_dev, lib.psm_bvh_signed_distance_dev):
            assert fn(th._h, P(p), ctypes.c_size_t(0), ctypes.c_uint32(2), P(p)) == 0      # n = 0: nothing is touched
            assert fn(th._h, None, one, three, P(p)) == -1
            assert fn(th._h, P(p), one, three, None) == -1
            assert fn(th._h, P(p + 4), one, three, P(p)) == -1
            for s in (0, 2, 4, 6):
                assert fn(th._h, P(p), one, ctypes.c_uint32(s), P(p)) == -1
        assert lib.psm_last_error(ctx._h).decode() == "psm_bvh_signed_distance_dev: samples must be 1, 3 or 5"
        assert lib.psm_bvh_count_hits_dev(th._h, P(p), ctypes.c_size_t(0), P(p)) == 0
        assert lib.psm_bvh_count_hits_dev(th._h, None, one, P(p)) == -1
        assert lib.psm_bvh_count_hits_dev(th._h, P(p), one, None) == -1
        assert lib.psm_last_error(ctx._h).decode() == "psm_bvh_count_hits_dev: NULL pointer"
        assert lib.psm_bvh_count_hits_dev(th._h, P(p + 4), one, P(p)) == -1
        assert lib.psm_last_error(ctx._h).decode() == "psm_bvh_count_hits_dev: rays not 16-byte aligned"
        assert lib.psm_bvh_count_hits_dev(th._h, P(p), one, P(p + 2)) == -1
        assert lib.psm_last_error(ctx._h).decode() == "psm_bvh_count_hits_dev: counts not 4-byte aligned"
        assert lib.psm_bvh_count_hits_dev(th._h, P(p), one, P(p + 4)) == -5                # 4-byte aligned counts pass the check
        assert lib.psm_bvh_inside_dev(th._h, P(p), one, three, P(p + 1)) == -5             # a byte per point: any address
        assert lib.psm_bvh_signed_distance_dev(th._h, P(p), one, three, P(p + 4)) == -1
        assert lib.psm_last_error(ctx._h).decode() == "psm_bvh_signed_distance_dev: points or hits not 16-byte aligned"
        ctx.buf_free(h)
    finally:
        th.close()


def test_inside_query_refuses_other_sample_counts(psm, ctx):
    tris = IQ.cube()
    th = _hier(psm, ctx, tris)
    try:
        p = np.full((4, 3), 0.5, F)
        for s in (0, 2, 4, 6):
            with pytest.raises(psm.PsmError, match="samples must be 1, 3 or 5"):
                th.inside(p, s)
            with pytest.raises(psm.PsmError, match="samples must be 1, 3 or 5"):
                th.signedDistance(p, samples=s)
        assert th.inside(p).all() and np.signbit(th.signedDistance(p).t).all()   # the default: 3
    finally:
        th.close()


def test_inside_query_after_refit(psm, ctx):
    """the icosphere scaled about its centre within the build's bounds and refitted: the answers are the moved mesh's"""
    tris = IQ.icosphere(3)
    th = _hier(psm, ctx, tris)
    try:
        moved = (tris * F(0.75)).astype(F)
        th.clearTribuffer()
        th.loadTriangles(moved.reshape(-1, 9))
        th.refit()
        rng = np.random.RandomState(9)
        p = rng.uniform(-1.1, 1.1, (3000, 3)).astype(F)
        ins = _check_points(psm, th, moved, p, samples=(3,))[3]
        rad = np.linalg.norm(p.astype(np.float64), axis=1)
        clear = np.abs(rad - 0.75) > 0.01
        assert np.array_equal(ins[clear], (rad < 0.75)[clear])
        _check_count(psm, th, moved, p, rng.normal(size=p.shape).astype(F))
    finally:
        th.close()


@functools.lru_cache(maxsize=None)
def _cases():
    return IQ.geometry_cases()


@pytest.mark.parametrize("case", range(5), ids=["icosphere", "torus", "cube_grid", "shell", "shell_flipped"])
def test_inside_closed_meshes(psm, ctx, case):
    """On the closed meshes and point sets of the CPU test: the model's answers exactly, and the geometric check on the GPU's own
    answers -- zero disagreements with the analytic inside for 3 and for 5 rays; the sign of the distance is that answer, with
    rmax = inf and inside a band"""
    name, tris, p, truth, clearance, gap = _cases()[case]
    assert gap < clearance
    th = _hier(psm, ctx, tris)
    try:
        assert th.info().leaf_count == tris.shape[0]
        ins = _check_points(psm, th, tris, p)
        print("%s: one ray wrong on %d of %d points" % (name, int((ins[1] != truth).sum()), p.shape[0]))
        for s in (3, 5):
            bad = np.nonzero(ins[s] != truth)[0]
            assert bad.size == 0, (name, s, bad.size, p[bad[:4]])
            sd = th.signedDistance(p, samples=s)
            assert (sd.tri >= 0).all() and np.array_equal(np.signbit(sd.t), truth)
        band = F(0.05)
        sd = _band(th, p, band)
        near = sd.tri >= 0
        assert near.any() and (~near).any() and np.array_equal(np.signbit(sd.t[near]), truth[near])
        assert (np.abs(sd.t[near]) <= band).all()
    finally:
        th.close()


def _band(th, p, band):
    """signedDistance with a finite rmax: the misses are {0, 0, +inf, -1}"""
    sd = th.signedDistance(p, rmax=band)
    miss = sd.buffer[sd.tri < 0]
    assert np.isposinf(miss[:, 2]).all() and not miss[:, :2].any() and not np.signbit(miss[:, :3]).any()
    return sd


def test_inside_sponza_like_points(psm, ctx, scenes):
    """an open scene: parity means nothing there, the result is the model's all the same"""
    tris = scenes.sponza_like(30011)["tris"].reshape(-1, 3, 3)
    th = _hier(psm, ctx, tris)
    try:
        rng = np.random.RandomState(3)
        p = _scene_points(rng, tris, 1024)
        _check_points(psm, th, tris, p)
        diag = float(np.linalg.norm(tris.reshape(-1, 3).max(0) - tris.reshape(-1, 3).min(0)))
        r = rng.uniform(0, 0.05 * diag, p.shape[0]).astype(F)
        r[:8] = [np.inf, 0, -0.0, -1, np.nan, np.inf, 0, -1]
        _check_points(psm, th, tris, p, r)
    finally:
        th.close()


def test_inside_query_torch_tensors(psm, ctx, scenes):
    if torch is None:
        pytest.skip("torch is not installed")
    tris = IQ.torus()
    rng = np.random.RandomState(6)
    p = rng.uniform([-1.6, -1.6, -0.6], [1.6, 1.6, 0.6], (4099, 3)).astype(F)
    p[-1] = [np.nan, 0, 0]
    o, d = p, rng.normal(size=p.shape).astype(F)
    tmin = rng.uniform(-1, 0.5, p.shape[0]).astype(F)
    r = rng.uniform(0, 0.3, p.shape[0]).astype(F)
    own = psm.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        for c in (own, ctx):     # a context on torch's current stream, and one with its own stream
            th = _hier(psm, c, tris)
            try:
                dev = torch.device("cuda", 0)
                to, td, tt, tr = (torch.from_numpy(x).to(dev) for x in (o, d, tmin, r))
                cnt = th.countHits(to, td, tt)
                assert cnt.device == dev and cnt.dtype == torch.int32 and cnt.shape == (p.shape[0],)
                assert np.array_equal(cnt.cpu().numpy().view(np.uint32), th.countHits(o, d, tmin))
                for s in (1, 3, 5):
                    ins = th.inside(to, s)
                    assert ins.device == dev and ins.dtype == torch.bool
                    assert np.array_equal(ins.cpu().numpy(), th.inside(p, s))
                    sd = th.signedDistance(to, tr, s)
                    assert sd.buffer.device == dev and sd.buffer.shape == (p.shape[0], 4)
                    assert np.array_equal(sd.buffer.cpu().numpy().view(np.uint32), th.signedDistance(p, r, s).buffer.view(np.uint32))
                # one packed [n, 4] tensor serves closestPoint's records and inside (rmax is ignored)
                q = torch.empty((p.shape[0], 4), dtype=torch.float32, device=dev)
                q[:, 0:3], q[:, 3] = to, tr
                assert np.array_equal(th.inside(q).cpu().numpy(), th.inside(p))
                assert np.array_equal(th.inside(q.cpu().numpy()), th.inside(p))
            finally:
                th.close()
    finally:
        own.close()


def test_inside_queries_interleaved_with_the_others(psm, ctx):
    """all seven queries on one context back to back without a synchronisation between them (they share the stack's spill area,
    and the deep fixture uses it): every result equals its model"""
    import point_query_model as PQ
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
        sizes = (rays.nbytes, pts.nbytes, 16 * 512, 16 * 512, 4 * 512, 512, 16 * 512)
        hs = [ctx.buf_alloc(n) for n in sizes]
        ctx.buf_upload(hs[0], rays)
        ctx.buf_upload(hs[1], pts)
        lib = psm.lib()
        ptr = [ctypes.c_void_p(ctx.buf_ptr(h)[0]) for h in hs]
        n, three = ctypes.c_size_t(512), ctypes.c_uint32(3)
        for _ in range(3):
            assert lib.psm_bvh_intersect_dev(th._h, ptr[0], n, ptr[2]) == 0
            assert lib.psm_bvh_signed_distance_dev(th._h, ptr[1], n, three, ptr[6]) == 0
            assert lib.psm_bvh_count_hits_dev(th._h, ptr[0], n, ptr[4]) == 0
            assert lib.psm_bvh_closest_point_dev(th._h, ptr[1], n, ptr[3]) == 0
            assert lib.psm_bvh_inside_dev(th._h, ptr[1], n, three, ptr[5]) == 0
        ray_hits = ctx.buf_download(hs[2], F, 4 * 512).reshape(512, 4)
        pt_hits = ctx.buf_download(hs[3], F, 4 * 512).reshape(512, 4)
        cnt = ctx.buf_download(hs[4], np.uint32, 512)
        ins = ctx.buf_download(hs[5], np.uint8, 512)
        sd = ctx.buf_download(hs[6], F, 4 * 512).reshape(512, 4)
        for h in hs:
            ctx.buf_free(h)
        assert np.array_equal(ray_hits.view(np.uint32), Q.query(tris, leaves, o, d)[0].view(np.uint32))
        assert np.array_equal(pt_hits.view(np.uint32), PQ.query(tris, leaves, p)[0].view(np.uint32))
        assert np.array_equal(cnt, IQ.count(tris, leaves, o, d))
        assert np.array_equal(ins.astype(bool), IQ.inside(tris, leaves, p, 3))
        assert np.array_equal(sd.view(np.uint32), IQ.signed_distance(tris, leaves, p, np.inf, 3).view(np.uint32))
    finally:
        th.close()
