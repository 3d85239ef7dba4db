"""The k-best queries of an instance world on the GPU (psm_world_first_hits_dev / psm_world_nearest_dev, world.hip;
InstanceWorld.firstHits / nearest). The yardstick is tests/world_kbest_query_model.py: the per-instance brute force
rows merged by (value, inst, tri) and cut at k. Every comparison is bit for bit on every query, and every case is also held
against the world's own older answers on the device: slot 0 and its inst are intersect's / closestPoint's record and geom, the
count is min(k, countHits), and it is positive iff occluded / within say so."""
import ctypes

import numpy as np
import pytest

import instance_query_model as NQ
import query_model as Q
import world_kbest_query_model as WK
from test_gpu_kbest_query import GRID_CAP, _quad
from test_gpu_point_query import ROT_SCALE, SHEAR
from test_gpu_world_query import _World, _meshes, _posed_entries, _queries, matrix_world_queries
from test_world_query_cpu import _same, _shift

try:   # (imported before the library loads its HIP runtime, as tests/test_gpu_query.py)
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
KS = (1, 2, 3, 8, 16)


def _col(n, x):
    return np.broadcast_to(np.asarray(x, F), (n,)).copy()


def check_rays(sc, o, d, ks, tmin=0.0, tmax=np.inf, insts=None):
    """firstHits for every k of ks against the model (computed once at the largest: its rows are prefixes, test_world_kbest_cpu)
    and against intersect / countHits / occluded of the same world; returns the model's rows, inst and counts at the largest k"""
    w = sc.world
    o, d = np.ascontiguousarray(o, F).reshape(-1, 3), np.ascontiguousarray(d, F).reshape(-1, 3)
    n = o.shape[0]
    lo, hi = _col(n, tmin), _col(n, tmax)
    exp, einst, ecount = WK.first_hits(sc.insts() if insts is None else insts, o, d, max(ks), lo, hi)
    closest, counts, occ = w.intersect(o, d, lo, hi), w.countHits(o, d, lo, hi), w.occluded(o, d, lo, hi)
    for k in ks:
        got = w.firstHits(o, d, k, lo, hi)
        assert got.buffer.shape == (n, k, 4) and got.geom.shape == (n, k) and got.geom.dtype == np.int32
        assert got.count.shape == (n,) and got.count.dtype == U
        _same(got.buffer, exp[:, :k], "firstHits k = %d" % k)
        _same(got.geom, einst[:, :k], "firstHits inst k = %d" % k)
        _same(got.count, np.minimum(ecount, k), "firstHits count k = %d" % k)
        _same(got.buffer[:, 0], closest.buffer, "firstHits slot 0 against intersect, k = %d" % k)
        _same(got.geom[:, 0], closest.geom, "firstHits inst 0 against intersect, k = %d" % k)
        _same(got.count, np.minimum(counts, k), "firstHits count against countHits, k = %d" % k)
        assert np.array_equal(got.count > 0, occ), k
    return exp, einst, ecount


def check_points(sc, p, ks, rmax=np.inf, insts=None):
    w = sc.world
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    n = p.shape[0]
    rm = _col(n, rmax)
    exp, einst, ecount = WK.nearest(sc.insts() if insts is None else insts, p, max(ks), rm)
    closest, within = w.closestPoint(p, rm), w.within(p, rm)
    for k in ks:
        got = w.nearest(p, k, rm)
        assert got.buffer.shape == (n, k, 4) and got.geom.shape == (n, k) and got.count.shape == (n,)
        _same(got.buffer, exp[:, :k], "nearest k = %d" % k)
        _same(got.geom, einst[:, :k], "nearest inst k = %d" % k)
        _same(got.count, np.minimum(ecount, k), "nearest count k = %d" % k)
        _same(got.buffer[:, 0], closest.buffer, "nearest slot 0 against closestPoint, k = %d" % k)
        _same(got.geom[:, 0], closest.geom, "nearest inst 0 against closestPoint, k = %d" % k)
        assert np.array_equal(got.count > 0, within), k
    return exp, einst, ecount


def _spread_rows(inst, count):
    """the queries whose row holds 3 or more records from 2 or more instances"""
    live = np.arange(inst.shape[1])[None] < count[:, None]
    first = inst[:, :1]
    return (count >= 3) & ((inst != first) & live).any(axis=1)


@pytest.mark.parametrize("n", [1, 2, 33, 257])
def test_world_kbest_parity_with_the_model(psm, ctx, n):
    """the entries and queries of test_gpu_world_query's parity test: k = 2, 3 fill most lists (the prune against the last slot),
    k = 16 lists are mostly complete"""
    ico, tor = _meshes()
    entries, spread = _posed_entries(n, 100 + n)
    with _World(psm, ctx, [ico, tor], entries) as sc:
        (o, d, tmin, tmax), (p, rmax) = _queries(np.random.RandomState(n), spread)
        insts = sc.insts()
        _, einst, ecount = check_rays(sc, o, d, KS, tmin, tmax, insts)
        _, pinst, pcount = check_points(sc, p, KS, rmax, insts)
        if n == 33:   # so that the case cannot pass emptily
            assert _spread_rows(einst, ecount).sum() >= 100 and _spread_rows(pinst, pcount).sum() >= 100
        if n > 1:
            assert (ecount > 2).any() and (pcount > 2).any()


@pytest.mark.parametrize("opt", [ROT_SCALE, SHEAR], ids=["rotate_scale", "shear"])
def test_a_member_built_with_an_optimisation_matrix(psm, ctx, opt):
    """the torus of a two-mesh world built with a matrix: firstHits on the rays that are fully well-posed in every instance
    (tests/ray_prune_model.py; at most 1 % are left out) and nearest on every point, bit for bit against the model and the
    world's own older answers"""
    ico, tor = _meshes()
    entries, _ = _posed_entries(7, 107)
    with _World(psm, ctx, [ico, tor], entries, [None, opt]) as sc:
        t = np.array(sc.ths[1].info().transform).reshape(4, 4)[:3, :3]
        assert np.abs(t - np.diag(np.diag(t))).max() > 0.01
        (o, d, tmin, tmax), _ = matrix_world_queries(sc, 64)
        _, (p, rmax) = _queries(np.random.RandomState(65), 2.0, 1024)
        insts = sc.insts()
        _, einst, ecount = check_rays(sc, o, d, KS, tmin, tmax, insts)
        check_rays(sc, o, d, (4, 16), insts=insts)
        _, pinst, pcount = check_points(sc, p, KS, rmax, insts)
        assert (ecount > 2).any() and (pcount > 2).any() and (einst[:, 0] % 2 == 1).any() and (pinst[:, 0] % 2 == 1).any()


def test_world_kbest_stacked_sheets(psm, ctx):
    """20 instances of one two-triangle quad at z = 1 .. 20 and, behind them, an instance whose hierarchy holds a single triangle
    (the lone-leaf path of enter()): more hits than k and fewer, rays that miss, rays that start between sheets, windows whose ends
    sit exactly on a sheet"""
    rng = np.random.RandomState(31)
    lone = np.array([[[-0.5, -0.5, 0], [0.5, -0.5, 0], [0, 0.5, 0]]], F)
    entries = [(0, _shift(0, 0, z)) for z in range(1, 21)] + [(1, _shift(0, 0, 21.5))]
    with _World(psm, ctx, [_quad(0.0), lone], entries) as sc:
        assert sc.ths[0].info().leaf_count == 2 and sc.ths[1].info().leaf_count == 1
        insts = sc.insts()
        o = np.zeros((320, 3), F)
        o[:, :2] = rng.uniform(-0.1, 0.1, (320, 2))               # (inside the quad and inside the lone triangle)
        o[:, 2] = -1.0
        d = np.tile(F([0, 0, 1]), (320, 1))
        d[:, :2] = rng.uniform(-0.002, 0.002, (320, 2))
        o[256:288, 0] += 2.0                                         # 32 that miss
        o[288:, 2] = rng.uniform(6.1, 16.9, 32)                      # 32 that start between sheets
        exp, einst, count = check_rays(sc, o, d, KS, insts=insts)
        assert (count[:256] == 16).all() and (count[256:288] == 0).all() and ((count[288:] > 4) & (count[288:] < 16)).all()
        # sheet after sheet (a ray that crosses a quad's diagonal within the test's 1e-5 counts both of its triangles)
        assert (einst[:256, 0] == 0).all() and (np.diff(einst[:256], axis=1) >= 0).all() and (einst[:256, 15] >= 14).all()
        assert ((einst[288:] == 20).sum(axis=1) == 1).all()          # the lone triangle closes every short list
        # the window's ends exactly at the t of the 4th and the 11th sheet crossed: both ends count (8 sheets: fewer than 16)
        lo, hi = exp[:256, 3, 2].copy(), exp[:256, 10, 2].copy()
        _, winst, wcount = check_rays(sc, o[:256], d[:256], KS, lo, hi, insts=insts)
        assert (wcount >= 8).all() and (wcount < 16).all() and (winst[:, 0] == 3).all()
        # points inside the stack: the nearest sheets in order, rmax exactly at a sheet's distance
        p = o[:256].copy()
        p[:, 2] = rng.uniform(0.0, 22.0, 256)
        pexp, _, pcount = check_points(sc, p, KS, insts=insts)
        assert (pcount == 16).all()
        check_points(sc, p, (1, 3, 16), pexp[:, 5, 2].copy(), insts=insts)


def test_world_kbest_coincident_instances(psm, ctx):
    """one icosphere at one pose five times, interleaved in the list with other bodies -- their tree order differs from their
    index order --: every hit of it ties five times; k = 3 cuts the group, k = 16 lists inst ascending inside each equal value"""
    ico, tor = _meshes()
    rng = np.random.RandomState(32)
    pose = NQ.random_pose(rng, shift=0.5)
    others = [NQ.random_pose(rng, reflect=bool(k & 1), shift=2.5) for k in range(6)]
    entries = [(0, pose), (1, others[0]), (0, pose), (0, others[1]), (1, others[2]), (0, pose), (0, pose), (1, others[3]),
               (0, others[4]), (0, pose), (1, others[5])]
    same = np.array([0, 2, 5, 6, 9])
    with _World(psm, ctx, [ico, tor], entries) as sc:
        insts = sc.insts()
        n = 512
        o = (pose[:, 3] + rng.uniform(-3, 3, (n, 3))).astype(F)
        d = (pose[:, 3] + rng.uniform(-0.4, 0.4, (n, 3)) - o).astype(F)
        exp, einst, ecount = check_rays(sc, o, d, (1, 3, 4, 5, 6, 16), insts=insts)
        t = exp[:, :, 2]
        live = np.arange(16)[None] < ecount[:, None]
        tied = 0
        for i in range(n):
            for s in np.nonzero(live[i] & np.isin(einst[i], same))[0]:
                if einst[i, s] == 0 and s + 5 <= ecount[i]:              # a whole group: inst ascending at one bit-equal value
                    assert list(einst[i, s:s + 5]) == list(same) and (t[i, s:s + 5].view(U) == t[i, s].view(U)).all()
                    tied += 1
        assert tied > 200
        with np.errstate(invalid="ignore"):
            asc = (t[:, :-1] < t[:, 1:]) | ((t[:, :-1] == t[:, 1:]) & (einst[:, :-1] <= einst[:, 1:]))
        assert (asc | ~live[:, 1:]).all()
        p = (pose[:, 3] + rng.uniform(-1.5, 1.5, (n, 3))).astype(F)
        _, pinst, pcount = check_points(sc, p, (1, 3, 4, 5, 6, 16), rng.uniform(0.3, 2.0, n).astype(F), insts=insts)
        assert (np.isin(pinst[:, 0], same) & (pcount >= 5)).sum() > 100


def test_world_kbest_deep_stack_beside_the_list(psm, ctx):
    """the deep fixture of test_gpu_kbest_query at two poses, k = 16: the stack spills past its 16 LDS entries while the list
    lives in dynamic LDS beside it"""
    tris, o, d = Q.deep_fixture()
    with _World(psm, ctx, [tris], [(0, _shift(0, 0, 0)), (0, _shift(0.03125, 0, 0))]) as sc:
        insts = sc.insts()
        _, einst, count = check_rays(sc, o, d, (16,), insts=insts)
        assert (count > 0).sum() > o.shape[0] // 2 and (count == 16).any()
        assert ((einst == 0).any(axis=1) & (einst == 1).any(axis=1)).any()
        p = (o + d * np.linspace(0.4, 1.6, o.shape[0]).astype(F)[:, None]).astype(F)
        _, _, pcount = check_points(sc, p, (16,), insts=insts)
        assert (pcount == 16).all()


@pytest.mark.parametrize("n", [1, 63, 65, GRID_CAP * 64 + 65])
def test_world_kbest_batch_sizes(psm, ctx, n):
    """the last size takes a second trip of the grid-stride loop: the list must start empty again"""
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    tris = np.concatenate([tri, tri + F([0.5, 0, 0]), tri + F([1, 0.5, 0]), tri + F([1.5, 0, 0.5])])
    rng = np.random.RandomState(n % 1000)
    o = rng.uniform(-0.5, 0.5, (n, 3)).astype(F)
    d = (F([2, 0, 0]) + rng.uniform(-1.5, 1.5, (n, 3)).astype(F) - o).astype(F)
    with _World(psm, ctx, [tris], [(0, _shift(0, 0, 0)), (0, _shift(0.25, 0.125, 0))]) as sc:
        insts = sc.insts()
        _, _, count = check_rays(sc, o, d, (3,), insts=insts)
        if n > 64:
            assert len(np.unique(count)) > 1 and len(np.unique(count[-65:])) > 1
        check_points(sc, o, (3,), rng.uniform(0.5, 2.5, n).astype(F), insts=insts)


def test_world_kbest_invalid_queries_are_rows_of_misses(psm, ctx):
    ico, tor = _meshes()
    with _World(psm, ctx, [ico, tor], [(0, _shift(0, 0, 0)), (1, _shift(0.5, 0, 0)), (0, _shift(0, 0.5, 0))]) as sc:
        insts = sc.insts()
        o = np.tile(F([-3, 0.1, 0.05]), (8, 1))
        d = np.tile(F([1, 0, 0]), (8, 1))
        tmin, tmax = np.zeros(8, F), np.full(8, np.inf, F)
        o[0, 1], o[1, 0] = np.nan, np.inf                            # a NaN / infinite origin
        d[2, 2] = np.nan
        tmin[3], tmax[3] = 2.0, 1.0                                  # tmin > tmax
        tmin[4] = np.nan
        tmax[5] = np.nan
        for k in (1, 5, 16):
            got = sc.world.firstHits(o, d, k, tmin, tmax)
            assert (got.count[:6] == 0).all() and (got.count[6:] > 0).all()
            assert (got.tri[:6] == -1).all() and (got.geom[:6] == -1).all() and np.isinf(got.t[:6]).all()
            assert not got.buffer[:6, :, :2].any()
        check_rays(sc, o, d, (1, 5, 16), tmin, tmax, insts=insts)
        p = np.tile(F([0.2, 0.1, 0.9]), (8, 1))
        rmax = np.full(8, np.inf, F)
        p[0, 0], p[1, 2] = np.nan, -np.inf
        rmax[2], rmax[3], rmax[4] = -1.0, np.nan, -np.inf
        for k in (1, 5, 16):
            got = sc.world.nearest(p, k, rmax)
            assert (got.count[:5] == 0).all() and (got.count[5:] == k).all()
            assert (got.tri[:5] == -1).all() and (got.geom[:5] == -1).all() and np.isinf(got.t[:5]).all()
            assert not got.buffer[:5, :, :2].any()
        check_points(sc, p, (1, 5, 16), rmax, insts=insts)


def test_world_kbest_empty_world(psm, ctx):
    """n x k miss records, inst = -1 and counts 0, over whatever the buffers held"""
    world = psm.InstanceWorld(ctx, [], capacity=4)
    try:
        assert len(world) == 0
        rng = np.random.RandomState(33)
        o, d = rng.uniform(-1, 1, (300, 3)).astype(F), rng.normal(size=(300, 3)).astype(F)
        for k in (1, 7, 16):
            for got in (world.firstHits(o, d, k), world.nearest(o, k)):
                assert got.buffer.shape == (300, k, 4) and got.geom.shape == (300, k)
                assert (got.count == 0).all() and (got.geom == -1).all() and (got.tri == -1).all()
                assert np.isinf(got.t).all() and (got.t > 0).all() and not got.buffer[:, :, :2].any()
    finally:
        world.close()


def test_world_kbest_set_transform_moves_the_rows_without_a_rebuild(psm, ctx):
    ico, tor = _meshes()
    with _World(psm, ctx, [ico, tor], [(0, _shift(0, 0, 0)), (0, _shift(5, 0, 0)), (1, _shift(0, 5, 0))]) as sc:
        nodes = [th.download(psm.BVH_NODE32, np.uint32, 8 * max(th.info().leaf_count - 1, 1)).copy() for th in sc.ths]
        o, d = np.asarray([[-3, 0.1, 0.05]], F), np.asarray([[1, 0, 0]], F)
        got = sc.world.firstHits(o, d, 8)
        assert got.count[0] == 4 and list(got.geom[0, :4]) == [0, 0, 1, 1]
        sc.world.setTransform(0, _shift(0, -9, 0))
        got = sc.world.firstHits(o, d, 8)
        assert got.count[0] == 2 and list(got.geom[0, :2]) == [1, 1]
        sc.world.setTransforms(1, [_shift(0, 9, 0), _shift(2, 0, 0)])
        got = sc.world.firstHits(o, d, 8)
        assert got.count[0] > 0 and (got.geom[0, :got.count[0]] == 2).all()
        rays, points = _queries(np.random.RandomState(2), 5.0, 500)
        check_rays(sc, rays[0], rays[1], (1, 3, 16), rays[2], rays[3])
        check_points(sc, points[0], (1, 3, 16), points[1])
        for th, before in zip(sc.ths, nodes):
            assert np.array_equal(th.download(psm.BVH_NODE32, np.uint32, before.size), before)


def test_world_kbest_a_rebuilt_member_refuses(psm, ctx):
    ico, tor = _meshes()
    shifts = [_shift(0, 0, 0), _shift(3, 0, 0), _shift(0, 3, 0)]
    with _World(psm, ctx, [ico, tor], [(0, shifts[0]), (1, shifts[1]), (0, shifts[2])]) as sc:
        rays, points = _queries(np.random.RandomState(3), 3.0, 300)
        check_rays(sc, rays[0], rays[1], (4,), rays[2], rays[3])
        h = sc.ths[1]
        h.markDirty()
        h.build()
        with pytest.raises(psm.PsmError, match="psm_world_first_hits_dev: instance 1's hierarchy was rebuilt"):
            sc.world.firstHits(rays[0], rays[1], 4)
        with pytest.raises(psm.PsmError, match="psm_world_nearest_dev: instance 1's hierarchy was rebuilt"):
            sc.world.nearest(points[0], 4)
        sc.world.setInstances([(sc.ths[k], m) for k, m in zip(sc.which, shifts)])
        check_rays(sc, rays[0], rays[1], (4,), rays[2], rays[3])
        check_points(sc, points[0], (4,), points[1])


@pytest.mark.skipif(torch is None, reason="torch is not installed")
def test_world_kbest_torch_tensors_on_a_side_stream(psm, ctx):
    ico, tor = _meshes()
    entries, spread = _posed_entries(40, 77)
    with _World(psm, ctx, [ico, tor], entries) as sc:
        (o, d, tmin, tmax), (p, rmax) = _queries(np.random.RandomState(8), spread, 1000)
        ref, pref = sc.world.firstHits(o, d, 5, tmin, tmax), sc.world.nearest(p, 5, rmax)
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            t = [torch.from_numpy(a).to(dev, non_blocking=True) for a in (o, d, tmin, tmax, p, rmax)]
            got, pgot = sc.world.firstHits(t[0], t[1], 5, t[2], t[3]), sc.world.nearest(t[4], 5, t[5])
            bufs = [x.cpu() for x in (got.buffer, got.geom, got.count, got.tri, pgot.buffer, pgot.geom, pgot.count)]   # (in order)
        assert got.buffer.device == dev and got.buffer.shape == (1000, 5, 4) and got.geom.shape == (1000, 5)
        assert got.geom.dtype == torch.int32 and got.count.dtype == torch.int32
        _same(bufs[0].numpy(), ref.buffer, "torch firstHits")
        _same(bufs[1].numpy(), ref.geom, "torch firstHits inst")
        _same(bufs[2].numpy().view(U), ref.count, "torch firstHits count")
        assert np.array_equal(bufs[3].numpy(), ref.tri)
        _same(bufs[4].numpy(), pref.buffer, "torch nearest")
        _same(bufs[5].numpy(), pref.geom, "torch nearest inst")
        _same(bufs[6].numpy().view(U), pref.count, "torch nearest count")
        assert (ref.count > 1).sum() > 50 and (pref.count > 1).sum() > 50


def test_world_kbest_refusals_launch_nothing(psm, ctx):
    """k = 0, k = 17, NULL and misaligned pointers are refused on the host by their messages: the outputs keep what they held"""
    lib = psm.lib()
    ico, _ = _meshes()
    with _World(psm, ctx, [ico], [(0, _shift(0, 0, 0)), (0, _shift(0.25, 0, 0))]) as sc:
        n = 4
        hin, hout, hinst, hcnt = ctx.buf_alloc(32 * n), ctx.buf_alloc(16 * 17 * n), ctx.buf_alloc(4 * 17 * n), ctx.buf_alloc(4 * n)
        try:
            rays = np.zeros((n, 8), F)
            rays[:, 0:3], rays[:, 4], rays[:, 7] = (-3.0, 0.1, 0.05), 1.0, np.inf   # (off the icosphere's edges)
            ctx.buf_upload(hin, rays)
            ctx.buf_upload(hout, np.full(4 * 17 * n, 7.0, F))
            ctx.buf_upload(hinst, np.full(17 * n, 55, np.int32))
            ctx.buf_upload(hcnt, np.full(n, 77, U))
            pin, pout, pinst, pcnt = (ctypes.c_void_p(ctx.buf_ptr(h)[0]) for h in (hin, hout, hinst, hcnt))
            w = sc.world._w

            def call(fn, k, p_in=pin, p_out=pout, p_inst=pinst, p_cnt=pcnt, count=n):
                return fn(w, p_in, ctypes.c_size_t(count), ctypes.c_uint32(k), p_out, p_inst, p_cnt)

            def err():
                return lib.psm_last_error(ctx._h).decode()
            off = lambda p, by: ctypes.c_void_p(p.value + by)
            for name in ("psm_world_first_hits_dev", "psm_world_nearest_dev"):
                fn = getattr(lib, name)
                what = "rays" if name == "psm_world_first_hits_dev" else "points"
                assert call(fn, 4, count=0) == 0                       # n = 0 is answered first, as for every query
                for k in (0, 17, 1 << 31):
                    assert call(fn, k) == -1 and err() == name + ": k must be 1 .. 16"
                for kw in ("p_in", "p_out", "p_inst", "p_cnt"):
                    assert call(fn, 4, **{kw: None}) == -1 and err() == name + ": NULL pointer", kw
                assert call(fn, 4, p_in=off(pin, 4)) == -1 and err() == "%s: %s or hits not 16-byte aligned" % (name, what)
                assert call(fn, 4, p_out=off(pout, 4)) == -1 and err() == "%s: %s or hits not 16-byte aligned" % (name, what)
                assert call(fn, 4, p_cnt=off(pcnt, 2)) == -1 and err() == name + ": counts not 4-byte aligned"
                assert call(fn, 4, p_inst=off(pinst, 2)) == -1 and err() == name + ": inst not 4-byte aligned"
            ctx.sync()
            assert (ctx.buf_download(hout, F, 4 * 17 * n) == 7.0).all() and (ctx.buf_download(hinst, np.int32, 17 * n) == 55).all()
            assert (ctx.buf_download(hcnt, U, n) == 77).all()
            for k in (0, 17):
                with pytest.raises(psm.PsmError):
                    sc.world.firstHits(rays[:, 0:3], rays[:, 4:7], k)
                with pytest.raises(psm.PsmError):
                    sc.world.nearest(rays[:, 0:3], k)
            assert call(lib.psm_world_first_hits_dev, 16) == 0             # and the same buffers are fine at k = 16
            ctx.sync()
            assert (ctx.buf_download(hcnt, U, n) == 4).all()               # two spheres, each crossed twice
            assert list(ctx.buf_download(hinst, np.int32, 16 * n)[:6]) == [0, 1, 0, 1, -1, -1]
        finally:
            for h in (hin, hout, hinst, hcnt):
                ctx.buf_free(h)
