"""The triangle queries of an instance world on the GPU (psm_world_tri_overlaps_dev / psm_world_tri_count_dev /
psm_world_tri_triangles_dev, world_tri.hip; InstanceWorld.overlapsTriangle / countOnTriangle / trianglesOnTriangle; DESIGN.md
4.20). The yardstick is tests/world_tri_query_model.py part (a): tri_tri in numpy float32 over the forward-posed downloaded leaves
of every instance. Every comparison is exact on every query, and in every case the three queries are also held against one
another: overlaps == (count > 0), the rows' count == min(k, count), the live slots are the non-negative ones, the rows are
prefixes."""
import ctypes

import numpy as np
import pytest

import inside_query_model as IQ
import instance_query_model as NQ
import world_box_query_model as WB
import world_tri_query_model as WT
from test_gpu_box_query import GRID_CAP, ROT_SCALE, SHEAR
from test_gpu_world_box import KS, _World, _members, _rigid_entries, _same, _soup
from test_world_box_cpu import _pose, _rotation, cube, lattice_world
from test_world_tri_cpu import lattice_queries, posed_triangles

try:   # (imported before the library loads its HIP runtime, as tests/test_gpu_query.py)
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
U = np.uint32


def check_tris(sc, q, ks=KS, insts=None):
    """the three queries against (a) (computed once at the largest k: its rows are prefixes, test_world_tri_cpu) and against one
    another; returns (a) at the largest k: flag, count, tri rows, inst rows"""
    w = sc.world
    q = np.ascontiguousarray(q, F).reshape(-1, 3, 3)
    n = q.shape[0]
    flag, count, trows, irows, _ = WT.flat(sc.insts() if insts is None else insts, q, max(ks))
    got_flag, got_count = w.overlapsTriangle(q), w.countOnTriangle(q.reshape(-1, 9))
    assert got_flag.shape == (n,) and got_flag.dtype == np.bool_ and got_count.shape == (n,) and got_count.dtype == U
    _same(got_flag, flag, "overlapsTriangle")
    _same(got_count, count, "countOnTriangle")
    assert np.array_equal(got_flag, got_count > 0)
    widest = None
    for k in sorted(ks, reverse=True):
        got = w.trianglesOnTriangle(q, k)
        assert got.tri.shape == (n, k) and got.tri.dtype == np.int32 and got.geom.shape == (n, k) and got.geom.dtype == np.int32
        assert got.count.shape == (n,) and got.count.dtype == U
        _same(got.tri, trows[:, :k], "trianglesOnTriangle tri, k = %d" % k)
        _same(got.geom, irows[:, :k], "trianglesOnTriangle inst, k = %d" % k)
        _same(got.count, np.minimum(got_count, U(k)), "trianglesOnTriangle count against countOnTriangle, k = %d" % k)
        live = np.arange(k)[None] < got.count[:, None]
        assert np.array_equal(got.tri >= 0, live) and np.array_equal(got.geom >= 0, live)
        if widest is None:
            widest = got
        _same(got.tri, widest.tri[:, :k], "trianglesOnTriangle k = %d is a prefix" % k)
        _same(got.geom, widest.geom[:, :k], "trianglesOnTriangle inst k = %d is a prefix" % k)
    return flag, count, trows, irows


def _around(rng, centre, size):
    """a triangle per centre: its vertices normal around it with the standard deviation `size` [n, 1, 1]"""
    return centre[:, None, :] + rng.normal(size=(centre.shape[0], 3, 3)) * size


def test_identity_world_of_one_equals_the_hierarchy(psm, ctx):
    tris = _soup(61, 600, 1.0, 0.1)
    rng = np.random.RandomState(62)
    q = _around(rng, rng.uniform(-1.1, 1.1, (2048, 3)), 10.0 ** rng.uniform(-3, -0.1, (2048, 1, 1))).astype(F)
    q[0, 0, 0], q[1, 1, 1], q[2, 2, 2] = np.nan, np.inf, -np.inf
    pick = rng.choice(600, 37)
    q[3:40] = tris[pick, :1]                                               # points on stored v0
    q[40:77] = tris[pick]                                                  # the stored triangles themselves
    q[77] = [[-3, -3, 0.1], [3, -3, 0.0], [0, 3, -0.1]]                    # a plane through the soup
    with _World(psm, ctx, [tris], [(0, NQ.IDENTITY)]) as sc:
        th, w = sc.ths[0], sc.world
        _same(w.overlapsTriangle(q), th.triOverlaps(q), "overlaps")
        _same(w.countOnTriangle(q), th.triCount(q), "count")
        for k in (1, 4, 16):
            a, b = w.trianglesOnTriangle(q, k), th.triTriangles(q, k)
            _same(a.tri, b.tri, "rows k = %d" % k)
            _same(a.count, b.count, "rows' count k = %d" % k)
            assert np.array_equal(a.geom, np.where(b.tri >= 0, 0, -1))
        _, count, _, _ = check_tris(sc, q, (16,))
        assert (count[:3] == 0).all() and (count[3:77] >= 1).all() and count[77] > 16 and (count[78:] == 0).any()


def test_lattice_world_and_lattice_queries(psm, ctx):
    """cubes at the 48 signed axis permutations and integer translations, three of them twice: all arithmetic exact; lattice
    triangles, copies of posed stored triangles, coplanar neighbours, points and segments on vertices and edges. Coincident
    instances are listed lowest instance first."""
    model = lattice_world()
    q = lattice_queries(model)
    with _World(psm, ctx, [cube()], [(0, m[2]) for m in model]) as sc:
        assert sc.ths[0].info().leaf_count == 12
        flag, count, trows, irows = check_tris(sc, q)
        assert (count > 16).any() and ((count > 0) & (count < 16)).any() and (count[:500] == 0).any() and (count[500:] >= 1).all()
        both = np.nonzero((irows == 0).any(axis=1) & (irows == 48).any(axis=1) & (count <= 16))[0]
        assert both.size > 0
        for i in both[:20]:
            assert list(trows[i][irows[i] == 0]) == list(trows[i][irows[i] == 48])
            live = irows[i][irows[i] >= 0]
            assert list(live) == sorted(live)


def parity_queries(n, insts, spread):
    """1 024 world triangles for a world of n random rigid poses: [0, 8) invalid; then per instance (the first 8) 8 points on posed
    v0' and 8 posed copies of stored triangles; [136] one huge triangle through everything; the rest over three decades of size,
    every second one centred near a posed vertex"""
    rng = np.random.RandomState(n)
    B = 1024
    centre = rng.uniform(-spread - 1.2, spread + 1.2, (B, 3))
    for i in range(1, B, 2):                                               # every second one near a posed vertex
        inst = insts[rng.randint(len(insts))]
        one = rng.randint(len(inst[1]))
        centre[i] = posed_triangles((inst[0], inst[1][one:one + 1], inst[2]))[0, 0] + rng.normal(size=3) * 0.05
    q = _around(rng, centre, 10.0 ** rng.uniform(-3, 0.3, (B, 1, 1)) * spread).astype(F)      # sizes over three decades
    q[0, 0, 0], q[1, 1, 1], q[2, 2, 2], q[3, 0, 2] = np.nan, np.nan, np.inf, np.inf
    q[4, 1, 0], q[5, 2, 1] = -np.inf, -np.inf
    q[6], q[7, 1] = np.nan, np.inf
    at = 8
    for inst in insts[:8]:
        t = posed_triangles((inst[0], np.sort(inst[1])[:8], inst[2])).astype(F)
        q[at:at + t.shape[0]] = t[:, :1]
        q[at + 8:at + 8 + t.shape[0]] = t
        at += 16
    q[136] = [[-4 * spread - 16, -3 * spread - 12, -spread - 4], [4 * spread + 16, -3 * spread - 12, 0], [0, 5 * spread + 20, spread + 4]]
    return q


def parity_conditions(n, count, insts):
    """what makes the parity case meaningful: the invalid queries answer nothing, the points and the copies count, the huge
    triangle meets many, and queries with count 0, with 1 .. 16 and with more than 16 all occur among the rest"""
    assert (count[:8] == 0).all() and (count[8:8 + 16 * min(n, 8)] >= 1).all()
    rest = count[137:]
    none, some, many = (rest == 0).sum(), ((rest > 0) & (rest <= 16)).sum(), (rest > 16).sum()
    assert count[136] > 16 and none > 20 and some > 20 and many > 4, (count[136], none, some, many)


@pytest.mark.parametrize("n", [2, 33, 257])
def test_world_tri_parity_with_the_flat_answer(psm, ctx, n):
    members = _members()
    assert members[0].shape[0] == 80 and members[1].shape[0] == 200
    entries, spread = _rigid_entries(n, 200 + n)
    with _World(psm, ctx, members, entries) as sc:
        insts = sc.insts()
        q = parity_queries(n, insts, spread)
        flag, count, trows, irows = check_tris(sc, q, KS, insts)
        parity_conditions(n, count, insts)
        assert sc.ths[2].info().leaf_count > 900                         # (the deep member: the spill path)
        assert (irows[136] >= 0).all() and list(zip(irows[136], trows[136])) == sorted(zip(irows[136], trows[136]))


def test_a_member_far_from_its_origin(psm, ctx):
    """object coordinates at +1000, the pose brings the body back; beside it the same body at -1000 taken out to +2000"""
    rng = np.random.RandomState(64)
    near = _soup(65, 150, 1.0, 0.15)
    far = (near + F(1000)).astype(F)
    r0, r1 = _rotation(rng), _rotation(rng, True)
    entries = [(0, _pose(r0, -r0 @ np.full(3, 1000.0))), (1, _pose(r1, r1 @ np.full(3, 1000.0) + 2000.0)), (1, NQ.IDENTITY)]
    with _World(psm, ctx, [far, (near - F(1000)).astype(F)], entries) as sc:
        insts = sc.insts()
        q = []
        for inst in insts:
            v0 = posed_triangles(inst)[:, 0]
            c = v0[rng.randint(0, v0.shape[0], 300)] + rng.normal(size=(300, 3)) * 0.05
            q.append(_around(rng, c, 10.0 ** rng.uniform(-2, 0, (300, 1, 1))))
        _, count, _, irows = check_tris(sc, np.concatenate(q), (4, 16), insts)
        for j in range(3):
            assert (count[300 * j:300 * (j + 1)] > 0).mean() > 0.2 and (irows[300 * j:300 * (j + 1), 0] == j).any()


def test_tiny_members_and_the_empty_world(psm, ctx):
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    degenerate = np.repeat(tri[:, :1], 3, axis=1)                    # three equal vertices: the build keeps no leaf
    meshes = [np.concatenate([degenerate] * 4), np.concatenate([degenerate, tri, degenerate]),
              np.concatenate([tri, degenerate, tri + F([0.5, 0, 0])]), np.concatenate([tri, tri + F([0.25, 0, 0]), degenerate, tri + F([0.5, 0, 0])])]
    rng = np.random.RandomState(66)
    entries = [(k % 4, NQ.random_pose(rng, reflect=bool(k & 2), shift=1.5)) for k in range(12)]
    q = _around(rng, rng.uniform(-3, 3, (600, 3)), rng.uniform(0.0, 1.5, (600, 1, 1))).astype(F)
    with _World(psm, ctx, meshes, entries) as sc:
        assert [th.info().leaf_count for th in sc.ths] == [0, 1, 2, 3]
        insts = sc.insts()
        q[0:12] = np.concatenate([posed_triangles(i)[:1] for i in insts if len(i[1])] + [np.zeros((3, 3, 3))])[:12]   # copies: they count
        _, count, _, _ = check_tris(sc, q, (1, 16), insts)
        assert (count[:9] >= 1).all() and count.min() == 0 and (count[12:] > 0).any()
        for one in range(4):                                          # worlds of one: no tree, the instance is entered by every query
            sc.world.setInstances([(sc.ths[one], entries[one][1])])
            sc.which = [one]
            one_inst = sc.insts()
            if one:
                q[0] = posed_triangles(one_inst[0])[0]
            _, c1, _, _ = check_tris(sc, q, (2,), one_inst)
            assert (c1[0] >= 1) == (one > 0) and c1.max() <= one
        sc.world.setInstances([])                                     # the empty world answers without a tree
        sc.which = []
        assert len(sc.world) == 0
        assert not sc.world.overlapsTriangle(q).any() and not sc.world.countOnTriangle(q).any()
        got = sc.world.trianglesOnTriangle(q, 5)
        assert (got.tri == -1).all() and (got.geom == -1).all() and not got.count.any() and got.tri.shape == (600, 5)


@pytest.mark.parametrize("n", [1, 63, 65, GRID_CAP * 64 + 65])
def test_world_tri_batch_sizes(psm, ctx, n):
    """the last size takes a second trip of the grid-stride loop: the count and the list must start empty again"""
    rng = np.random.RandomState(67)
    entries = [(0, NQ.random_pose(rng, reflect=bool(k & 1), shift=1.0)) for k in range(3)]
    rng = np.random.RandomState(n % 1000)
    q = _around(rng, rng.uniform(-2.2, 2.2, (n, 3)), rng.uniform(0.0, 0.7, (n, 1, 1))).astype(F)
    with _World(psm, ctx, [_soup(68, 24, 1.0, 0.3)], entries) as sc:
        _, count, trows, _ = check_tris(sc, q, (2,))
        if n > 64:
            assert len(np.unique(count)) > 2 and len(np.unique(count[-65:])) > 2
            assert (count[-65:] == 0).any() and (trows[-65:, 0] >= 0).any()      # the second trip: empty rows beside live ones


def test_4096_poses_of_the_cube_against_4096_small_triangles(psm, ctx):
    rng = np.random.RandomState(69)
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), axis=-1).reshape(-1, 3)
    entries = [(0, _pose(_rotation(rng, bool(k & 1)), 2.0 * g[k] + rng.uniform(-0.4, 0.4, 3))) for k in range(4096)]
    q = _around(rng, 2.0 * g[rng.permutation(4096)] + 0.5 + rng.uniform(-0.9, 0.9, (4096, 3)), 0.6).astype(F)
    with _World(psm, ctx, [cube()], entries) as sc:
        assert len(sc.world) == 4096
        _, count, _, irows = check_tris(sc, q, (4, 16))
        assert (count > 0).sum() > 1500 and (count == 0).sum() > 50 and len(np.unique(irows[irows >= 0])) > 1500


@pytest.mark.parametrize("opt", [ROT_SCALE, SHEAR], ids=["rotate_scale", "shear"])
def test_a_member_built_with_an_optimisation_matrix(psm, ctx, opt):
    rng = np.random.RandomState(70)
    c = rng.uniform(-1, 1, (800, 1, 3)) * [1.0, 0.3, 2.0]
    tris = (c + rng.uniform(-0.08, 0.08, (800, 3, 3))).astype(F)
    entries = [(0, NQ.random_pose(rng, reflect=bool(k & 1), shift=2.0)) for k in range(6)]
    with _World(psm, ctx, [tris], entries, [opt]) as sc:
        t = np.array(sc.ths[0].info().transform).reshape(4, 4)[:3, :3]
        assert np.abs(t - np.diag(np.diag(t))).max() > 0.01
        insts = sc.insts()
        q = []
        for inst in insts:
            pt = posed_triangles(inst)
            pick = pt[rng.randint(0, pt.shape[0], 64)]
            touch = pick.copy()                                       # a vertex on the posed v0', the others leaving it: the tightest case
            touch[:, 1:] = touch[:, :1] + rng.normal(size=(64, 2, 3)) * 10.0 ** rng.uniform(-3, -0.5, (64, 1, 1))
            q.append(touch)
            q.append(_around(rng, pick[:, 0] + rng.normal(size=(64, 3)) * 0.05, 10.0 ** rng.uniform(-3, -0.3, (64, 1, 1))))
        q.append(np.array([[[-9, -9, 0], [9, -9, 0.1], [0, 9, -0.1]]], D))      # a plane through all six
        _, count, _, _ = check_tris(sc, np.concatenate(q).astype(F), (3, 16), insts)
        assert all((count[128 * j:128 * j + 64] >= 1).all() for j in range(6)) and count[-1] > 16


def test_set_transform_refit_and_refresh(psm, ctx):
    rng = np.random.RandomState(71)
    a, b = _soup(72, 120, 1.0, 0.2), _soup(73, 90, 1.0, 0.2)
    entries = [(k % 2, NQ.random_pose(rng, reflect=bool(k & 1), shift=2.0)) for k in range(9)]
    q = _around(rng, rng.uniform(-3.5, 3.5, (1500, 3)), 10.0 ** rng.uniform(-2, 0.2, (1500, 1, 1))).astype(F)
    with _World(psm, ctx, [a, b], entries) as sc:
        _, before, _, _ = check_tris(sc, q, (4,))
        sc.world.setTransform(3, NQ.random_pose(rng, shift=2.0))
        sc.world.setTransforms(5, [NQ.random_pose(rng, reflect=True, shift=2.0), NQ.random_pose(rng, shift=2.0)])
        _, after, _, _ = check_tris(sc, q, (4, 16))
        assert (before != after).any()
        # a rebuilt member is stale: refused by message
        h = sc.ths[1]
        h.markDirty()
        h.build()
        with pytest.raises(psm.PsmError, match="psm_world_tri_count_dev: instance 1's hierarchy was rebuilt"):
            sc.world.countOnTriangle(q)
        sc.world.setInstances([(sc.ths[k], m) for k, m in zip(sc.which, sc.world.transforms())])
        # a refit: the triangles move within the build's bounds; after refresh() the answers are exact again
        blo, bhi = b.reshape(-1, 3).min(0), b.reshape(-1, 3).max(0)
        moved = b.copy()
        k = rng.choice(b.shape[0], 10, replace=False)
        cc = moved[k].mean(axis=1, keepdims=True)
        moved[k] = np.clip(cc + (moved[k] - cc) * F(0.5) + rng.uniform(-0.3, 0.3, (10, 1, 3)).astype(F), blo, bhi).astype(F)
        h.clearTribuffer()
        h.loadTriangles(moved.reshape(-1, 9))
        h.refit()
        sc.world.refresh()
        sc.meshes[1] = moved
        _, refit, _, _ = check_tris(sc, q, (4, 16))
        assert (refit != after).any()


def test_world_tri_refusals_launch_nothing(psm, ctx):
    """a stale world, k = 0, k = 17, k = 2^31, NULL and misaligned pointers are refused on the host by their messages: the outputs
    keep what they held; then the same buffers succeed at k = 16"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    n = 4
    with _World(psm, ctx, [tri, tri + F(1)], [(0, NQ.IDENTITY), (1, NQ.IDENTITY)]) as sc:
        w = sc.world._w
        hin, hout, hinst, hcnt = ctx.buf_alloc(48 * n + 16), ctx.buf_alloc(4 * 17 * n), ctx.buf_alloc(4 * 17 * n), ctx.buf_alloc(4 * n + 16)
        try:
            packed = np.zeros((n, 3, 4), F)
            packed[:, :, :3] = [[-3, -3, -3], [3, 3, 3], [3.5, 3, -3]]     # through both triangles
            ctx.buf_upload(hin, packed)
            ctx.buf_upload(hout, np.full(17 * n, 7, np.int32))
            ctx.buf_upload(hinst, np.full(17 * n, 9, np.int32))
            ctx.buf_upload(hcnt, np.full(n + 4, 77, U))
            pin, pout, pinst, pcnt = (ctypes.c_void_p(ctx.buf_ptr(h)[0]) for h in (hin, hout, hinst, hcnt))
            size = ctypes.c_size_t(n)

            def tris_call(k, p_in=pin, p_out=pout, p_inst=pinst, p_cnt=pcnt, count=size):
                return lib.psm_world_tri_triangles_dev(w, p_in, count, ctypes.c_uint32(k), p_out, p_inst, p_cnt)

            def flat_call(fn, p_in=pin, p_out=pcnt, count=size):
                return fn(w, p_in, count, p_out)
            for k in (0, 17, 1 << 31):
                assert tris_call(k) == -1
                assert b"psm_world_tri_triangles_dev: k must be 1 .. 16" in lib.psm_last_error(ctx._h)
            assert tris_call(4, p_out=None) == -1 and tris_call(4, p_cnt=None) == -1 and tris_call(4, p_in=None) == -1
            assert tris_call(4, p_inst=None) == -1 and b"psm_world_tri_triangles_dev: NULL pointer" in lib.psm_last_error(ctx._h)
            assert tris_call(4, p_in=ctypes.c_void_p(pin.value + 4)) == -1 and b"triangles not 16-byte aligned" in lib.psm_last_error(ctx._h)
            assert tris_call(4, p_out=ctypes.c_void_p(pout.value + 2)) == -1 and b"tris not 4-byte aligned" in lib.psm_last_error(ctx._h)
            assert tris_call(4, p_inst=ctypes.c_void_p(pinst.value + 2)) == -1 and b"inst not 4-byte aligned" in lib.psm_last_error(ctx._h)
            assert tris_call(4, p_cnt=ctypes.c_void_p(pcnt.value + 2)) == -1 and b"counts not 4-byte aligned" in lib.psm_last_error(ctx._h)
            for fn in (lib.psm_world_tri_overlaps_dev, lib.psm_world_tri_count_dev):
                assert flat_call(fn, p_in=None) == -1 and flat_call(fn, p_out=None) == -1
                assert flat_call(fn, p_in=ctypes.c_void_p(pin.value + 8)) == -1
                assert flat_call(fn, count=ctypes.c_size_t(0)) == 0
            assert flat_call(lib.psm_world_tri_count_dev, p_out=ctypes.c_void_p(pcnt.value + 2)) == -1
            for k in (0, 17):
                with pytest.raises(psm.PsmError, match="k must be 1 .. 16"):
                    sc.world.trianglesOnTriangle(packed[:, :, :3], k)
            sc.ths[1].markDirty()
            sc.ths[1].build()                                          # stale: PSM_ERR_STATE
            assert tris_call(4) == -5 and b"psm_world_tri_triangles_dev: instance 1's hierarchy was rebuilt" in lib.psm_last_error(ctx._h)
            for fn in (lib.psm_world_tri_overlaps_dev, lib.psm_world_tri_count_dev):
                assert flat_call(fn) == -5 and b"instance 1's hierarchy was rebuilt" in lib.psm_last_error(ctx._h)
            ctx.sync()
            assert (ctx.buf_download(hout, np.int32, 17 * n) == 7).all() and (ctx.buf_download(hinst, np.int32, 17 * n) == 9).all()
            assert (ctx.buf_download(hcnt, U, n + 4) == 77).all()
            sc.world.setInstances([(sc.ths[0], NQ.IDENTITY), (sc.ths[1], NQ.IDENTITY)])
            w = sc.world._w
            assert tris_call(16) == 0                                  # and the same buffers are fine at k = 16
            ctx.sync()
            assert (ctx.buf_download(hcnt, U, n) == 2).all()
            rows, irows = ctx.buf_download(hout, np.int32, 17 * n), ctx.buf_download(hinst, np.int32, 17 * n)
            assert (rows[:16 * n].reshape(n, 16) == [0, 0] + [-1] * 14).all() and (rows[16 * n:] == 7).all()
            assert (irows[:16 * n].reshape(n, 16) == [0, 1] + [-1] * 14).all() and (irows[16 * n:] == 9).all()
        finally:
            for h in (hin, hout, hinst, hcnt):
                ctx.buf_free(h)


def test_world_tri_torch_tensors_on_a_side_stream(psm, ctx):
    if torch is None:
        pytest.skip("torch is not installed")
    rng = np.random.RandomState(74)
    entries = [(k % 2, NQ.random_pose(rng, reflect=bool(k & 1), shift=3.0)) for k in range(40)]
    q = _around(rng, rng.uniform(-4, 4, (4099, 3)), 10.0 ** rng.uniform(-2, 0.2, (4099, 1, 1))).astype(F)
    with _World(psm, ctx, [IQ.icosphere(1, 0.6), _soup(75, 150, 0.8, 0.2)], entries) as sc:
        w = sc.world
        flag, count, lists = w.overlapsTriangle(q), w.countOnTriangle(q), w.trianglesOnTriangle(q, 5)
        assert flag.any() and not flag.all()
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            tq = torch.from_numpy(q).to(dev, non_blocking=True)
            gflag, gcount, glists = w.overlapsTriangle(tq), w.countOnTriangle(tq.reshape(-1, 9)), w.trianglesOnTriangle(tq, 5)
            bufs = [x.cpu() for x in (gflag, gcount, glists.tri, glists.geom, glists.count)]   # (on the side stream: in order)
        assert gflag.device == dev and gflag.dtype == torch.bool and gcount.dtype == torch.int32
        assert glists.tri.shape == (4099, 5) and glists.geom.shape == (4099, 5) and glists.geom.dtype == torch.int32
        _same(bufs[0].numpy(), flag, "torch overlapsTriangle")
        _same(bufs[1].numpy().view(U), count, "torch countOnTriangle")
        _same(bufs[2].numpy(), lists.tri, "torch trianglesOnTriangle tri")
        _same(bufs[3].numpy(), lists.geom, "torch trianglesOnTriangle inst")
        _same(bufs[4].numpy().view(U), lists.count, "torch trianglesOnTriangle count")
