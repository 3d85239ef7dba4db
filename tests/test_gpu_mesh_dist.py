"""Mesh clearance on the GPU (psm_bvh_mesh_closest_dev / psm_bvh_mesh_within_dev / psm_bvh_mesh_clearance_dev, mesh_dist.hip;
TriangleHierarchy.meshClosest / meshWithin / meshClearance). Every comparison is exact: meshClosest is
triClosest of the host-posed triangles bit for bit, meshClearance the (dist, t) minimum of meshClosest bit for bit, meshWithin
its predicate, and a pose that meshOverlaps reports is at distance 0 -- on a lattice against the numpy model, on soups under
rotations and reflections, on the ties, at every size where the code takes another path, under every rmax, with the shared
bound forced on and off, under other trees, after refit(), through torch on a side stream; and every refusal leaves the
buffers as they were."""
import ctypes
import os

import numpy as np
import pytest

import mesh_dist_query_model as MD
import mesh_query_model as MQ
import tri_dist_query_model as TD
from test_gpu_mesh_query import GRID_CAP, POINT, ROT_SCALE, SHEAR, _hier, _leaves, _pose, _soup, general_case, lattice_case, lattice_soup, rotations
from test_mesh_dist_cpu import MISS, tie_cases

try:
    import torch
except ImportError:   # pragma: no cover
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32
I = np.int32
U = np.uint32


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.size == 0:
        return
    bad = np.nonzero((a.view(U) != b.view(U)).reshape(a.shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, "%s: %d poses differ, first %d" % (what, bad.size, bad[0])


def reduce(hits):
    """MD.reduce, vectorised: the (dist, t) minimum of [p, T, 8] records, t in slot 6"""
    p, t = hits.shape[:2]
    out = TD.miss_records(p)
    out.view(I)[:, 6] = -1
    if t == 0:
        return out
    key = (hits[:, :, 2].view(U).astype(np.uint64) << np.uint64(32)) | np.arange(t, dtype=np.uint64)[None]
    key[hits.view(I)[:, :, 3] < 0] = np.uint64(MD.NONE)
    best = key.argmin(axis=1)
    found = key[np.arange(p), best] != np.uint64(MD.NONE)
    out[found] = hits[np.arange(p), best][found]
    out.view(I)[found, 6] = best[found]
    return out


def check(psm, th, tris, other, otris, poses, rmax=np.inf, model=False):
    """the three queries at one rmax against triClosest of the host-posed triangles, against one another and against
    meshOverlaps; with `model` against the numpy model too. Returns (closest [p, T, 8], clearance [p, 8], within [p])"""
    p, t = MQ.poses12(poses).shape[0], np.asarray(otris).reshape(-1, 9).shape[0]
    oleaves = np.sort(_leaves(psm, other))
    want = TD.miss_records(p * t).reshape(p, t, 8)
    if oleaves.size and p:
        q = MQ.posed(otris, poses)[:, oleaves].reshape(-1, 3, 3)
        want[:, oleaves] = th.triClosest(q, rmax).buffer.reshape(p, oleaves.size, 8)
    got = th.meshClosest(other, poses, rmax)
    assert isinstance(got, psm.QueryMeshHits) and got.other is None and got.buffer.shape == (p, t, 8) and got.buffer.dtype == F
    assert got.tri.shape == (p, t) and got.tri.dtype == I
    _bits(got.buffer, want, "meshClosest against triClosest")
    pair = th.meshClearance(other, poses, rmax)
    assert pair.buffer.shape == (p, 8) and pair.other.dtype == I and pair.other.shape == (p,)
    _bits(pair.buffer, reduce(got.buffer), "meshClearance against the minimum of meshClosest")
    within = th.meshWithin(other, poses, rmax)
    assert within.shape == (p,) and within.dtype == np.bool_ and np.array_equal(within, pair.tri >= 0)
    assert np.array_equal(pair.tri >= 0, pair.other >= 0) and (pair.buffer[:, 7] == 0).all()
    with np.errstate(invalid="ignore"):
        if rmax >= 0:
            cut = th.meshOverlaps(other, poses)
            assert (pair.dist[cut] == 0).all() and within[cut].all()                # meshOverlaps => dist == 0
    if model:
        hits, rec, flag = MD.query(tris, _leaves(psm, th), otris, oleaves, poses, rmax)
        _bits(got.buffer, hits, "meshClosest against the model")
        _bits(pair.buffer, rec, "meshClearance against the model")
        assert np.array_equal(within, flag)
    return got.buffer, pair.buffer, within


def test_mesh_dist_lattice_against_the_model(psm, ctx):
    tris, otris, poses = lattice_case()
    th, other = _hier(psm, ctx, tris), _hier(psm, ctx, otris)
    try:
        assert other.info().leaf_count == 130 and otris.shape[0] == 131 and tris.shape[0] == 500 and len(poses) == 6
        hits, rec, within = check(psm, th, tris, other, otris, poses, model=True)
        assert within.all() and (rec[:, 2] == 0).sum() >= 3 and (rec[:, 2] > 1).sum() >= 2
        assert (hits.view(I)[:, 130, 3] == -1).all() and np.isinf(hits[:, 130, 2]).all()       # the dropped triangle, at every pose
        _, rec2, within2 = check(psm, th, tris, other, otris, poses, 0.125, model=True)
        assert within2.sum() >= 3 and (~within2).sum() >= 2
        assert [list(r[:3]) + [r.view(I)[3]] + list(r[4:6]) + [r.view(I)[6], r[7]] for r in rec2[~within2]] == [MISS] * int((~within2).sum())
        # the witness points are dist apart
        pair = th.meshClearance(other, poses)
        a, b = pair.points(tris, otris, poses)
        assert np.allclose(np.linalg.norm(a - b, axis=1), pair.dist, atol=1e-5)
    finally:
        th.close()
        other.close()


def test_mesh_dist_soup_under_rotations_and_reflections(psm, ctx):
    tris, otris, poses = general_case()
    th, other = _hier(psm, ctx, tris), _hier(psm, ctx, otris)
    try:
        hits, rec, within = check(psm, th, tris, other, otris, poses)
        assert within.all() and (rec[:, 2] == 0).sum() >= 5 and (rec[:, 2] > 0).sum() >= 1
        assert (hits[:, :, 2] > 0).sum() > 500
        # a 4 x 4 matrix, and one pose alone: its row of the batch
        m44 = np.concatenate([poses[7], [[0, 0, 0, 1]]])
        _bits(th.meshClearance(other, m44).buffer, rec[7:8], "one 4 x 4 pose")
        _bits(th.meshClosest(other, np.stack([np.concatenate([m, [[0, 0, 0, 1]]]) for m in poses])).buffer, hits, "[p, 4, 4] poses")
        # apart: the other mesh shrunk into a gap beside the soup, so that most poses have a positive clearance
        far = [_pose(m[:, :3], m[:, 3] + [2.5, 0, 0]) for m in poses]
        _, rec3, within3 = check(psm, th, tris, other, otris, far)
        assert (rec3[:, 2] > 0).all() and within3.all()
        _, _, within4 = check(psm, th, tris, other, otris, far, float(np.median(rec3[:, 2])))
        assert within4.any() and not within4.all()
    finally:
        th.close()
        other.close()


def test_mesh_dist_self_query(psm, ctx):
    """other == bvh at the identity: every leaf is at distance 0 of itself, and the pose's pair is (the lowest leaf, itself or a
    lower-numbered triangle that meets it)"""
    rng = np.random.RandomState(72)
    tris = np.concatenate([POINT, lattice_soup(7, 200), (rng.uniform(-1, 1, (600, 1, 3)) + rng.uniform(-0.08, 0.08, (600, 3, 3))).astype(F)])
    th = _hier(psm, ctx, tris)
    try:
        leaves = np.sort(_leaves(psm, th))
        assert 0 not in leaves and leaves.size == 800
        hits, rec, within = check(psm, th, tris, th, tris, np.eye(3, 4))
        assert (hits[0, leaves, 2] == 0).all() and (hits.view(I)[0, leaves, 3] <= leaves).all() and hits.view(I)[0, 0, 3] == -1
        assert within[0] and rec[0, 2] == 0 and rec.view(I)[0, 6] == 1 and rec.view(I)[0, 3] <= 1
    finally:
        th.close()


@pytest.mark.parametrize("case", tie_cases(), ids=lambda c: c[0])
def test_mesh_dist_ties(psm, ctx, case):
    name, tris, otris, poses, (tri, other_id) = case
    th, other = _hier(psm, ctx, tris), _hier(psm, ctx, otris)
    try:
        assert th.info().leaf_count == tris.shape[0] and other.info().leaf_count == (2 if name == "dropped" else otris.shape[0])
        for bound in ("1", "0"):
            os.environ["PSM_MESH_BOUND"] = bound
            try:
                _, rec, _ = check(psm, th, tris, other, otris, poses, model=True)
            finally:
                del os.environ["PSM_MESH_BOUND"]
            assert list(rec.view(I)[:, 3]) == [tri, tri] and list(rec.view(I)[:, 6]) == [other_id, other_id] and list(rec[:, 2]) == [0.5, 0.75]
    finally:
        th.close()
        other.close()


@pytest.mark.parametrize("leaves", [0, 1, 63, 65])
@pytest.mark.parametrize("p", [1, 3])
def test_mesh_dist_other_sizes(psm, ctx, leaves, p):
    rng = np.random.RandomState(100 * leaves + p)
    tris = _soup(np.random.RandomState(73), 200, 0.2)
    otris = np.concatenate([_soup(rng, leaves // 2, 0.2), POINT, _soup(rng, leaves - leaves // 2, 0.2)])   # a dropped triangle among them
    poses = [_pose(r, t) for r, t in zip(rotations(rng, p), rng.uniform(-0.3, 0.3, (p, 3)))]
    th, other = _hier(psm, ctx, tris), _hier(psm, ctx, otris)
    try:
        assert other.info().leaf_count == leaves
        hits, rec, within = check(psm, th, tris, other, otris, poses)
        assert (hits.view(I)[:, leaves // 2, 3] == -1).all() and within.all() == (leaves > 0) and within.any() == (leaves > 0)
        check(psm, th, tris, other, otris, poses, 0.01)
    finally:
        th.close()
        other.close()


def test_mesh_dist_tiny_hierarchies(psm, ctx):
    """bvh with 0, 1, 2 and 3 leaves (no tree, the lone leaf, the smallest trees), and an other without leaves"""
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    degenerate = np.repeat(tri[:, :1], 3, axis=1)
    rng = np.random.RandomState(74)
    otris = np.concatenate([_soup(rng, 70, 0.8) + F([0.7, 0, 0]), F([[[-4, -0.5, -0.25], [4, -0.5, -0.25], [4, 0.5, 0.5]]])])   # the last: through all
    poses = [np.eye(3, 4), _pose(rotations(rng, 1)[0], [0.1, 0, 0]), _pose(np.eye(3), [30, 0, 0])]
    other = _hier(psm, ctx, otris)
    empty = _hier(psm, ctx, np.concatenate([degenerate] * 4))
    try:
        assert empty.info().leaf_count == 0
        for tris, leaves in ((np.concatenate([degenerate] * 4), 0), (np.concatenate([degenerate, tri, degenerate]), 1),
                             (np.concatenate([tri, degenerate, tri + F([0.5, 0, 0])]), 2),
                             (np.concatenate([tri, tri + F([0.25, 0, 0]), degenerate, tri + F([0.5, 0, 0])]), 3)):
            th = _hier(psm, ctx, tris)
            try:
                assert th.info().leaf_count == leaves
                for rmax in (np.inf, 1.0):
                    hits, rec, within = check(psm, th, tris, other, otris, poses, rmax, model=True)
                    assert within[:2].all() == (leaves > 0) and within[2] == (leaves > 0 and rmax > 1)
                _, rec0, within0 = check(psm, th, tris, empty, np.concatenate([degenerate] * 4), poses)   # a mesh without leaves: a miss
                assert not within0.any() and (rec0.view(I)[:, [3, 6]] == -1).all()
            finally:
                th.close()
    finally:
        other.close()
        empty.close()


@pytest.mark.parametrize("rmax", [0.0, 0.02, np.inf, np.nan, -1.0])
def test_mesh_dist_rmax(psm, ctx, rmax):
    tris, otris, poses = general_case()
    tris, otris = tris[:600], otris[:100]
    poses = poses[:3] + [_pose(m[:, :3], m[:, 3] + [2.2, 0, 0]) for m in poses[:3]]
    th, other = _hier(psm, ctx, tris), _hier(psm, ctx, otris)
    try:
        hits, rec, within = check(psm, th, tris, other, otris, poses, rmax)
        if not rmax >= 0:                                                        # NaN, negative: a miss everywhere, no refusal
            assert not within.any() and (hits.view(I)[:, :, 3] == -1).all() and (rec.view(I)[:, [3, 6]] == -1).all() and np.isinf(rec[:, 2]).all()
        elif rmax == np.inf:
            assert within.all() and (rec[3:, 2] > 0).all()
        else:
            assert within[:3].all() and not within[3:].any() and (rec[within, 2] <= F(rmax)).all()
    finally:
        th.close()
        other.close()


def test_mesh_dist_grid_stride_second_trip(psm, ctx):
    """p x L just above PSM_QUERY_GRID_CAP x 64 + 65: the last queries take a second trip of the grid-stride loop, where the
    lane's best, its bound, its read of the word and its retirement must start clean again"""
    rng = np.random.RandomState(75)
    tris = _soup(np.random.RandomState(76), 16, 0.6)
    otris = np.concatenate([_soup(rng, 30, 0.5), POINT, _soup(rng, 35, 0.5)])
    leaves = 65
    p = -(-(GRID_CAP * 64 + 65) // leaves)
    assert GRID_CAP * 64 + 65 <= p * leaves < GRID_CAP * 64 + 65 + leaves
    poses = np.concatenate([rotations(rng, p), rng.uniform(-0.8, 0.8, (p, 3, 1))], axis=2)
    poses[-1, :, 3] += 2.5                                                   # the last pose, walked on the second trip: apart
    th, other = _hier(psm, ctx, tris), _hier(psm, ctx, otris)
    try:
        assert other.info().leaf_count == leaves
        hits, rec, within = check(psm, th, tris, other, otris, poses)
        assert within.all() and (rec[:, 2] == 0).any() and rec[-1, 2] > 0 and len(np.unique(rec[-3:, 2])) >= 2
        _, _, w2 = check(psm, th, tris, other, otris, poses, 0.05)
        assert w2.any() and not w2[-1]
    finally:
        th.close()
        other.close()


def test_mesh_dist_sharing_changes_no_record(psm, ctx):
    """PSM_MESH_BOUND forced to 1, 1, 0 (and the two variants between them): what the lanes see of one another depends on
    timing, the records do not"""
    tris, otris, poses = general_case()
    poses = poses + [_pose(m[:, :3], m[:, 3] + [2.3, 0.1, 0]) for m in poses]
    th, other = _hier(psm, ctx, tris), _hier(psm, ctx, otris)
    try:
        want = reduce(th.meshClosest(other, poses).buffer)
        assert (want[:, 2] == 0).sum() >= 5 and (want[:, 2] > 0).sum() >= 8
        for bound in ("1", "1", "0", "2", "3"):
            os.environ["PSM_MESH_BOUND"] = bound
            try:
                _bits(th.meshClearance(other, poses).buffer, want, "PSM_MESH_BOUND = " + bound)
                _bits(th.meshClearance(other, poses, 0.3).buffer, reduce(th.meshClosest(other, poses, 0.3).buffer), "rmax 0.3, PSM_MESH_BOUND = " + bound)
            finally:
                del os.environ["PSM_MESH_BOUND"]
        for skip in ("1", "1", "0"):
            os.environ["PSM_MESH_SKIP"] = skip
            try:
                assert np.array_equal(th.meshWithin(other, poses, 0.3), want[:, 2] <= F(0.3)), skip
            finally:
                del os.environ["PSM_MESH_SKIP"]
    finally:
        th.close()
        other.close()


def test_mesh_dist_answers_do_not_depend_on_the_trees(psm, ctx):
    """both hierarchies rebuilt under a rotating and a shearing optimisation matrix, and refitted: the same records"""
    tris, otris, poses = general_case()
    tris, otris = tris[:800], otris[:150]
    poses = poses[:3] + [_pose(m[:, :3], m[:, 3] + [2.3, 0, 0]) for m in poses[:3]]
    th, plain = _hier(psm, ctx, tris), _hier(psm, ctx, otris)
    try:
        hits, rec, within = check(psm, th, tris, plain, otris, poses)
        near = float(np.sort(rec[:, 2])[4])
        for opt in (ROT_SCALE, SHEAR):
            other, th2 = _hier(psm, ctx, otris, opt), _hier(psm, ctx, tris, opt)
            try:
                for a, b, what in ((th, other, "other"), (th2, plain, "the queried hierarchy"), (th2, other, "both")):
                    _bits(a.meshClosest(b, poses).buffer, hits, "meshClosest under an optimisation matrix of " + what)
                    _bits(a.meshClearance(b, poses).buffer, rec, "meshClearance under an optimisation matrix of " + what)
                    assert np.array_equal(a.meshWithin(b, poses, near), rec[:, 2] <= F(near)), what
                for x, t in ((other, otris), (th2, tris)):
                    x.clearTribuffer()
                    x.loadTriangles(t.reshape(-1, 9))
                    x.refit()
                _bits(th2.meshClosest(other, poses).buffer, hits, "meshClosest after refit()")
                _bits(th2.meshClearance(other, poses).buffer, rec, "meshClearance after refit()")
                assert np.array_equal(th2.meshWithin(other, poses, near), rec[:, 2] <= F(near))
            finally:
                other.close()
                th2.close()
    finally:
        th.close()
        plain.close()


def test_mesh_dist_torch_tensors_on_a_side_stream(psm, ctx):
    if torch is None:
        pytest.skip("torch is not installed")
    tris, otris, poses = general_case()
    th, other = _hier(psm, ctx, tris), _hier(psm, ctx, otris)
    try:
        hits, pair, within = th.meshClosest(other, poses, 0.4), th.meshClearance(other, poses, 0.4), th.meshWithin(other, poses, 0.01)
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            ghits, gpair = th.meshClosest(other, poses, 0.4, as_torch=True), th.meshClearance(other, poses, 0.4, as_torch=True)
            gwithin = th.meshWithin(other, poses, 0.01, as_torch=True)
            least = ghits.dist.min(dim=1).values                                  # (torch work on the side stream: in order)
            bufs = [x.cpu() for x in (ghits.buffer, gpair.buffer, gwithin, least, gpair.other, ghits.tri)]
        assert ghits.buffer.device == dev and ghits.buffer.shape == (8, 300, 8) and ghits.other is None and ghits.tri.dtype == torch.int32
        assert gpair.buffer.shape == (8, 8) and gpair.other.dtype == torch.int32 and gwithin.dtype == torch.bool and gwithin.shape == (8,)
        _bits(bufs[0].numpy(), hits.buffer, "torch meshClosest")
        _bits(bufs[1].numpy(), pair.buffer, "torch meshClearance")
        assert np.array_equal(bufs[2].numpy(), within) and np.array_equal(bufs[3].numpy(), pair.dist)
        assert np.array_equal(bufs[4].numpy(), pair.other) and np.array_equal(bufs[5].numpy(), hits.tri)
    finally:
        th.close()
        other.close()


def test_mesh_dist_refusals_launch_nothing(psm, ctx):
    """a call before either build, NULL and misaligned pointers, poses that are not finite or not rigid and hierarchies of two
    contexts are refused on the host under the mesh queries' texts: the outputs keep what they held"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    through = F([[[0, 0, -2], [2, 0, 2], [2, 1, 2]], [[0, 0.25, -2], [2, 0.25, 2], [2, 1.25, 2]]])
    th, other = psm.TriangleHierarchy(ctx), psm.TriangleHierarchy(ctx)
    th.allocate(4)
    th.loadTriangles(tri.reshape(1, 9))
    other.allocate(4)
    other.loadTriangles(through.reshape(2, 9))
    ctx2 = psm.Context(0)
    foreign = None
    p, t = 3, 2
    words = 8 * p * t + 8
    hout = ctx.buf_alloc(4 * words)
    try:
        ctx.buf_upload(hout, np.full(words, 7, np.int32))
        pout = ctypes.c_void_p(ctx.buf_ptr(hout)[0])
        good = np.ascontiguousarray(np.tile(np.eye(3, 4, dtype=F).reshape(1, 12), (p, 1)))
        size = ctypes.c_size_t(p)
        err = lambda: lib.psm_last_error(ctx._h)
        fns = {s: getattr(lib, s) for s in ("psm_bvh_mesh_closest_dev", "psm_bvh_mesh_within_dev", "psm_bvh_mesh_clearance_dev")}

        def call(fn, a=th, b=other, m=good, p_out=pout, count=size, rmax=1.0):
            return fn(None if a is None else a._h, None if b is None else b._h, None if m is None else m.ctypes.data_as(ctypes.c_void_p), count,
                      ctypes.c_float(rmax), p_out)
        for fn in fns.values():
            assert call(fn) == -5 and b"mesh query before build" in err()         # neither is built: PSM_ERR_STATE
            assert call(fn, count=ctypes.c_size_t(0)) == 0                         # p = 0 is answered first
        th.build()
        for fn in fns.values():
            assert call(fn) == -5 and b"mesh query before build" in err()         # other is not built
            assert call(fn, a=other, b=th) == -5 and b"mesh query before build" in err()   # the queried one is not built
        other.build()
        scaled, nan = good.copy(), good.copy()
        scaled[1, [0, 5, 10]] = 1.01                                              # pose 1 scaled by 1.01
        nan[2, 7] = np.nan
        foreign = psm.TriangleHierarchy(ctx2)                                     # a built hierarchy of another context
        foreign.allocate(4)
        foreign.loadTriangles(through.reshape(2, 9))
        foreign.build()
        ctx2.sync()
        for name, fn in fns.items():
            assert call(fn, m=None) == -1 and (name + ": NULL pointer").encode() in err()
            assert call(fn, p_out=None) == -1 and (name + ": NULL pointer").encode() in err()
            assert call(fn, a=None) == -1 and call(fn, b=None) == -1
            assert call(fn, a=None, count=ctypes.c_size_t(0)) == -1               # ... before p == 0 is answered
            if "within" not in name:
                assert call(fn, p_out=ctypes.c_void_p(pout.value + 8)) == -1 and (name + ": hits not 16-byte aligned").encode() in err()
            assert call(fn, m=scaled) == -1 and (name + ": pose 1 has a transform that is not rigid").encode() in err()
            assert call(fn, m=nan) == -1 and (name + ": pose 2 has a non-finite transform").encode() in err()
            assert call(fn, b=foreign) == -1 and (name + ": the two hierarchies are of different contexts").encode() in err()
        ctx.sync()
        assert (ctx.buf_download(hout, np.int32, words) == 7).all()
        with pytest.raises(ValueError):
            th.meshClearance(other, scaled.reshape(p, 3, 4))
        with pytest.raises(psm.PsmError, match="different contexts"):
            th.meshClosest(foreign, good.reshape(p, 3, 4))
        # NaN and a negative rmax are no refusals: misses, written
        assert call(fns["psm_bvh_mesh_clearance_dev"], rmax=float("nan")) == 0
        ctx.sync()
        got = ctx.buf_download(hout, np.int32, words)
        assert (got[8 * p:] == 7).all() and (got[:8 * p].reshape(p, 8)[:, [3, 6]] == -1).all()
        assert call(fns["psm_bvh_mesh_closest_dev"]) == 0                          # and the same buffer is fine for a real call
        ctx.sync()
        got = ctx.buf_download(hout, np.int32, words)
        assert (got[8 * p * t:] == 7).all() and (got[:8 * p * t].reshape(p * t, 8)[:, 3] == 0).all()
        before = ctx.buf_download(hout, np.uint8, 4 * words)
        assert call(fns["psm_bvh_mesh_within_dev"]) == 0                           # p bytes, and not one more
        ctx.sync()
        after = ctx.buf_download(hout, np.uint8, 4 * words)
        assert after[:p].tolist() == [1] * p and np.array_equal(after[p:], before[p:]) and before[:p].tolist() != [1] * p
    finally:
        ctx.buf_free(hout)
        th.close()
        other.close()
        if foreign is not None:
            foreign.close()
        ctx2.close()
