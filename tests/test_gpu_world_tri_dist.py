"""The clearance queries of an instance world on the GPU (psm_world_tri_closest_dev / psm_world_tri_within_dev,
world_tri_dist.hip; InstanceWorld.closestToTriangle / withinOfTriangle). The yardstick is
tests/world_tri_dist_query_model.py part (a): tri_dist in numpy float32 over the forward-posed downloaded leaves of every
instance, the smallest d2 and on a bit-equal d2 the lowest (instance, triangle). Every comparison is exact on every query, and in
every case the queries are also held against one another and against the world's own overlapsTriangle()."""
import numpy as np
import pytest

import instance_query_model as NQ
import tri_dist_query_model as TD
import world_box_query_model as WB
import world_tri_dist_query_model as WD
from test_gpu_box_query import GRID_CAP
from test_gpu_world_box import _World
from test_world_box_cpu import _edge_pose, cube
from test_world_tri_cpu import posed_triangles

try:   # (imported before the library loads its HIP runtime, as tests/test_gpu_query.py)
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64


def _same(a, b, what):
    """bit for bit (a float32 array by its words: -0 and +0 differ, a NaN equals itself)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    ua, ub = (x.view(np.uint32) if x.dtype == F else x for x in (a, b))
    bad = np.nonzero(np.atleast_1d((ua != ub).reshape(a.shape[0], -1).any(axis=1)))[0]
    assert bad.size == 0, "%s: %d differ, first %d: %s against %s" % (what, bad.size, bad[0], a[bad[0]], b[bad[0]])


def torus(nu=16, nv=8, major=1.0, minor=0.35):
    """a torus around the z axis, 2 nu nv = 256 triangles"""
    u, v = np.arange(nu + 1) * (2 * np.pi / nu), np.arange(nv + 1) * (2 * np.pi / nv)

    def at(i, j):
        return np.array([(major + minor * np.cos(v[j])) * np.cos(u[i]), (major + minor * np.cos(v[j])) * np.sin(u[i]), minor * np.sin(v[j])])
    t = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            t += [[a, b, c], [a, c, d]]
    return np.array(t, F)


ONE = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
EMPTY = np.repeat(ONE[:, :1], 3, axis=1).repeat(4, axis=0)           # three equal vertices each: the build keeps no leaf
COINCIDENT, EDGE = (5, 17), 7


def meshes():
    return [cube(), torus(), ONE, EMPTY]


def entries(n):
    """(mesh, pose) of a world of n instances: 1 the torus, 2 the cube and the torus, 24 all four meshes -- instance 17 lies
    exactly on instance 5 (the same torus at the same pose) and instance 7 has a pose at the edge of the pose check"""
    rng = np.random.RandomState(70 + n)
    if n == 1:
        return [(1, NQ.random_pose(rng, shift=1.0))]
    if n == 2:
        return [(0, NQ.random_pose(rng, shift=1.0)), (1, NQ.random_pose(rng, reflect=True, shift=1.0))]
    kinds = [0, 1, 0, 2, 0, 1, 3, 0, 0, 1, 0, 2, 0, 1, 3, 0, 0, 1, 0, 2, 0, 1, 0, 0]
    out = [(k, NQ.random_pose(rng, reflect=bool(i & 1), shift=3.0)) for i, k in enumerate(kinds[:n])]
    out[EDGE] = (out[EDGE][0], _edge_pose(rng, rng.uniform(-3, 3, 3)))
    out[COINCIDENT[1]] = (out[COINCIDENT[0]][0], out[COINCIDENT[0]][1].copy())
    return out


def queries(seed, insts, total):
    """world triangles and their rmax: [0, 8) invalid (six with a non-finite coordinate, one rmax NaN, one negative); then per
    instance with leaves (up to 16 of them) 4 posed copies of stored triangles, 2 points on posed vertices and 2 segments along
    posed edges; the rest over three decades of size around points near posed vertices or anywhere in the world. rmax: a third
    +inf, a third 0, the rest over three decades"""
    rng = np.random.RandomState(seed)
    live = [i for i in insts if len(i[1])]
    centre = rng.uniform(-4.5, 4.5, (total, 3))
    for i in range(1, total, 2):                                           # every second one near a posed vertex
        inst = live[rng.randint(len(live))]
        one = rng.randint(len(inst[1]))
        centre[i] = posed_triangles((inst[0], inst[1][one:one + 1], inst[2]))[0, 0] + rng.normal(size=3) * 10.0 ** rng.uniform(-3, 0)
    q = (centre[:, None, :] + rng.normal(size=(total, 3, 3)) * 10.0 ** rng.uniform(-3, 0, (total, 1, 1))).astype(F)
    rm = (10.0 ** rng.uniform(-3, 0, total)).astype(F)
    rm[::3] = np.inf
    rm[1::3] = 0
    at = 8
    for inst in live[:16]:
        if at + 8 > total:
            break
        t = posed_triangles((inst[0], np.sort(inst[1])[:4], inst[2])).astype(F)
        t = np.concatenate([t] * 4)[:4]
        q[at:at + 4] = t
        q[at + 4:at + 6] = t[:2, :1]
        q[at + 6:at + 8] = np.stack([t[:2, 0], t[:2, 1], t[:2, 1]], axis=1)
        at += 8
    q[0, 0, 0], q[1, 1, 1], q[2, 2, 2], q[3, 0, 2], q[4, 1, 0] = np.nan, np.nan, np.inf, np.inf, -np.inf
    q[5] = np.nan
    rm[:8] = np.inf
    rm[6], rm[7] = np.nan, -1.0
    return q, rm


def check(sc, q, rm, insts=None):
    """closestToTriangle and withinOfTriangle against (a), against one another and against overlapsTriangle; returns (a)"""
    w = sc.world
    n = q.shape[0]
    hits, inst, within = WD.flat_near(sc.insts() if insts is None else insts, q, rm)
    got = w.closestToTriangle(q, rm)
    assert got.buffer.shape == (n, 8) and got.buffer.dtype == F and got.geom.shape == (n,) and got.geom.dtype == np.int32
    _same(got.buffer, hits, "closestToTriangle records")
    _same(got.geom, inst, "closestToTriangle instances")
    flags = w.withinOfTriangle(q.reshape(-1, 9), rm)
    assert flags.shape == (n,) and flags.dtype == np.bool_
    _same(flags, within, "withinOfTriangle")
    assert np.array_equal(flags, got.tri >= 0) and np.array_equal(got.geom >= 0, got.tri >= 0)
    assert not got.buffer[:, 6:].any() and np.isinf(got.dist[got.tri < 0]).all()
    # dist == 0 exactly where the world's own triangle query counts a pair (rmax = +inf: every valid query has its nearest)
    free = w.closestToTriangle(q)
    assert np.array_equal(free.dist == 0, w.overlapsTriangle(q))
    return hits, inst, within


@pytest.mark.parametrize("n,total", [(1, 600), (2, 600), (24, 4000)])
def test_world_clearance_is_the_flat_answer(psm, ctx, n, total):
    ms, ent = meshes(), entries(n)
    with _World(psm, ctx, ms, ent) as sc:
        assert [th.info().leaf_count for th in sc.ths] == [12, 256, 1, 0]
        insts = sc.insts()
        q, rm = queries(80 + n, insts, total)
        hits, inst, within = check(sc, q, rm, insts)
        dist = hits[:, 2]
        valid = np.arange(total) >= 8
        assert not within[:8].any()                                                     # the invalid queries
        assert (~within & valid).sum() > 50 and (within & (dist > 0)).sum() > 50 and (dist == 0).sum() > 50
        assert within[valid & np.isinf(rm)].all()
        if n == 24:
            # ties broken by the instance: the winners on instance 5 tie with its coincident twin, 17, bit for bit
            on = np.nonzero(inst == COINCIDENT[0])[0]
            assert on.size > 20 and not (inst == COINCIDENT[1]).any() and (inst == EDGE).any()
            h2, i2, _ = WD.flat_near([insts[COINCIDENT[1]]], q[on], rm[on])          # the twin alone holds the same record
            _same(h2, hits[on], "the twin's records")
            assert (i2 == 0).all() and (hits[on, 2] > 0).any()
            # a winner that lies in an instance other than the first the walk enters (the walk restated: model (b))
            some = np.nonzero(valid & within)[0][:200]
            full = [(i[0], i[1], i[2], WB.plain_fit(i[0])) for i in insts if len(i[1])]
            index = [j for j, i in enumerate(insts) if len(i[1])]
            (hb, gb), entered, _ = WD.TriDistWorld(full).closest(q[some], rm[some])
            _same(hb, hits[some], "the walk restated")
            assert np.array_equal(np.array(index)[gb], inst[some])
            assert sum(1 for e, g in zip(entered, gb) if e[0] != g) > 5


@pytest.mark.parametrize("n", [70, 130, GRID_CAP * 64 + 70])
def test_world_clearance_batch_sizes(psm, ctx, n):
    """a partial last wave; the last size takes a second trip of the grid-stride loop: the record must start empty again"""
    ms, ent = meshes(), entries(24)
    if n > 1000:                                              # a world of two single triangles, 4096 distinct queries repeated
        ent = [(2, e[1]) for e in ent[:2]]
    with _World(psm, ctx, ms, ent) as sc:
        insts = sc.insts()
        q, rm = queries(90, insts, min(n, 4096))
        if n > 1000:
            w = sc.world
            hits, inst, within = WD.flat_near(insts, q, rm)
            reps = -(-n // 4096)
            Q, RM = np.concatenate([q] * reps)[:n], np.concatenate([rm] * reps)[:n]
            got = w.closestToTriangle(Q, RM)
            _same(got.buffer, np.concatenate([hits] * reps)[:n], "records")
            _same(got.geom, np.concatenate([inst] * reps)[:n], "instances")
            _same(w.withinOfTriangle(Q, RM), np.concatenate([within] * reps)[:n], "within")
        else:
            hits, inst, within = check(sc, q, rm, insts)
        assert within[-60:].any() and not within[-60:].all() and len(np.unique(inst[-60:])) > 1


def test_identity_world_of_one_is_the_hierarchy_s_own_answer(psm, ctx):
    tris = torus()
    with _World(psm, ctx, [tris], [(0, NQ.IDENTITY)]) as sc:
        q, rm = queries(92, sc.insts(), 1500)
        th, w = sc.ths[0], sc.world
        a, b = w.closestToTriangle(q, rm), th.triClosest(q, rm)
        _same(a.buffer, b.buffer, "records")
        assert b.geom is None and np.array_equal(a.geom, np.where(b.tri >= 0, 0, -1))
        _same(w.withinOfTriangle(q, rm), th.triWithin(q, rm), "within")
        assert (b.tri >= 0).sum() > 100 and (b.tri < 0).sum() > 100 and (b.dist == 0).sum() > 20


def test_tiny_members_and_the_empty_world(psm, ctx):
    ms = meshes()
    with _World(psm, ctx, ms, [(3, NQ.IDENTITY), (2, NQ.IDENTITY), (3, NQ.IDENTITY)]) as sc:
        insts = sc.insts()
        q, rm = queries(93, insts, 300)
        hits, inst, within = check(sc, q, rm, insts)                         # empty hierarchies beside a one-leaf one
        assert within.any() and (inst[within] == 1).all()
        for one in (2, 3):                                                   # worlds of one: no tree
            sc.world.setInstances([(sc.ths[one], NQ.IDENTITY)])
            sc.which = [one]
            _, _, w1 = check(sc, q, rm, sc.insts())
            assert w1.any() == (one == 2)
        sc.world.setInstances([])                                            # the empty world answers without a walk
        sc.which = []
        got = sc.world.closestToTriangle(q, rm)
        _same(got.buffer, TD.miss_records(300), "empty world")
        assert (got.geom == -1).all() and not sc.world.withinOfTriangle(q, rm).any()
        none = sc.world.closestToTriangle(np.zeros((0, 3, 3), F))
        assert len(none) == 0 and none.geom.shape == (0,)


def test_set_transform_is_stale_until_refresh(psm, ctx):
    """a rebuilt member is refused by message and the outputs keep what they held; a moved instance answers anew"""
    rng = np.random.RandomState(94)
    with _World(psm, ctx, meshes(), entries(2)) as sc:
        insts = sc.insts()
        q, rm = queries(95, insts, 500)
        before, _, _ = check(sc, q, rm, insts)
        sc.world.setTransform(1, NQ.random_pose(rng, shift=2.0))
        after, _, _ = check(sc, q, rm)
        assert (before.view(np.uint32) != after.view(np.uint32)).any()
        h = sc.ths[1]
        h.markDirty()
        h.build()
        with pytest.raises(psm.PsmError, match="psm_world_tri_closest_dev: instance 1's hierarchy was rebuilt"):
            sc.world.closestToTriangle(q, rm)
        with pytest.raises(psm.PsmError, match="psm_world_tri_within_dev: instance 1's hierarchy was rebuilt"):
            sc.world.withinOfTriangle(q, rm)
        sc.world.setInstances([(sc.ths[k], m) for k, m in zip(sc.which, sc.world.transforms())])
        again, _, _ = check(sc, q, rm)
        _same(again, after, "after the instances were set again")
        # a refit: the torus shrinks within its build's bounds; stale boxes until refresh(), then the right answer
        small = (sc.meshes[1] * F(0.5)).astype(F)
        h.clearTribuffer()
        h.loadTriangles(small.reshape(-1, 9))
        h.refit()
        sc.world.refresh()
        sc.meshes[1] = small
        refit, _, _ = check(sc, q, rm)
        assert (refit.view(np.uint32) != after.view(np.uint32)).any()


def test_world_clearance_torch_tensors_on_a_side_stream(psm, ctx):
    if torch is None:
        pytest.skip("torch is not installed")
    with _World(psm, ctx, meshes(), entries(24)) as sc:
        q, rm = queries(96, sc.insts(), 2051)
        w = sc.world
        hits, flags = w.closestToTriangle(q, rm), w.withinOfTriangle(q, rm)
        assert flags.any() and not flags.all()
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
            tq, trm = (torch.from_numpy(x).to(dev, non_blocking=True) for x in (q, rm))
            gh, gf = w.closestToTriangle(tq, trm), w.withinOfTriangle(tq.reshape(-1, 9), trm)
            bufs = [x.cpu() for x in (gh.buffer, gh.geom, gf, gh.tri)]          # (on the side stream: in order)
        assert gh.buffer.device == dev and gh.geom.dtype == torch.int32 and gf.dtype == torch.bool
        _same(bufs[0].numpy(), hits.buffer, "torch closestToTriangle records")
        _same(bufs[1].numpy(), hits.geom, "torch closestToTriangle instances")
        _same(bufs[2].numpy(), flags, "torch withinOfTriangle")
        _same(bufs[3].numpy(), hits.tri, "torch tri view")
