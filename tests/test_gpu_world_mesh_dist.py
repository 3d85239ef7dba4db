"""Mesh clearance over an instance world on the GPU (psm_world_mesh_closest_dev / psm_world_mesh_within_dev /
psm_world_mesh_clearance_dev, world_mesh_dist.hip; InstanceWorld.closestToMesh / withinOfMesh / clearanceToMesh).
The yardstick is the contract's own statement: closestToMesh's records and instances are, bit for bit, the GPU's own
closestToTriangle of the posed triangles -- posed on the host in the model's float32 order (mesh_query_model.posed) --,
clearanceToMesh is the reduction of those (world_mesh_dist_query_model.reduce: the smallest stored dist, then the lowest t),
withinOfMesh is tri >= 0 of that at the same r, and dist == 0 at a pose iff overlapsMesh flags it under the same skip. With skip
the reference world has the skipped instance's hierarchy replaced by one without leaves: the list without it, the indices kept."""
import ctypes
import os

import numpy as np
import pytest

import instance_query_model as NQ
import mesh_query_model as MQ
import tri_dist_query_model as TD
import world_box_query_model as WB
import world_mesh_dist_query_model as WM
import world_tri_dist_query_model as WD
from test_gpu_box_query import GRID_CAP, ROT_SCALE, SHEAR
from test_gpu_world_box import _World, _hier, _soup
from test_gpu_world_mesh import POINT, _leaves, general_poses, rotations
from test_gpu_world_tri_dist import COINCIDENT, EMPTY, _same, entries, meshes, torus
from test_world_box_cpu import _pose, cube

try:   # (imported before the library loads its HIP runtime, as tests/test_gpu_query.py)
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F = np.float32
I = np.int32


# ---- the populations case: shared with tests/test_world_mesh_dist_cpu.py, which shows every population by the flat model alone -----

POPULATIONS = ("misses by rmax", "poses at dist > 0", "poses at dist == 0", "ties broken by t", "ties broken by the instance",
               "winners beyond the first instance entered", "winners changed by skip")


def populations_case():
    """(meshes, entries, otris, poses, rmax): cubes on a lattice -- two of them coincident --, posed soups and a frame of two far
    triangles; a mesh with the same triangle loaded twice, a dropped one and a small soup; poses above a cube, through it, far
    off and at random"""
    rng = np.random.RandomState(131)
    frame = F([[[-9, -9, -9], [-9, -8.5, -9], [-8.5, -9, -9]], [[9, 9, 9], [9, 8.5, 9], [8.5, 9, 9]]])   # a box around everything, far triangles
    ms = [cube(), _soup(132, 40, 0.8, 0.3), frame]
    ent = [(0, NQ.IDENTITY), (0, _pose(np.eye(3), [5, 0, 0])), (0, NQ.IDENTITY.copy())]
    ent += [(1, NQ.random_pose(rng, reflect=bool(k & 1), shift=4.0)) for k in range(6)] + [(2, NQ.IDENTITY.copy())]
    near = F([[[0.25, 0.25, 1.5], [0.75, 0.25, 1.5], [0.25, 0.75, 1.75]]])                  # 0.5 above the cube's top face
    far = F([[[0.25, 0.25, 9], [0.75, 0.25, 9], [0.25, 0.75, 9]]])
    otris = np.concatenate([far, near, POINT, near, (_soup(133, 10, 0.3, 0.2) + F([0.5, 0.5, 3.0])).astype(F)])
    poses = [NQ.IDENTITY, _pose(np.eye(3), [0, 0, -0.75]), _pose(np.eye(3), [0, 0, 60]), _pose(np.eye(3), [5, 0, 0.25])]
    poses += general_poses(rng, 6, 0.0, 0.7)
    return ms, ent, otris, poses, 4.0


def populations(insts, otris, oleaves, poses, rmax):
    """how often each of POPULATIONS occurs in the flat answer of a case (and, for the first instance entered, in the walk (b))"""
    insts = [tuple(i[:3]) + (WB.plain_fit(i[0]),) for i in insts]
    hits, geom, rec, inst, within = WM.flat(insts, otris, oleaves, poses, rmax)
    free = WM.flat(insts, otris, oleaves, poses, np.inf)
    tri = hits.view(I)[:, :, 3]
    out = {"misses by rmax": int(((tri < 0) & (free[0].view(I)[:, :, 3] >= 0)).sum()),
           "poses at dist > 0": int((within & (rec[:, 2] > 0)).sum()), "poses at dist == 0": int((within & (rec[:, 2] == 0)).sum()),
           "ties broken by t": int(sum(((tri[q] >= 0) & (hits[q, :, 2] == rec[q, 2])).sum() > 1 for q in np.nonzero(within)[0]))}
    q = MQ.posed(otris, poses)
    by_inst, beyond = 0, 0
    world = WM.MeshDistWorld(insts)
    for m in np.nonzero(within)[0]:
        t = rec.view(I)[m, 6]
        lows = [WD.pair_records(i, q[m, t][None])[0] for i in insts]
        best = min(float(x.min()) for x in lows if x.size)
        by_inst += sum(1 for x in lows if x.size and float(x.min()) == best) > 1
        tab = world.prepare(q[m, t][None])
        _, g, entered = world.closest(tab, rmax, None)
        assert g[0] == inst[m]
        beyond += entered[0][0] != inst[m]
    out["ties broken by the instance"] = int(by_inst)
    out["winners beyond the first instance entered"] = int(beyond)
    changed = 0
    for s in sorted(set(int(x) for x in inst[inst >= 0])):
        other = WM.flat(insts, otris, oleaves, poses, rmax, s)[3]
        changed += int(((inst == s) & (other != s) & (other >= 0)).sum())
    out["winners changed by skip"] = changed
    return out


# ---- the check -----------------------------------------------------------------------------------------------------------------------

def reference(sc, other, otris, poses, rmax, skip):
    """closestToTriangle of the host-posed leaves of other on the same world (skip: that instance's hierarchy replaced by one
    without leaves), spread to [p, T]: (records [p, T, 8], instances [p, T])"""
    psm, w = sc.psm, sc.world
    q = MQ.posed(otris, poses)
    p, t = q.shape[:2]
    hits, geom = TD.miss_records(p * t).reshape(p, t, 8), np.full((p, t), -1, I)
    oleaves = _leaves(psm, other)
    if oleaves.size == 0 or len(w) == 0:
        return hits, geom
    packed = q[:, oleaves].reshape(-1, 3, 3)
    if skip is None:
        got = w.closestToTriangle(packed, rmax)
    else:
        empty = _hier(psm, sc.ctx, EMPTY)
        ref = psm.InstanceWorld(sc.ctx, [(empty if j == skip else th, m) for j, (th, m) in enumerate(zip(w.hierarchies, w.transforms()))])
        try:
            got = ref.closestToTriangle(packed, rmax)
        finally:
            ref.close()
            empty.close()
    hits[:, oleaves], geom[:, oleaves] = got.buffer.reshape(p, -1, 8), got.geom.reshape(p, -1)
    return hits, geom


def check(sc, other, otris, poses, rmax=np.inf, skip=None):
    """the three queries against the reference, against one another and against overlapsMesh; returns the reference's closest
    records and instances and its reduction"""
    w = sc.world
    otris = np.ascontiguousarray(otris, F).reshape(-1, 3, 3)
    p, t = MQ.poses12(poses).shape[0], otris.shape[0]
    hits, geom = reference(sc, other, otris, poses, rmax, skip)
    rec, inst = WM.reduce(hits, geom)
    got = w.closestToMesh(other, poses, rmax, skip=skip)
    assert got.buffer.shape == (p, t, 8) and got.buffer.dtype == F and got.geom.shape == (p, t) and got.geom.dtype == I
    _same(got.buffer, hits, "closestToMesh records")
    _same(got.geom, geom, "closestToMesh instances")
    one = w.clearanceToMesh(other, poses, rmax, skip=skip)
    assert one.buffer.shape == (p, 8) and one.geom.shape == (p,) and one.geom.dtype == I and one.other.dtype == I
    _same(one.buffer, rec, "clearanceToMesh records")
    _same(one.geom, inst, "clearanceToMesh instances")
    flag = w.withinOfMesh(other, poses, rmax, skip=skip)
    assert flag.shape == (p,) and flag.dtype == np.bool_
    _same(flag, one.tri >= 0, "withinOfMesh")
    with np.errstate(invalid="ignore"):
        counts = bool(F(rmax) >= 0)
    if counts:                                                                          # dist == 0 iff the pose cuts the world
        _same(one.dist == 0, w.overlapsMesh(other, poses, skip=skip), "dist == 0 against overlapsMesh")
    return hits, geom, rec, inst


# ---- 1: worlds of 1, 2 and 24 against other meshes of 0, 1, 63 and 65 leaves -----------------------------------------------------------

@pytest.mark.parametrize("leaves", [0, 1, 63, 65])
@pytest.mark.parametrize("n", [1, 2, 24])
def test_world_mesh_clearance_is_closest_to_triangle(psm, ctx, n, leaves):
    """the cube, the 256-triangle torus, a one-triangle mesh and an empty hierarchy, two instances coincident and one at an edge
    pose (n = 24); other with a dropped triangle first (L < T); p = 1 and 3"""
    rng = np.random.RandomState(1000 * n + leaves)
    otris = np.concatenate([POINT, _soup(2000 + leaves, leaves, 0.8, 0.3)]) if leaves else np.concatenate([POINT] * 3)
    with _World(psm, ctx, meshes(), entries(n)) as sc:
        other = _hier(psm, ctx, otris)
        try:
            assert other.info().leaf_count == leaves
            centre = sc.world.transforms()[:, :, 3]
            for p in (1, 3):
                poses = [_pose(r, centre[k % n] + t) for k, (r, t) in enumerate(zip(rotations(rng, p), rng.uniform(-0.6, 0.6, (p, 3))))]
                hits, geom, rec, inst = check(sc, other, otris, poses)
                assert (geom[:, 0] == -1).all() and ((inst >= 0).all() if leaves else (inst == -1).all())
                check(sc, other, otris, poses, 0.05)
                check(sc, other, otris, poses, np.inf, skip=int(inst[0]) if leaves else 0)
        finally:
            other.close()


# ---- 2: the populations ----------------------------------------------------------------------------------------------------------------

def test_populations_ties_and_skip(psm, ctx):
    """the case of populations_case(): the GPU against closestToTriangle and against the flat model; every population occurs;
    skip = none, the winner and a non-winner"""
    ms, ent, otris, poses, rmax = populations_case()
    with _World(psm, ctx, ms, ent) as sc:
        other = _hier(psm, ctx, otris)
        try:
            insts, oleaves = sc.insts(), _leaves(psm, other)
            assert list(oleaves) == [0, 1] + list(range(3, 14))
            hits, geom, rec, inst = check(sc, other, otris, poses, rmax)
            want = WM.flat(insts, otris, oleaves, poses, rmax)
            for got, model, what in zip((hits, geom, rec, inst), want, ("closest", "closest instances", "clearance", "clearance instances")):
                _same(got, model, "the flat model: " + what)
            counts = populations(insts, otris, oleaves, poses, rmax)
            for name in POPULATIONS:
                assert counts[name] > 0, (name, counts)
            # pose 0: 0.5 above cube 0 = cube 2, triangle 1 = triangle 3 of other; pose 3 the same above cube 1
            assert rec[0, 2] == 0.5 and rec.view(I)[0, 6] == 1 and inst[0] == 0 and rec[3, 2] == 0.75 and inst[3] == 1
            assert rec[1, 2] == 0 and inst[2] == -1
            _, _, r2, i2 = check(sc, other, otris, poses, rmax, skip=0)                # the winner skipped: its twin, the same record
            assert i2[0] == 2 and np.array_equal(r2[0].view(np.uint32), rec[0].view(np.uint32))
            _, _, r3, i3 = check(sc, other, otris, poses, rmax, skip=5)                # a non-winner of pose 0
            assert i3[0] == 0 and np.array_equal(r3[0].view(np.uint32), rec[0].view(np.uint32))
            for r in (0.0, -0.0, 1e-30, 0.5, np.nextafter(F(0.5), F(0)), np.nan, -1.0):
                _, _, rr, ii = check(sc, other, otris, poses, r)
                assert (ii[1] == inst[1]) == (not r < 0 and r == r) and (ii[0] == 0) == (r == 0.5)
        finally:
            other.close()


def test_identity_world_of_one_is_the_hierarchy_s_mesh_clearance(psm, ctx):
    rng = np.random.RandomState(134)
    otris = np.concatenate([_soup(135, 40, 1.0, 0.3), POINT, _soup(136, 30, 1.0, 0.3)])
    poses = general_poses(rng, 4, -2.0, 0.5)
    with _World(psm, ctx, [torus()], [(0, NQ.IDENTITY)]) as sc:
        other = _hier(psm, ctx, otris)
        try:
            th, w = sc.ths[0], sc.world
            for rmax in (np.inf, 0.3):
                a, b = w.closestToMesh(other, poses, rmax), th.meshClosest(other, poses, rmax)
                _same(a.buffer, b.buffer, "closest")
                assert np.array_equal(a.geom, np.where(b.tri >= 0, 0, -1))
                c, d = w.clearanceToMesh(other, poses, rmax), th.meshClearance(other, poses, rmax)
                _same(c.buffer, d.buffer, "clearance")
                assert np.array_equal(c.geom, np.where(d.tri >= 0, 0, -1))
                _same(w.withinOfMesh(other, poses, rmax), th.meshWithin(other, poses, rmax), "within")
            assert (d.tri >= 0).any() and (d.tri < 0).any()
            none = w.clearanceToMesh(other, poses, skip=0)                              # a world of one, skipped: enter() declines
            _same(none.buffer, WM.miss_clearance(4), "a world of one, skipped")
            assert (none.geom == -1).all() and not w.withinOfMesh(other, poses, np.inf, skip=0).any()
        finally:
            other.close()


def test_tiny_members_and_the_empty_world(psm, ctx):
    otris = np.concatenate([_soup(137, 20, 1.5, 0.5), POINT])
    rng = np.random.RandomState(138)
    poses = general_poses(rng, 3, -1.0, 0.3)
    with _World(psm, ctx, meshes(), [(3, NQ.IDENTITY), (2, NQ.IDENTITY), (3, NQ.IDENTITY)]) as sc:
        other = _hier(psm, ctx, otris)
        try:
            _, _, _, inst = check(sc, other, otris, poses)                              # a one-leaf member between empty ones
            assert (inst == 1).all()
            _, _, _, inst = check(sc, other, otris, poses, np.inf, skip=1)
            assert (inst == -1).all()
            sc.world.setInstances([(sc.ths[2], NQ.IDENTITY)])                           # a world of one leaf: the lone leaf in enter()
            sc.which = [2]
            check(sc, other, otris, poses)
            sc.world.setInstances([])                                                   # the empty world: the miss records, no walk
            sc.which = []
            got, one = sc.world.closestToMesh(other, poses), sc.world.clearanceToMesh(other, poses)
            _same(got.buffer, TD.miss_records(63).reshape(3, 21, 8), "empty world: closest")
            _same(one.buffer, WM.miss_clearance(3), "empty world: clearance")
            assert (got.geom == -1).all() and (one.geom == -1).all() and not sc.world.withinOfMesh(other, poses, np.inf).any()
        finally:
            other.close()


# ---- 3: the grid-stride loop and the study knobs ---------------------------------------------------------------------------------------

def test_grid_stride_second_trip_starts_clean(psm, ctx):
    """p x L just above PSM_QUERY_GRID_CAP x 64 + 65 with 65 leaves against two tiny members: the last queries take a second trip
    of the grid-stride loop, where the lane's best, its bound, the last key it saw and its retirement must start anew. The last
    pose stands apart from every other"""
    rng = np.random.RandomState(139)
    otris = np.concatenate([_soup(140, 30, 0.6, 0.5), POINT, _soup(141, 35, 0.6, 0.5)])
    leaves = 65
    p = -(-(GRID_CAP * 64 + 65) // leaves)
    assert GRID_CAP * 64 + 65 <= p * leaves < GRID_CAP * 64 + 65 + leaves
    poses = np.concatenate([rotations(rng, p), rng.uniform(-1.5, 1.5, (p, 3, 1))], axis=2)
    poses[-1, :, 3] = [7.0, -3.0, 2.0]
    ent = [(0, NQ.random_pose(rng, shift=0.5)), (1, NQ.random_pose(rng, reflect=True, shift=0.5))]
    with _World(psm, ctx, [_soup(142, 8, 0.5, 0.5), _soup(143, 7, 0.5, 0.5)], ent) as sc:
        other = _hier(psm, ctx, otris)
        try:
            assert other.info().leaf_count == leaves
            hits, geom, rec, inst = check(sc, other, otris, poses)
            assert (rec[:, 2] == 0).sum() > 100 and (rec[:, 2] > 0).sum() > 100 and (inst == 0).any() and (inst == 1).any()
            assert rec[-1, 2] > 4 and rec[-1, 2] > rec[:-1, 2].max() and (geom[:, 30] == -1).all()
            check(sc, other, otris, poses, 0.05, skip=1)                                # misses on both trips, one member left out
        finally:
            other.close()


def test_study_knobs_change_nothing(psm, ctx):
    rng = np.random.RandomState(144)
    otris = np.concatenate([_soup(145, 70, 1.0, 0.3), POINT])
    with _World(psm, ctx, meshes(), entries(24)) as sc:
        other = _hier(psm, ctx, otris)
        try:
            centre = sc.world.transforms()[:, :, 3]
            poses = [_pose(r, centre[k % 24] + t) for k, (r, t) in enumerate(zip(rotations(rng, 40), rng.uniform(-1, 1, (40, 3))))]
            w = sc.world
            want = w.clearanceToMesh(other, poses, skip=3)
            flag = w.withinOfMesh(other, poses, 0.1, skip=3)
            assert (want.dist == 0).any() and (want.dist > 0).any() and flag.any() and not flag.all()
            for knob in ("1", "1", "0", "2", "3"):
                os.environ["PSM_MESH_BOUND"] = knob
                try:
                    got = w.clearanceToMesh(other, poses, skip=3)
                finally:
                    del os.environ["PSM_MESH_BOUND"]
                _same(got.buffer, want.buffer, "PSM_MESH_BOUND=" + knob)
                _same(got.geom, want.geom, "PSM_MESH_BOUND=%s instances" % knob)
            for knob in ("1", "1", "0"):
                os.environ["PSM_MESH_SKIP"] = knob
                try:
                    _same(w.withinOfMesh(other, poses, 0.1, skip=3), flag, "PSM_MESH_SKIP=" + knob)
                finally:
                    del os.environ["PSM_MESH_SKIP"]
        finally:
            other.close()


# ---- 4: other trees, refits, stale worlds ---------------------------------------------------------------------------------------------

def test_answers_do_not_depend_on_the_trees_and_follow_a_refit(psm, ctx):
    rng = np.random.RandomState(146)
    a, b = _soup(147, 150, 1.0, 0.2), _soup(148, 100, 1.0, 0.2)
    ent = [(k % 2, NQ.random_pose(rng, reflect=bool(k & 1), shift=1.5)) for k in range(6)]
    otris = _soup(149, 80, 1.2, 0.4)
    poses = general_poses(rng, 3, -2.0, 0.3)
    with _World(psm, ctx, [a, b], ent) as plain:
        other = _hier(psm, ctx, otris)
        try:
            hits, geom, rec, inst = check(plain, other, otris, poses)
            skipped = plain.world.clearanceToMesh(other, poses, skip=1)
            for opt in (ROT_SCALE, SHEAR):
                with _World(psm, ctx, [a, b], ent, [opt, opt]) as sc:
                    other2 = _hier(psm, ctx, otris, opt)
                    try:
                        for o in (other, other2):
                            got, one = sc.world.closestToMesh(o, poses), sc.world.clearanceToMesh(o, poses)
                            _same(got.buffer, hits, "closest under a build matrix")
                            _same(got.geom, geom, "closest instances under a build matrix")
                            _same(one.buffer, rec, "clearance under a build matrix")
                            _same(one.geom, inst, "clearance instances under a build matrix")
                        _same(sc.world.clearanceToMesh(other2, poses, skip=1).buffer, skipped.buffer, "skip under a build matrix")
                    finally:
                        other2.close()
            # a refit of a member (then refresh()) and of other: the records follow the triangles as they now are
            h = plain.ths[1]
            small = (b * F(0.5)).astype(F)
            h.clearTribuffer()
            h.loadTriangles(small.reshape(-1, 9))
            h.refit()
            plain.world.refresh()
            plain.meshes[1] = small
            hits2, _, _, _ = check(plain, other, otris, poses)
            assert (geom == 1).any() and (hits2.view(np.uint32) != hits.view(np.uint32)).any()
            shrunk = (otris * F(0.75)).astype(F)
            other.clearTribuffer()
            other.loadTriangles(shrunk.reshape(-1, 9))
            other.refit()
            check(plain, other, shrunk, poses, np.inf, skip=2)
        finally:
            other.close()


def test_stale_world_set_transform_and_refresh(psm, ctx):
    rng = np.random.RandomState(150)
    otris = _soup(151, 30, 1.0, 0.3)
    poses = general_poses(rng, 3, -1.0, 0.3)
    with _World(psm, ctx, meshes(), entries(2)) as sc:
        other = _hier(psm, ctx, otris)
        try:
            _, _, before, _ = check(sc, other, otris, poses)
            sc.world.setTransform(1, NQ.random_pose(rng, shift=2.0))
            _, _, after, _ = check(sc, other, otris, poses)
            assert (before.view(np.uint32) != after.view(np.uint32)).any()
            h = sc.ths[1]
            h.markDirty()
            h.build()
            for call, name in ((lambda: sc.world.closestToMesh(other, poses), "closest"), (lambda: sc.world.withinOfMesh(other, poses, 1.0), "within"),
                               (lambda: sc.world.clearanceToMesh(other, poses), "clearance")):
                with pytest.raises(psm.PsmError, match="psm_world_mesh_%s_dev: instance 1's hierarchy was rebuilt" % name):
                    call()
            sc.world.setInstances([(sc.ths[k], m) for k, m in zip(sc.which, sc.world.transforms())])
            _, _, again, _ = check(sc, other, otris, poses)
            _same(again, after, "after the instances were set again")
            sc.world.refresh()
            _same(sc.world.clearanceToMesh(other, poses).buffer, after, "after refresh()")
        finally:
            other.close()


# ---- 5: torch ------------------------------------------------------------------------------------------------------------------------------

def test_world_mesh_clearance_torch_tensors_on_a_side_stream(psm, ctx):
    if torch is None:
        pytest.skip("torch is not installed")
    rng = np.random.RandomState(152)
    otris = _soup(153, 150, 1.5, 0.4)
    poses = general_poses(rng, 8, -2.0, 1.0)
    with _World(psm, ctx, meshes(), entries(24)) as sc:
        other = _hier(psm, ctx, otris)
        try:
            w = sc.world
            hits, one, flag = w.closestToMesh(other, poses, 2.0, skip=4), w.clearanceToMesh(other, poses, 2.0, skip=4), w.withinOfMesh(other, poses, 0.5, skip=4)
            dev = torch.device("cuda", 0)
            side = torch.cuda.Stream(dev)
            with torch.cuda.stream(side):      # neither the context's stream nor torch's default one
                gh = w.closestToMesh(other, poses, 2.0, skip=4, as_torch=True)
                go = w.clearanceToMesh(other, poses, 2.0, skip=4, as_torch=True)
                gf = w.withinOfMesh(other, poses, 0.5, skip=4, as_torch=True)
                bufs = [x.cpu() for x in (gh.buffer, gh.geom, go.buffer, go.geom, gf, go.other)]   # (on the side stream: in order)
            assert gh.buffer.device == dev and gh.buffer.shape == (8, 150, 8) and gh.geom.dtype == torch.int32 and gh.geom.shape == (8, 150)
            assert go.buffer.shape == (8, 8) and go.geom.shape == (8,) and gf.dtype == torch.bool and gf.shape == (8,)
            _same(bufs[0].numpy(), hits.buffer, "torch closestToMesh records")
            _same(bufs[1].numpy(), hits.geom, "torch closestToMesh instances")
            _same(bufs[2].numpy(), one.buffer, "torch clearanceToMesh records")
            _same(bufs[3].numpy(), one.geom, "torch clearanceToMesh instances")
            _same(bufs[4].numpy(), flag, "torch withinOfMesh")
            _same(bufs[5].numpy(), one.other, "torch other view")
        finally:
            other.close()


# ---- 6: refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(psm, ctx):
    """NULL other, poses and outputs, misaligned outputs, other not built, other of another context, a stale world, a bad pose
    named by its index, skip out of range and p x T = 2^32 are refused on the host in world_mesh_query()'s order and with its
    texts: the outputs keep what they held; then the same buffers succeed"""
    lib = psm.lib()
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    through = F([[[0, 0, -2], [2, 0, 2], [2, 1, 2]], [[0, 0.25, -2], [2, 0.25, 2], [2, 1.25, 2]]])
    p, t = 3, 2
    ctx2 = psm.Context(0)
    foreign = big = unbuilt = None
    with _World(psm, ctx, [tri, tri + F([0.125, 0, 0])], [(0, NQ.IDENTITY), (1, NQ.IDENTITY)]) as sc:
        other = _hier(psm, ctx, through)
        hout, hinst, hbig = ctx.buf_alloc(32 * p * t + 32), ctx.buf_alloc(4 * p * t + 16), ctx.buf_alloc(65536 + 16)
        try:
            w = sc.world._w
            ctx.buf_upload(hout, np.full(8 * p * t + 8, 7, np.int32))
            ctx.buf_upload(hinst, np.full(p * t + 4, 9, np.int32))
            ctx.buf_upload(hbig, np.full(65536 + 16, 5, np.uint8))
            pout, pinst, pbig = (ctypes.c_void_p(ctx.buf_ptr(h)[0]) for h in (hout, hinst, hbig))
            good = np.ascontiguousarray(np.tile(np.eye(3, 4, dtype=F).reshape(1, 12), (p, 1)))
            size, none = ctypes.c_size_t(p), ctypes.c_int32(-1)
            err = lambda: lib.psm_last_error(ctx._h)

            def ptr(a):
                return a.ctypes.data_as(ctypes.c_void_p)

            def rec_call(fn, o=other, m=good, skip=none, r=1.0, p_out=pout, p_inst=pinst, count=size, world=w):
                return fn(world, None if o is None else o._h, None if m is None else ptr(m), count, skip, ctypes.c_float(r), p_out, p_inst)

            def flag_call(o=other, m=good, skip=none, r=1.0, p_out=pbig, count=size, world=w):
                return lib.psm_world_mesh_within_dev(world, None if o is None else o._h, None if m is None else ptr(m), count, skip, ctypes.c_float(r), p_out)
            recs = ((lib.psm_world_mesh_closest_dev, b"psm_world_mesh_closest_dev"), (lib.psm_world_mesh_clearance_dev, b"psm_world_mesh_clearance_dev"))
            no_world = lib.psm_world_tri_count_dev(None, pinst, size, pinst)
            for fn, name in recs:
                assert rec_call(fn, world=None) == no_world != 0
                assert rec_call(fn, count=ctypes.c_size_t(0), o=None, m=None) == 0       # p = 0 is answered first
                assert rec_call(fn, o=None) == -1 and rec_call(fn, m=None) == -1 and rec_call(fn, p_out=None) == -1
                assert rec_call(fn, p_inst=None) == -1 and name + b": NULL pointer" in err()
                assert rec_call(fn, p_out=ctypes.c_void_p(pout.value + 8)) == -1 and name + b": hits not 16-byte aligned" in err()
                assert rec_call(fn, p_inst=ctypes.c_void_p(pinst.value + 2)) == -1 and name + b": inst not 4-byte aligned" in err()
            assert flag_call(world=None) == no_world and flag_call(count=ctypes.c_size_t(0)) == 0
            assert flag_call(o=None) == -1 and flag_call(m=None) == -1 and flag_call(p_out=None) == -1 and b"psm_world_mesh_within_dev: NULL pointer" in err()
            unbuilt = psm.TriangleHierarchy(ctx)                                      # other not built: PSM_ERR_STATE
            unbuilt.allocate(4)
            unbuilt.loadTriangles(through.reshape(2, 9))
            foreign = _hier(psm, ctx2, through)                                       # a built hierarchy of another context
            ctx2.sync()
            scaled, nan = good.copy(), good.copy()
            scaled[1, [0, 5, 10]] = 1.01                                              # pose 1 scaled by 1.01
            nan[2, 7] = np.nan
            big = psm.TriangleHierarchy(ctx)
            big.allocate(65536)
            big.loadTriangles(np.tile(through.reshape(2, 9), (32768, 1)))
            big.build()
            many = np.ascontiguousarray(np.tile(np.eye(3, 4, dtype=F).reshape(1, 12), (65536, 1)))
            calls = [lambda fn=fn, **kw: rec_call(fn, **kw) for fn, _ in recs] + [flag_call]
            for call in calls:
                assert call(o=unbuilt) == -5 and b"mesh query before build" in err()
                assert call(o=foreign) == -1 and b"the world and the other hierarchy are of different contexts" in err()
                assert call(m=scaled) == -1 and b"pose 1 has a transform that is not rigid" in err()
                assert call(m=nan) == -1 and b"pose 2 has a non-finite transform" in err()
                for s in (2, 3, -2, 1 << 30):
                    assert call(skip=ctypes.c_int32(s)) == -1 and b"skip %d of a world of 2" % s in err()
                assert call(m=scaled, skip=ctypes.c_int32(5)) == -1 and b"pose 1" in err()     # the pose before skip
            # p x T = 2^32: PSM_ERR_CAPACITY (-4), before any upload, through the flag entry alone (a byte per pose)
            assert flag_call(o=big, m=many, count=ctypes.c_size_t(65536)) == -4 and b"psm_world_mesh_within_dev: 65536 poses of 65536 triangles are more than 2^32 answers" in err()
            sc.ths[1].markDirty()
            sc.ths[1].build()                                                         # stale: PSM_ERR_STATE, every world query's message
            for call in calls:
                assert call() == -5 and b"instance 1's hierarchy was rebuilt, or reloaded and not refitted, after psm_world_set_instances" in err()
                assert call(m=nan) == -5 and b"hierarchy was rebuilt" in err()        # the stale world before the poses
            ctx.sync()
            assert (ctx.buf_download(hout, np.int32, 8 * p * t + 8) == 7).all() and (ctx.buf_download(hinst, np.int32, p * t + 4) == 9).all()
            assert (ctx.buf_download(hbig, np.uint8, 65536 + 16) == 5).all()
            sc.world.setInstances([(sc.ths[0], NQ.IDENTITY), (sc.ths[1], NQ.IDENTITY)])
            w = sc.world._w
            assert rec_call(lib.psm_world_mesh_closest_dev, world=w) == 0             # and the same buffers are fine
            ctx.sync()
            rows, geom = ctx.buf_download(hout, np.int32, 8 * p * t + 8), ctx.buf_download(hinst, np.int32, p * t + 4)
            assert (rows[8 * p * t:] == 7).all() and (geom[p * t:] == 9).all() and (geom[:p * t] == 0).all()
            assert (rows[:8 * p * t].reshape(p * t, 8)[:, 3] == 0).all() and (rows[:8 * p * t].reshape(p * t, 8).view(F)[:, 2] == 0).all()
            assert rec_call(lib.psm_world_mesh_clearance_dev, world=w, skip=ctypes.c_int32(0)) == 0
            assert flag_call(world=w, skip=ctypes.c_int32(0)) == 0
            ctx.sync()
            rows, geom = ctx.buf_download(hout, np.int32, 8 * p), ctx.buf_download(hinst, np.int32, p * t + 4)
            assert (geom[:p] == 1).all() and (geom[p:p * t] == 0).all() and (rows.reshape(p, 8)[:, 6] == 0).all()
            assert list(ctx.buf_download(hbig, np.uint8, p + 4)) == [1] * p + [5] * 4
            with pytest.raises(psm.PsmError, match="skip must be None"):
                sc.world.clearanceToMesh(other, good.reshape(p, 3, 4), skip=2)
            with pytest.raises(psm.PsmError, match="different contexts"):
                sc.world.withinOfMesh(foreign, good.reshape(p, 3, 4), 1.0)
        finally:
            for h in (hout, hinst, hbig):
                ctx.buf_free(h)
            for th in (other, foreign, big, unbuilt):
                if th is not None:
                    th.close()
            ctx2.close()
