"""CPU tests (no GPU) of the instance worlds at edge-of-rigid, far and mixed-scale poses (tests/world_pose_cases.py; DESIGN.md
4.11, 4.14, 4.16, 4.18, 4.20, 4.25, 4.26): what the generators promise; that the case queries are within the project's own
well-posedness rule; that every family's walk model -- boxes, padding, tree, prune -- answers bit for bit what the flat list
answers, on every case and on both passes, and still culls; and the 4.11 bound observed on the forward image, with the move's
rounding and R against R^-T both in the figure. tests/test_gpu_world_pose_edges.py holds the kernels to the same flat answers."""
import functools

import numpy as np
import pytest

import inside_query_model as IQ
import mesh_query_model as MQ
import ray_prune_model as RP
import world_box_query_model as WB
import world_kbest_query_model as WK
import world_mesh_dist_query_model as WMD
import world_pose_cases as PC
import world_query_model as WQ
import world_sweep_query_model as WS
import world_tri_dist_query_model as WD
import world_tri_query_model as WT
from test_world_query_cpu import _same, check_world_model

F = np.float32
D = np.float64
N = 96                 # queries per family and pass: the walk models take a python step per query and node
LEFT_OUT_CAP = 0.01    # matrix_world_queries' cap (tests/test_gpu_world_query.py): a condition, not a measurement


# ---- the generators ---------------------------------------------------------------------------------------------------------------

def test_edge_pose_stays_in_its_window_and_draws_both_kinds():
    """the window is tests/test_world_box_cpu.py's _edge_pose's; half the draws stretch, half shear; reflections are reflections"""
    rng = np.random.RandomState(1)
    kinds = []
    for k in range(400):
        p = PC.edge_pose(rng, bool(k & 1), rng.uniform(-5, 5, 3))
        assert PC.E_WINDOW[0] < PC.pose_error(p) <= PC.E_WINDOW[1] and PC.pose_accepted(p)
        assert (np.linalg.det(p[:, :3].astype(D)) < 0) == bool(k & 1)
        kinds.append(PC.edge_kind(p))
    assert 120 < kinds.count("stretch") < 280 and kinds.count("stretch") + kinds.count("shear") == 400
    p = PC.edge_pose(rng, False, np.zeros(3), PC.signed_permutation(rng))
    assert np.sort(np.abs(p[:, :3]).round().sum(axis=0)).tolist() == [1, 1, 1] and PC.E_WINDOW[0] < PC.pose_error(p)


def test_drifted_pose_is_accepted_and_has_drifted():
    rng = np.random.RandomState(2)
    for _ in range(4):
        p = PC.drifted_pose(rng)
        assert PC.pose_accepted(p) and PC.pose_error(p) > 1e-6


def test_pose_accepted_is_the_pose_check():
    bad = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(F)
    assert PC.pose_accepted(bad)
    for at, v in (((0, 0), 1.0 + 6e-6), ((0, 1), 1.1e-5), ((2, 3), np.nan)):
        m = bad.copy()
        m[at] = v
        assert not PC.pose_accepted(m), at
    m = bad.copy()
    m[0, 0] = 1.0 + 4e-6                      # E = 8e-6: admitted
    assert PC.pose_accepted(m)


@pytest.mark.parametrize("name", PC.CASES)
def test_case_worlds_are_what_their_docstrings_say(name):
    c = PC.case(name)
    poses = np.array([m for _, m in c.entries])
    T = np.abs(poses[:, :, 3]).max(axis=1)
    E = np.array([PC.pose_error(m) for m in poses])
    obj = np.array([np.abs(c.meshes[k]).max() for k, _ in c.entries])
    assert len(c.entries) == PC.INSTANCES and len(c.meshes) <= 4 and all(PC.pose_accepted(m) for m in poses)
    assert sorted(t.shape[0] for t in c.meshes[:2]) == [20, 64] or name in ("object_far", "mixed")
    for k in range(4, PC.INSTANCES, 5):       # every fifth exactly at its predecessor's pose, of the same mesh
        assert c.entries[k][0] == c.entries[k - 1][0] and np.array_equal(poses[k], poses[k - 1])
    mid = np.abs(c.middle).max(axis=1)
    if name in ("far", "edge_far"):
        assert [(np.abs(mid - x) < 0.02 * x + 8).sum() for x in (0.0, 1e2, 1e4)] == [16, 16, 16]
    if name in ("far", "mixed", "object_far"):
        assert E.max() < 2e-7
    if name in ("edge", "edge_far"):
        assert PC.E_WINDOW[0] < E.min() and E.max() <= PC.E_WINDOW[1]
        assert {PC.edge_kind(m) for m in poses} == {"stretch", "shear"}
    if name == "edge":
        assert T.max() < 8 and obj.max() < 1
    if name == "object_far":                  # stored ~300 away, posed back to within a few units of the origin
        far = obj > 100
        assert far.sum() >= 30 and mid.max() < 6 and (T[far] > 150).all() and (obj[far] / T[far]).max() > 1.2
    if name == "edge_far":
        far = obj > 100
        assert far.sum() >= 10 and (far & (mid < 8)).sum() >= 3        # some of them near the origin: S is all the padding has
    if name == "mixed":
        assert sorted(set(np.round(np.log10(c.radius / 0.6)).astype(int))) == [-3, 0, 2]
        big = np.nonzero(c.radius > 10)[0]
        small = np.nonzero(c.radius < 0.01)[0]
        gap = np.linalg.norm(c.middle[small][:, None] - c.middle[big][None], axis=2).min(axis=1)
        assert (gap < 62).sum() > 5 and big.size == 4 and small.size >= 24


# ---- the case queries, their flat answers and the rule ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _rays_and_points(name):
    """the local rays and points of a case cut down to the well-posed ones, and the share left out"""
    c = PC.case(name)
    rays, points, _ = PC.local_queries(c, 100 + PC.CASES.index(name), N)
    keep = RP.fully_well_posed(c.members(), rays[0], rays[1])
    sure = RP.vote_rays_well_posed(c.members(), points[0], IQ.INSIDE_DIRECTIONS)
    out = (~keep).mean(), (~sure).mean()
    return tuple(x[keep] for x in rays), tuple(x[sure] for x in points), out


@pytest.mark.parametrize("name", PC.CASES)
def test_the_case_queries_are_well_posed_by_the_project_s_rule(name):
    """ray_prune_model's rule with each member's plain fit: at most 1 % of the rays and of the points may be left out"""
    _, _, (rays_out, points_out) = _rays_and_points(name)
    print("%s: left out %.3g of the rays, %.3g of the points" % (name, rays_out, points_out))
    assert rays_out <= LEFT_OUT_CAP and points_out <= LEFT_OUT_CAP


# ---- every family's walk model against the flat answer ---------------------------------------------------------------------------------

def _culls(name, entered, what):
    avg = WQ.average_entered(entered)
    print("%s: %s enters %.2f of %d instances per query" % (name, what, avg, PC.INSTANCES))
    if name in ("far", "edge", "edge_far"):
        assert avg < 0.5 * PC.INSTANCES, (name, what, avg)


@pytest.mark.parametrize("name", PC.CASES)
def test_basic_kinds_and_kbest_walk_equals_flat(name):
    c = PC.case(name)
    insts = c.insts()
    rays, points, _ = _rays_and_points(name)
    ent = check_world_model(insts, rays, points)
    for kind, e in ent.items():
        _culls(name, e, kind)
    o, d, tmin, tmax = rays
    eh, ei, _, ec = WQ.flat_rays(WQ.per_instance_rays(insts, o, d, tmin, tmax))
    ph, pi, _ = WQ.flat_points(WQ.per_instance_points(insts, *points))
    assert (ei >= 0).sum() > 50 and (pi >= 0).sum() > 50 and len(set(ei[ei >= 0])) > 10
    for k in (1, 4, 16):                      # the k-best merge: slot 0 is the closest record, the count the hit count cut at k
        rows, rinst, count = WK.first_hits(insts, o, d, k, tmin, tmax)
        _same(rows[:, 0], eh, "firstHits slot 0, k = %d" % k)
        _same(rinst[:, 0], ei, "firstHits inst 0, k = %d" % k)
        _same(count, np.minimum(ec, k).astype(np.uint32), "firstHits count, k = %d" % k)
        rows, rinst, count = WK.nearest(insts, points[0], k, points[1])
        _same(rows[:, 0], ph, "nearest slot 0, k = %d" % k)
        _same(rinst[:, 0], pi, "nearest inst 0, k = %d" % k)
    # the decisive pass: tmax at the closest t and one float below it, rmax at the closest distance
    r2, p2 = PC.decisive_rays(insts, rays), PC.decisive_points(insts, points)
    check_world_model(insts, r2, p2)
    n = o.shape[0]
    h2 = WQ.flat_rays(WQ.per_instance_rays(insts, *r2))[0]
    hit = np.isfinite(eh[:, 2])
    _same(h2[:n][hit], eh[hit], "tmax = t keeps the record")
    assert np.isinf(h2[n:][hit, 2]).all()                          # one float below: nothing is left in the window
    assert (WQ.flat_points(WQ.per_instance_points(insts, *p2))[1] >= 0).all()


@pytest.mark.parametrize("name", PC.CASES)
def test_box_and_triangle_walks_equal_flat(name):
    c = PC.case(name)
    insts = c.box_insts()
    seed = 200 + PC.CASES.index(name)
    for what, (lo, hi) in (("boxes", PC.local_boxes(c, seed, N)), ("touching boxes", PC.decisive_boxes(c, seed + 10, 2))):
        want = WB.flat(insts, lo, hi, 16)
        got, ent = WB.BoxWorld(insts).boxes(lo, hi, 16)
        for g, w, part in zip(got, want, ("overlaps", "count", "tri", "inst", "rows' count")):
            _same(g, w, "%s: %s" % (what, part))
        assert (want[1] > 0).sum() > 20 and (what != "boxes" or (want[1] == 0).sum() > 10), (what, (want[1] > 0).sum())
        _culls(name, ent[0], what)
    q, _ = PC.local_triangles(c, seed + 20, N)
    for what, tris in (("triangles", q), ("touching triangles", PC.decisive_triangles(c, seed + 30, q))):
        want = WT.flat(insts, tris, 16)
        got, ent = WT.TriWorld(insts).tris(tris, 16)
        for g, w, part in zip(got, want, ("overlaps", "count", "tri", "inst", "rows' count")):
            _same(g, w, "%s: %s" % (what, part))
        assert (want[1] > 0).sum() > 10 and (want[1] == 0).sum() > 10, (what, (want[1] > 0).sum())
        _culls(name, ent[0], what)
    assert (WT.flat(insts, PC.decisive_triangles(c, seed + 30, q), 16)[1][::2] > 0).all()   # a shared vertex always counts


@pytest.mark.parametrize("name", PC.CASES)
def test_sweep_walk_equals_flat(name):
    c = PC.case(name)
    insts = c.box_insts()
    first = PC.local_sweeps(c, 300 + PC.CASES.index(name), N)
    for what, (o, d, r, tm) in (("sweeps", first), ("sweeps to their contact", PC.decisive_sweeps(c.insts(), first))):
        hits, inst, occ = WS.flat(c.insts(), o, d, r, tm)
        (gh, gi), go, ent = WS.SweepWorld(insts).sweeps(o, d, r, tm)
        _same(gh, hits, what)
        _same(gi, inst, what + ": inst")
        _same(go, occ, what + ": occluded")
        assert (inst >= 0).sum() > 50, (what, (inst >= 0).sum())
        _culls(name, ent[0], what)
    _same(WS.flat(c.insts(), *PC.decisive_sweeps(c.insts(), first))[0], WS.flat(c.insts(), *first)[0], "tmax = t keeps the contact")


@pytest.mark.parametrize("name", PC.CASES)
def test_clearance_walks_equal_flat(name):
    c = PC.case(name)
    insts = c.box_insts()
    seed = 400 + PC.CASES.index(name)
    q, rm = PC.local_triangles(c, seed, N)
    world = WD.TriDistWorld(insts)
    for what, rmax in (("clearance", rm), ("clearance at the flat dist", PC.decisive_clearance(insts, q))):
        pairs = [WD.pair_records(i, q) for i in insts]
        hits, inst, within = WD.flat(insts, q, rmax, pairs)
        (gh, gi), entered, _ = world.closest(q, rmax, pairs=pairs)
        _same(gh, hits, what)
        _same(gi, inst, what + ": inst")
        flags, _, _ = world.closest(q, rmax, within=True, pairs=pairs)
        _same(flags, within, what + ": within")
        assert within.sum() > 50 and (hits[within, 2] > 0).sum() > 20, (what, within.sum())
        _culls(name, entered, what)
    assert WD.flat(insts, q, PC.decisive_clearance(insts, q))[2].all()
    # mesh clearance: the torus at poses from edge_pose, the far shifts among them; with and without a skip
    tor = PC.base_meshes()[1]
    leaves = np.arange(tor.shape[0])
    poses = PC.other_poses(c, seed + 10, 2)
    mesh_world = WMD.MeshDistWorld(insts)
    posed = MQ.posed(tor, poses)
    for skip in (None, int(WMD.flat(insts, tor, leaves, poses)[3][0])):
        hits, geom, rec, rinst, _ = WMD.flat(insts, tor, leaves, poses, np.inf, skip)
        for m in range(len(poses)):
            tab = mesh_world.prepare(posed[m])
            gh, gg, _ = mesh_world.closest(tab, np.inf, skip)
            _same(gh, hits[m], "closestToMesh, pose %d, skip %s" % (m, skip))
            _same(gg, geom[m], "closestToMesh inst, pose %d, skip %s" % (m, skip))
            _, grec, ginst = mesh_world.clearance(tab, leaves, np.inf, skip, WMD.VARIANTS[-1])
            _same(grec[None], rec[m][None], "clearanceToMesh, pose %d, skip %s" % (m, skip))
            assert ginst == rinst[m] and (skip is None or ginst != skip)


# ---- the 4.11 bound, observed on the forward image ----------------------------------------------------------------------------------

def test_padding_bound_observed_on_the_forward_image():
    """DESIGN.md 4.11's chain on 10 000 poses at the edge of the pose check (edge_pose) and drifted in float32 (drifted_pose), over
    six decades of object size and of |T| / size: the distance between the forward image of an object point -- what the world box
    bounds -- and the world point whose float32 move is that object point (world_query_model.forward_discrepancy: the move's
    rounding and R against R^-T are both in it) stays under the derived bound, and the bound under a quarter of what the padding
    and the query slack grant (the factor 4 of test_padding_bound_has_four_times_headroom and of the box / triangle margin tests).
    Measured: the largest observed / bound 0.45, the largest bound / granted 0.090."""
    rng = np.random.RandomState(12)
    drifted = [r for r in PC.drifted_rotations(rng, PC.DRIFT_STEPS, 2400)
               if 1e-6 < PC.pose_error(np.concatenate([r, np.zeros((3, 1), F)], axis=1)) <= PC.E_LIMIT][:2000]
    assert len(drifted) == 2000
    worst_ob, worst_bg, worst_e = 0.0, 0.0, 0.0
    for k in range(10000):
        size = 10.0 ** rng.uniform(-3, 3)
        t = rng.normal(size=3)
        t = t / np.linalg.norm(t) * size * 10.0 ** rng.uniform(-3, 3)
        if k % 5 == 4:
            pose = np.concatenate([drifted[k // 5], t.reshape(3, 1).astype(F)], axis=1).astype(F)
        else:
            pose = PC.edge_pose(rng, bool(k & 1), t)
        assert PC.pose_accepted(pose)
        worst_e = max(worst_e, PC.pose_error(pose))
        seen, objmag, x = WQ.forward_discrepancy(pose, rng.uniform(-1, 1, 3) * size)
        bound = WQ.move_bound(pose, x, objmag)
        granted = float(WQ.WORLD_PAD) * max(objmag, float(np.abs(pose[:, 3]).max())) + float(WQ.WORLD_QSLACK) * float(np.abs(x).max())
        assert seen <= bound, (k, seen, bound)
        assert bound <= granted / 4, (k, bound, granted)
        worst_ob, worst_bg = max(worst_ob, seen / bound), max(worst_bg, bound / granted)
    print("forward image: the largest observed / bound %.3g, the largest bound / granted %.3g (E up to %.3g)" % (worst_ob, worst_bg, worst_e))
    assert worst_ob > 0.3 and worst_e > 0.9e-5           # the draws do reach the term that non-rigidity is charged for
