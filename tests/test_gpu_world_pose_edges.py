"""Every query of an instance world on the GPU at edge-of-rigid, far and mixed-scale poses (tests/world_pose_cases.py; DESIGN.md
4.11 and the sections of the families). The padding and the slacks of the two-level prune are derived from the move's rounding,
the non-rigidity the pose check admits and S; here the kernels run where those terms are large, and every exported world query
is held bit for bit against its FLAT model -- the brute force over the ordered list, which knows no box, no tree and no S -- on
a first pass of local queries and on a decisive second one (tmax at the closest t and one float below, rmax at the closest
distance, boxes that touch posed triangles to an ulp, tmax at a sweep's contact, rmax at a triangle's clearance). A dropped
instance is then another record, not a silent one. Rays and points are the ones tests/ray_prune_model.py's rule keeps (at most
1 % may be left out). The seven kinds are also held against InstancedScene, which shares no numpy model with the rest."""
import functools

import numpy as np
import pytest

import inside_query_model as IQ
import instance_query_model as NQ
import ray_prune_model as RP
import world_mesh_dist_query_model as WMD
import world_pose_cases as PC
from test_gpu_world_box import _hier, check_boxes
from test_gpu_world_grid import check_grid
from test_gpu_world_kbest_query import check_points, check_rays
from test_gpu_world_mesh import _leaves as sorted_leaves
from test_gpu_world_mesh import check_mesh
from test_gpu_world_mesh_dist import check as check_mesh_clearance
from test_gpu_world_query import _World, _check
from test_gpu_world_sweep import check_closed, check_sweeps
from test_gpu_world_tri import check_tris
from test_gpu_world_tri_dist import check as check_clearance
from test_gpu_world_tri_dist import _same as same_bits
from test_world_query_cpu import _same

pytestmark = pytest.mark.gpu

F = np.float32
N = 256                # queries per family and pass (the decisive ray pass holds every ray twice: 512)
KS = (1, 4, 16)
LEFT_OUT_CAP = 0.01    # matrix_world_queries' cap (tests/test_gpu_world_query.py): a condition, not a measurement


def _world(psm, ctx, c, entries=None):
    sc = _World(psm, ctx, c.meshes, c.entries if entries is None else entries)
    for th, t in zip(sc.ths, sc.meshes):
        assert th.info().leaf_count == t.shape[0]          # every triangle is a leaf: the case's own instance list is the world's
    return sc


@functools.lru_cache(maxsize=None)
def _local(name):
    c = PC.case(name)
    return PC.local_queries(c, 500 + PC.CASES.index(name), N)


def _well_posed(sc, name):
    """the case's local rays and points cut down by ray_prune_model's rule with the hierarchies' own transforms"""
    rays, points, _ = _local(name)
    members = sc.members()
    keep = RP.fully_well_posed(members, rays[0], rays[1])
    sure = RP.vote_rays_well_posed(members, points[0], IQ.INSIDE_DIRECTIONS)
    assert (~keep).mean() <= LEFT_OUT_CAP and (~sure).mean() <= LEFT_OUT_CAP, (int((~keep).sum()), int((~sure).sum()))
    return tuple(x[keep] for x in rays), tuple(x[sure] for x in points)


@pytest.mark.parametrize("name", PC.CASES)
def test_basic_kinds_and_kbest_against_the_flat_list(psm, ctx, name):
    c = PC.case(name)
    with _world(psm, ctx, c) as sc:
        insts = sc.insts()
        rays, points = _well_posed(sc, name)
        got, gp = _check(sc, rays, points, samples=(1, 3, 5), insts=insts)
        assert (got.geom >= 0).sum() > 50 and (gp.geom >= 0).sum() > 50 and len(np.unique(got.geom)) > 15
        check_rays(sc, rays[0], rays[1], KS, rays[2], rays[3], insts)
        check_points(sc, points[0], KS, points[1], insts)
        r2, p2 = PC.decisive_rays(insts, rays), PC.decisive_points(insts, points)
        got2, gp2 = _check(sc, r2, p2, samples=(3,), insts=insts)
        n = rays[0].shape[0]
        hit = got.geom >= 0
        _same(got2.buffer[:n][hit], got.buffer[hit], "tmax = t keeps the record")
        assert np.isinf(got2.t[n:][hit]).all() and (gp2.geom >= 0).all()
        check_rays(sc, r2[0], r2[1], KS, r2[2], r2[3], insts)
        check_points(sc, p2[0], KS, p2[1], insts)


@pytest.mark.parametrize("name", PC.CASES)
def test_boxes_and_sweeps_against_the_flat_list(psm, ctx, name):
    c = PC.case(name)
    seed = 600 + PC.CASES.index(name)
    with _world(psm, ctx, c) as sc:
        insts = sc.insts()
        lo, hi = PC.local_boxes(c, seed, N)
        _, count, _, _ = check_boxes(sc, lo, hi, KS, insts)
        assert (count > 0).sum() > 30 and (count == 0).sum() > 30
        lo, hi = PC.decisive_boxes(c, seed + 1, 10)
        assert lo.shape[0] <= 512
        _, count, _, irows = check_boxes(sc, lo, hi, KS, insts)
        assert (count > 0).sum() > 300 and len(np.unique(irows[:, 0])) > 30
        o, d, r, tm = PC.local_sweeps(c, seed + 2, N)
        want, winst = check_sweeps(sc, o, d, r, tm, insts)
        assert (winst >= 0).sum() > 100 and len(np.unique(winst)) > 20
        check_closed(sc, o, d, r, tm, want, winst, insts)
        o2, d2, r2, tm2 = PC.decisive_sweeps(insts, (o, d, r, tm))
        again, ainst = check_sweeps(sc, o2, d2, r2, tm2, insts)
        _same(again, want, "tmax at the contact keeps the contact")
        _same(sc.world.sphereCastOccluded(o2, d2, r2, tm2), winst >= 0, "sphereCastOccluded with tmax at the contact")


@pytest.mark.parametrize("name", PC.CASES)
def test_triangles_and_clearance_against_the_flat_list(psm, ctx, name):
    c = PC.case(name)
    seed = 700 + PC.CASES.index(name)
    with _world(psm, ctx, c) as sc:
        insts = sc.insts()
        q, rm = PC.local_triangles(c, seed, N)
        _, count, _, _ = check_tris(sc, q, KS, insts)
        assert (count > 0).sum() > 30 and (count == 0).sum() > 30
        q2 = PC.decisive_triangles(c, seed + 1, q)
        _, count, _, _ = check_tris(sc, q2, KS, insts)
        assert (count[::2] > 0).all()                                   # a shared vertex always counts
        hits, inst, within = check_clearance(sc, q, rm, insts)
        assert within.sum() > 100 and (hits[within, 2] > 0).sum() > 50 and (~within).sum() > 10 and len(np.unique(inst)) > 20
        hits2, inst2, within2 = check_clearance(sc, q, PC.decisive_clearance(insts, q), insts)
        assert within2.all() and (hits2[:, 2] > 0).sum() > 100


@pytest.mark.parametrize("name", PC.CASES)
def test_mesh_queries_against_the_flat_list(psm, ctx, name):
    """other is the torus at 6 poses from edge_pose, at bodies of every cluster (the far shifts among them): once with skip = None
    and once with the instance skipped that wins pose 0"""
    c = PC.case(name)
    tor = PC.base_meshes()[1]
    poses = PC.other_poses(c, 800 + PC.CASES.index(name), 6)
    with _world(psm, ctx, c) as sc:
        insts = sc.insts()
        oth = _hier(psm, ctx, tor)
        try:
            oleaves = sorted_leaves(psm, oth)
            assert oleaves.size == 64
            winner = int(WMD.flat(insts, tor, oleaves, poses[:1], np.inf, None, near=True)[3][0])
            assert winner >= 0
            for skip in (None, winner):
                flag, count, _, irows = check_mesh(sc, oth, tor, poses, KS, skip, insts)
                assert skip is None or not (irows == skip).any()
                for rmax in (np.inf, 0.25):
                    hits, geom, rec, inst = check_mesh_clearance(sc, oth, tor, poses, rmax, skip)
                    want = WMD.flat(insts, tor, oleaves, poses, rmax, skip, near=True)
                    for got, model, what in zip((hits, geom, rec, inst), want, ("closest", "closest instances", "clearance", "clearance instances")):
                        same_bits(got, model, "the flat model, rmax %s, skip %s: %s" % (rmax, skip, what))
                    assert (inst >= 0).all() or rmax < 1
                    assert skip is None or not (geom == skip).any()
            assert flag.any() and (count > 0).sum() > 10
        finally:
            oth.close()


@pytest.mark.parametrize("name", PC.CASES)
def test_voxel_grids_at_the_far_bodies(psm, ctx, name):
    """dims (10, 6, 9): partial bricks; the grid's origin lies at the far cluster, so the voxel planes are large float32 numbers"""
    c = PC.case(name)
    grid = PC.far_grid(c)
    with _world(psm, ctx, c) as sc:
        dense, count, owner = check_grid(psm, sc, grid, model=True)
        assert dense.any() and not dense.all() and len(np.unique(owner)) > (3 if name != "mixed" else 1)
    if name in ("far", "edge_far"):
        assert np.abs(grid[0]).max() > 5e3


@pytest.mark.parametrize("name", PC.CASES)
def test_the_seven_kinds_against_the_instanced_scene(psm, ctx, name):
    """the first 32 instances as a world and as an InstancedScene: two device paths that share no numpy model"""
    c = PC.case(name)
    with _world(psm, ctx, c, c.entries[:32]) as sc:
        rays, points, at = _local(name)
        rays, points = tuple(x[at < 32] for x in rays), tuple(x[at < 32] for x in points)
        members = sc.members()
        keep = RP.fully_well_posed(members, rays[0], rays[1])
        sure = RP.vote_rays_well_posed(members, points[0], IQ.INSIDE_DIRECTIONS)
        assert (~keep).mean() <= LEFT_OUT_CAP and (~sure).mean() <= LEFT_OUT_CAP
        rays, points = tuple(x[keep] for x in rays), tuple(x[sure] for x in points)
        flat = psm.InstancedScene(ctx, [(sc.ths[k], m) for k, m in c.entries[:32]])
        for r, p in ((rays, points), (PC.decisive_rays(sc.insts(), rays), PC.decisive_points(sc.insts(), points))):
            a, b = sc.world.intersect(*r), flat.intersect(*r)
            _same(a.buffer, b.buffer, "intersect")
            _same(a.geom, b.geom, "intersect inst")
            _same(sc.world.occluded(*r), flat.occluded(*r), "occluded")
            _same(sc.world.countHits(*r), flat.countHits(*r), "countHits")
            a, b = sc.world.closestPoint(*p), flat.closestPoint(*p)
            _same(a.buffer, b.buffer, "closestPoint")
            _same(a.geom, b.geom, "closestPoint inst")
            _same(sc.world.within(*p), flat.within(*p), "within")
            _same(sc.world.inside(p[0], 3), flat.inside(p[0], 3), "inside")
            a, b = sc.world.signedDistance(*p, 5), flat.signedDistance(*p, 5)
            _same(a.buffer, b.buffer, "signedDistance")
            _same(a.geom, b.geom, "signedDistance inst")
            assert (a.geom >= 0).sum() > 30


def test_set_transforms_into_the_hard_poses_and_back(psm, ctx):
    """a world built at benign poses (random_pose, shift 2) whose every instance is then moved to its edge_far pose: the boxes
    are redone with the new S -- |T| goes from 2 to 1e4, the rotations to the edge of the pose check -- and every family answers
    as the flat list at the new poses; then back, and the basic kinds again"""
    c = PC.case("edge_far")
    rng = np.random.RandomState(900)
    benign = [(k, NQ.random_pose(rng, reflect=bool(j & 1), shift=2.0)) for j, (k, _) in enumerate(c.entries)]
    hard = [m for _, m in c.entries]
    with _world(psm, ctx, c, benign) as sc:
        spread = _local("edge")                                          # local to bodies around the origin
        _check(sc, tuple(x[:128] for x in spread[0]), tuple(x[:128] for x in spread[1]), samples=(3,))
        sc.world.setTransforms(0, hard)
        assert np.array_equal(sc.world.transforms(), np.array(hard))
        insts = sc.insts()
        rays, points = _well_posed(sc, "edge_far")
        got, gp = _check(sc, rays, points, samples=(3,), insts=insts)
        assert (got.geom >= 0).sum() > 50 and (gp.geom >= 0).sum() > 50
        _check(sc, PC.decisive_rays(insts, rays), PC.decisive_points(insts, points), samples=(3,), insts=insts)
        lo, hi = PC.decisive_boxes(c, 901, 10)
        _, count, _, _ = check_boxes(sc, lo, hi, (4,), insts)
        assert (count > 0).sum() > 300
        first = PC.local_sweeps(c, 902, N)
        check_sweeps(sc, *PC.decisive_sweeps(insts, first), insts)
        q, _ = PC.local_triangles(c, 903, N)
        _, _, within = check_clearance(sc, q, PC.decisive_clearance(insts, q), insts)
        assert within.all()
        dense, _, _ = check_grid(psm, sc, PC.far_grid(c), model=True)
        assert dense.any() and not dense.all()
        sc.world.setTransforms(0, [m for _, m in benign])
        _check(sc, tuple(x[:128] for x in spread[0]), tuple(x[:128] for x in spread[1]), samples=(3,))
