"""CPU tests (no GPU) of the clearance queries over an instance world (psm_world_tri_closest_dev / psm_world_tri_within_dev,
world_tri_dist.hip; InstanceWorld.closestToTriangle / withinOfTriangle): the restatement of the top-level gap
test, the prune and the walk (world_tri_dist_query_model part (b)) answers bit for bit what the flat list answers (part (a)) on a
lattice world and on a general one, for both queries, and culls; an identity world of one is the bare hierarchy; ties; the
distance against a float64 reading; the prune's margin at both levels, measured in float64; invalid queries and the rmax edge
cases; the exports, the header text, the Python surface and the refusals that need no device; what world_tri_dist.hip compiles
to; the candidate test on the host under sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import test_tri_dist_query_cpu as TDT
import test_world_box_cpu as WBT
import test_world_tri_cpu as WTT
import tri_dist_query_model as TD
import world_box_query_model as WB
import world_tri_dist_query_model as WD
import world_tri_query_model as WT
from util import ROOT, csrc_asm, kernel_asm, kernel_meta

F = np.float32
D = np.float64


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    ua, ub = (x.view(np.uint32) if x.dtype == F else x for x in (a, b))
    bad = np.nonzero(np.atleast_1d((ua != ub).reshape(a.shape[0], -1).any(axis=1)))[0]
    assert bad.size == 0, "%s: %d differ, first %d: %s against %s" % (what, bad.size, bad[0], a[bad[0]], b[bad[0]])


def _walk_is_flat(insts, q, rmax, what):
    """(b) == (a) for both queries; returns (a)'s answer, the pairs, and the instances the closest / within walks entered"""
    pairs = [WD.pair_records(i, q) for i in insts]
    hits, inst, within = WD.flat(insts, q, rmax, pairs)
    world = WD.TriDistWorld(insts)
    (h, g), ent, _ = world.closest(q, rmax, pairs=pairs)
    _same(h, hits, what + ": records")
    _same(g, inst, what + ": instances")
    f, ent_w, _ = world.closest(q, rmax, within=True, pairs=pairs)
    _same(f, within, what + ": within")
    assert np.array_equal(within, hits.view(np.int32)[:, 3] >= 0) and np.array_equal(inst >= 0, within)
    return (hits, inst, within), pairs, (ent, ent_w), world


def _mixed_rmax(rng, n, scale):
    """a third +inf, a third 0, the rest over three decades of `scale`"""
    rm = (scale * 10.0 ** rng.uniform(-3, 0, n)).astype(F)
    rm[::3] = np.inf
    rm[1::3] = 0
    return rm


def _lattice_queries(insts, step):
    """test_world_tri_cpu's lattice queries, thinned, and some of them moved off the block of cubes by whole and half units (exact
    in float32): at a distance from everything"""
    q = WTT.lattice_queries(insts)
    off = np.array([[4, 0, 0], [0, -4.5, 0], [2.5, 2.5, 2.5], [8, 8, 8], [0, 0, 3.5], [-3, 1, 0]], F)
    moved = q[:4 * 120:4] + off[np.arange(120) % 6][:, None, :]
    assert np.array_equal((moved.astype(D) - q[:4 * 120:4].astype(D)), np.broadcast_to(off[np.arange(120) % 6][:, None, :].astype(D), moved.shape))
    return np.concatenate([q[::step], moved])


def test_lattice_world_walk_is_the_flat_answer():
    insts = WBT.lattice_world()
    q = _lattice_queries(insts, 4)
    rng = np.random.RandomState(41)
    rm = _mixed_rmax(rng, q.shape[0], 0.05)
    (hits, inst, within), pairs, (ent, ent_w), _ = _walk_is_flat(insts, q, rm, "lattice")
    for got, want, what in zip(WD.flat_near(insts, q, rm), (hits, inst, within), ("records", "instances", "within")):
        _same(got, want, "lattice: flat_near against flat, " + what)
    dist = hits[:, 2]
    assert (~within).sum() > 10 and (within & (dist > 0)).sum() > 10 and (dist == 0).sum() > 10
    assert (~within[1::3]).any() and within[1::3].any()                   # rmax = 0: the touching ones alone
    # coincident instances (0, 1, 2 come again as 48, 49, 50): the lower instance wins
    d2 = np.concatenate([p[0] for p in pairs], axis=1)
    owner = np.concatenate([np.full(p[5].size, j) for j, p in enumerate(pairs)])
    tied = 0
    for i in np.nonzero(within)[0]:
        w2 = pairs[inst[i]][0][i, list(pairs[inst[i]][5]).index(hits.view(np.int32)[i, 3])]
        same = np.unique(owner[d2[i] == w2])
        tied += same.size > 1
        assert inst[i] == same.min()
    assert tied > 10 and not np.isin(inst, (48, 49, 50)).any() and np.isin(inst, (0, 1, 2)).any()
    mean = np.mean([len(e) for e in ent]), np.mean([len(e) for e in ent_w])
    print("lattice: %d instances, entered on average %.1f (closest), %.1f (within)" % (len(insts), mean[0], mean[1]))
    assert mean[0] < 0.5 * len(insts) and mean[1] < 0.5 * len(insts)      # and it culls


def test_general_world_walk_is_the_flat_answer():
    rng = np.random.RandomState(42)
    insts = WBT.general_world()
    q = WTT.triangles_around(rng, insts, 24)
    rm = _mixed_rmax(rng, q.shape[0], 3.0)
    (hits, inst, within), _, (ent, ent_w), _ = _walk_is_flat(insts, q, rm, "general")
    for got, want, what in zip(WD.flat_near(insts, q, rm), (hits, inst, within), ("records", "instances", "within")):
        _same(got, want, "general: flat_near against flat, " + what)               # the shortcut the GPU tests' yardstick takes
    dist = hits[:, 2]
    assert not within[-4:].any() and all(e == [] for e in ent[-4:])                        # the invalid queries
    assert (~within[:-4]).sum() > 10 and (within & (dist > 0)).sum() > 10 and (dist == 0).sum() > 10
    assert (inst == len(insts) - 1).any()                                                  # the +1000 member is found
    first = np.array([e[0] if e else -1 for e in ent])
    assert ((inst >= 0) & (first != inst)).sum() > 5                                       # a winner beyond the first entered
    mean = np.mean([len(e) for e in ent[:-5]]), np.mean([len(e) for e in ent_w[:-5]])
    print("general: %d instances, entered on average %.1f (closest), %.1f (within)" % (len(insts), mean[0], mean[1]))
    assert mean[0] < 0.5 * len(insts) and mean[1] < 0.5 * len(insts)
    # every valid query with rmax = +inf finds something, whatever it entered first
    assert within[:-4][np.isinf(rm[:-4])].all()


def test_identity_world_of_one_is_the_bare_hierarchy():
    rng = np.random.RandomState(43)
    tris = WBT._soup(rng, 60)
    cand = rng.permutation(60)[:50]
    eye = WBT._pose(np.eye(3), np.zeros(3))
    inst = (tris, cand, eye, WB.plain_fit(tris))
    q = WTT.triangles_around(rng, [inst], 150)
    rm = _mixed_rmax(rng, q.shape[0], 1.0)
    want, want_within = TD.query(tris, cand, q, rm)
    (hits, g, within), _, _, _ = _walk_is_flat([inst], q, rm, "identity")
    _same(hits, want, "identity world of one: records")
    _same(within, want_within, "identity world of one: within")
    assert np.array_equal(g, np.where(within, 0, -1)) and within.any() and not within.all()


def test_ties_go_to_the_lowest_instance_then_the_lowest_triangle():
    c = WBT.cube()
    M = WB.plain_fit(c)
    eye = WBT._pose(np.eye(3), np.zeros(3))
    # a point above the middle of the top face's diagonal is equally far from the face's two triangles: the lower id
    top = [k for k in range(12) if (c[k, :, 2] == 1).all()]
    assert len(top) == 2
    q = np.array([[[0.5, 0.5, 1.5]] * 3], F)
    for cand in (np.arange(12), np.arange(12)[::-1]):
        (hits, g, _), pairs, _, _ = _walk_is_flat([(c, cand, eye, M)], q, np.inf, "two triangles")
        assert hits[0, 2] == 0.5 and hits.view(np.int32)[0, 3] == min(top) and g[0] == 0
        assert (pairs[0][0][0] == F(0.25)).sum() == 2
    # coincident instances, at a distance: the lower instance
    three = [(c, np.arange(12), eye, M), (c, np.arange(12), WBT._pose(np.eye(3), [5, 0, 0]), M), (c, np.arange(12), eye, M)]
    (hits, g, _), _, _, _ = _walk_is_flat(three, q, np.inf, "coincident")
    assert g[0] == 0 and hits[0, 2] == 0.5
    (hits, g, _), _, _, _ = _walk_is_flat(three[::-1], np.concatenate([q, q + F(5) * np.array([1, 0, 0], F)]), np.inf, "coincident, reversed")
    assert list(g) == [0, 1]
    # a query that cuts through several instances: dist 0 and the lowest (instance, triangle) that meets it
    insts = WBT.lattice_world()
    cut = WTT.lattice_queries(insts)[:500:3]
    (hits, g, _), _, _, _ = _walk_is_flat(insts, cut, np.inf, "cutting")
    _, count, trows, irows, _ = WT.flat(insts, cut, k=1)
    meets = count > 0
    assert meets.sum() > 20 and (count > 3).sum() > 10 and (~meets).sum() > 5
    assert np.array_equal(hits[:, 2] == 0, meets)
    assert np.array_equal(hits.view(np.int32)[meets, 3], trows[meets, 0]) and np.array_equal(g[meets], irows[meets, 0])


def _well_shaped_world(rng, members, per):
    insts = []
    for j in range(members):
        t, _ = TDT._well_shaped(rng, per)
        tris = (t + rng.uniform(-1, 1, (per, 1, 3))).astype(F)
        pose = WBT._pose(WBT._rotation(rng, j % 2 == 1), rng.uniform(-2, 2, 3))
        insts.append((tris, np.arange(per), pose, WB.plain_fit(tris)))
    return insts


def test_distance_against_the_float64_reading():
    """every pair's float32 distance -- the posed candidate as the kernel holds it, read in float64 -- stays within the
    clearance queries' own bound, TOL L (test_tri_dist_query_cpu: the same constant), and so does the winner's"""
    rng = np.random.RandomState(44)
    insts = _well_shaped_world(rng, 3, 40)
    tq, _ = TDT._well_shaped(rng, 150)
    q = (tq + rng.uniform(-3, 3, (150, 1, 3))).astype(F)
    (hits, inst, within), pairs, _, _ = _walk_is_flat(insts, q, np.inf, "well shaped")
    assert within.all()
    ref_min = np.full(150, np.inf)
    worst = 0.0
    for j, i_ in enumerate(insts):
        t64 = WTT.posed_triangles(i_)                                                   # [C, 3, 3], C = 40, sorted candidates
        assert min(TDT._sines(t64).min(), TDT._sines(q).min()) >= 0.19
        tt = np.repeat(t64[None], 150, axis=0).reshape(-1, 3, 3)
        qq = np.repeat(q.astype(D)[:, None], 40, axis=1).reshape(-1, 3, 3)
        ref = TDT._f64_reading(tt, qq).reshape(150, 40)
        L = TDT._span(tt, qq).reshape(150, 40)
        err = np.abs(np.sqrt(pairs[j][0].astype(D)) - ref) / L
        worst = max(worst, err.max())
        assert err.max() <= TDT.TOL, (j, err.max())
        ref_min = np.minimum(ref_min, ref.min(axis=1))
    print("the largest error of a pair: %.3g L (asserted: %.3g L)" % (worst, TDT.TOL))
    span = np.abs(q.astype(D)).max() + 4.0                                               # every pair's L is below this
    assert (np.abs(hits[:, 2].astype(D) - ref_min) <= TDT.TOL * span).all()


def _edge_world(seed, members=8):
    """the general world's kind of member under poses at the edge of the pose check (R^T R off by up to 1e-5)"""
    rng = np.random.RandomState(seed)
    insts = []
    for j in range(members):
        tris = WBT._soup(rng, 40, 10.0 ** rng.uniform(-1, 0.5))
        t = rng.uniform(-2, 2, 3) if j % 2 == 0 else rng.normal(size=3) * 10.0 ** rng.uniform(0, 2)
        insts.append((tris, np.arange(40), WBT._edge_pose(rng, t), WBT.fit_like(rng, tris, j % 3)))
    return insts


def test_prune_margin_at_both_levels_in_float64():
    """The chain of DESIGN.md 4.25, measured: over every query with a winner and every box above the winning leaf -- the child
    boxes of the top-level tree above its instance, the boxes of a real tree (tri_dist_query_model.build_tree: fp16, padded,
    unions) above the leaf inside it -- the kernel's float32 lower bound LB^2 stays below the winner's float32 forward-posed
    d2; a winner at d2 == 0 has LB^2 == 0 everywhere. Measured maxima of LB^2 / d2 (printed): see DESIGN.md 4.25."""
    tops, insides = [], []
    for name, insts, seed in (("general", WBT.general_world(), 45), ("lattice", WBT.lattice_world(), 46), ("edge poses", _edge_world(47), 48)):
        rng = np.random.RandomState(seed)
        q = _lattice_queries(insts, 8) if name == "lattice" else WTT.triangles_around(rng, insts, 24)[:-4]
        world = WD.TriDistWorld(insts)
        hits, inst, within = WD.flat(insts, q, np.inf)
        trees = [TD.build_tree(i[3], i[0], np.sort(i[1])) for i in insts]
        top, inside, bad = WD.margin_figures(world, q, hits, inst, trees)
        print("%s: %d winners at d2 > 0; the largest LB^2 / d2: %.6f at the top level, %.6f inside an instance"
              % (name, top.size, top.max(), inside.max()))
        assert bad == 0 and top.size > 50
        tops.append(top.max())
        insides.append(inside.max())
    assert max(tops) < 1.0 and max(insides) < 1.0
    assert max(tops) > 0.5 and max(insides) > 0.5                       # and the bounds bite: they are no token


def test_invalid_queries_and_rmax_edges():
    c = WBT.cube()
    one = np.array([[[0, 0, 3], [1, 0, 3], [0, 1, 3]]], F)              # a one-triangle mesh: the lone leaf of enter()
    eye = WBT._pose(np.eye(3), np.zeros(3))
    insts = [(c, np.arange(12), eye, WB.plain_fit(c)), (one, np.arange(1), eye, WB.plain_fit(one))]
    base = np.array([[0.25, 0.25, 2.0], [0.75, 0.25, 2.0], [0.25, 0.75, 2.0]], F)       # 1 above the cube, 1 below the triangle
    q = np.repeat(base[None], 12, axis=0)
    rm = np.array([np.inf, 1.0, np.nextafter(F(1), F(0)), 0.0, -0.0, 1e-30, np.nan, -1.0, -np.inf, np.inf, np.inf, np.inf], F)
    q[9, 0, 0], q[10, 1, 2], q[11, 2, 1] = np.nan, np.inf, -np.inf
    (hits, inst, within), _, (ent, _), _ = _walk_is_flat(insts, q, rm, "edges")
    assert list(within) == [True, True] + [False] * 10
    assert list(inst[:2]) == [0, 0] and (hits[:2, 2] == 1).all()         # equally far from both: the lower instance
    _same(hits[2:], TD.miss_records(10), "misses")
    assert all(e == [] for e in ent[6:])                                # an invalid query never walks
    # on the mesh: rmax = 0 and -0 find it, a tiny rmax too
    on = np.repeat(c[3][None], 3, axis=0)
    (hits, inst, within), _, _, _ = _walk_is_flat(insts, on, np.array([0.0, -0.0, 1e-30], F), "on the mesh")
    assert within.all() and (hits[:, 2] == 0).all() and (inst == 0).all()
    # the flat answer of an empty world and of a world whose only instance has an empty hierarchy: misses
    for empty in ([], [(np.zeros((0, 3, 3), F), np.zeros(0, np.int64), eye)]):
        h, g, w = WD.flat(empty, q, np.inf)
        _same(h, TD.miss_records(12), "empty")
        assert (g == -1).all() and not w.any()
    (h, g), e, _ = WD.TriDistWorld([]).closest(q, np.inf)
    _same(h, TD.miss_records(12), "empty world, the walk")
    assert (g == -1).all() and all(x == [] for x in e)


# ---- the library, the headers, the kernels ---------------------------------------------------------------------------------------

ENTRIES = ("psm_world_tri_closest_dev", "psm_world_tri_within_dev")
METHODS = ("closestToTriangle", "withinOfTriangle")


def test_library_exports_the_world_clearance_queries(psm):
    lib = psm.lib()
    header = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    for s in ENTRIES:
        assert hasattr(lib, s) and s in psm.EXPORTS and re.search(r"\b%s\(" % s, header), s
    assert "clearance queries over a world (new; no reference counterpart; DESIGN.md 4.25)" in header
    assert "tri_dist(fwd_point(m, v0), fwd_vec(m, e1), fwd_vec(m, e2), a, b, c)" in header
    assert "dist == 0 exactly for the pairs psm_world_tri_overlaps_dev counts" in header
    assert "an identity world of one answers as psm_bvh_tri_closest_dev" in header
    for m in METHODS:
        assert callable(getattr(psm.InstanceWorld, m)), m
        for other in (psm.QueryScene, psm.InstancedScene, psm.TriangleHierarchy):
            assert not hasattr(other, m), (other, m)
    assert "closestToTriangle()" in psm.InstanceWorld.__doc__ and "closestToTriangle()" in psm.TriangleHierarchy.triClosest.__doc__
    hpp = open(os.path.join(ROOT, "include", "Prismarine", "InstanceWorld.hpp")).read()
    inl = open(os.path.join(ROOT, "include", "Prismarine", "InstanceWorld.inl")).read()
    for m, s in zip(METHODS, ENTRIES):
        assert re.search(r"int %s\(const psm_tri_dist_query \*" % m, hpp) and "InstanceWorld::%s(" % m in inl and s + "(world," in inl
    csrc = os.path.join(ROOT, "prismarine-core_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRC := .*\bworld_tri_dist\.hip\b", mk, re.M) and re.search(r"^world_tri_dist\.o:.*psm_tri_dist_dev\.h", mk, re.M)
    assert "int world_tri_dist_launch(psm_ctx* c, bool within, uint32_t grid, const WorldArgs& a);" in open(os.path.join(csrc, "psm_world_dev.h")).read()
    body = open(os.path.join(csrc, "world_tri_dist.hip")).read()
    assert "struct WorldTriDistBody : WorldBoxPrune" in body and "tri_dist_lb2(" in body and "asm" not in body
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "closestToTriangle" in open(os.path.join(ROOT, doc)).read(), doc


def test_world_clearance_refusals_that_need_no_device(psm):
    """no world: the code the other world queries give, before anything is looked at; the Python layer packs [n, 3, 3] and [n, 9]
    and rmax into psm_tri_dist_query records; a single hierarchy's records have no instance"""
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    other = lib.psm_world_intersect_dev(None, None, ctypes.c_size_t(1), None, None)
    assert other != 0
    assert lib.psm_world_tri_closest_dev(None, p, ctypes.c_size_t(1), p, p) == other
    assert lib.psm_world_tri_closest_dev(None, None, ctypes.c_size_t(0), None, None) == other
    assert lib.psm_world_tri_within_dev(None, p, ctypes.c_size_t(1), p) == other
    assert lib.psm_world_tri_within_dev(None, None, ctypes.c_size_t(0), None) == other
    assert not any(buf)

    class NoCall:   # a world that cannot make a call
        ctx = None
        _scene = True
        seen = []

        def _launch_np(self, packed, out, name):
            self.seen.append((packed, out, name))
            raise AssertionError("a launch was made")
        _tri_dist_query = psm.InstanceWorld._tri_dist_query
        closestToTriangle = psm.InstanceWorld.closestToTriangle
        withinOfTriangle = psm.InstanceWorld.withinOfTriangle
    q = np.arange(18, dtype=F)
    for shape in ((2, 3, 3), (2, 9)):
        for call, out, name in ((lambda x: NoCall().closestToTriangle(x), "trihits", "psm_bvh_tri_closest_dev"),      # (_call renames it)
                                (lambda x: NoCall().closestToTriangle(x, F([0.5, 2])), "trihits", "psm_bvh_tri_closest_dev"),
                                (lambda x: NoCall().withinOfTriangle(x, 0.25), "bool", "psm_bvh_tri_within_dev")):
            with pytest.raises(AssertionError, match="a launch was made"):
                call(q.reshape(shape))
            packed, got_out, got_name = NoCall.seen[-1]
            assert (got_out, got_name) == (out, name) and packed.shape == (2, 12) and packed.dtype == F
            assert np.array_equal(packed.reshape(2, 3, 4)[:, :, :3].reshape(2, 9), q.reshape(2, 9)) and not packed[:, [7, 11]].any()
    assert list(NoCall.seen[-1][0][:, 3]) == [0.25, 0.25] and list(NoCall.seen[-2][0][:, 3]) == [0.5, 2] and np.isinf(NoCall.seen[-3][0][:, 3]).all()
    assert psm.QueryTriHits(TD.miss_records(2)).geom is None                        # a single hierarchy's: as before
    rec = TD.miss_records(3)
    rec[0, :2], rec[0, 2], rec[0, 4:6] = (0.25, 0.5), 1.0, (0.5, 0.25)
    rec.view(np.int32)[0, 3] = 1
    rec[2, 2] = 2.0
    rec.view(np.int32)[2, 3] = 0
    hits = psm.QueryTriHits(rec, np.array([1, -1, 0], np.int32))
    assert list(hits.geom) == [1, -1, 0] and len(hits) == 3
    posed = [np.arange(18, dtype=F).reshape(2, 3, 3), np.arange(18, dtype=F).reshape(2, 3, 3) + F(100)]
    qs = np.arange(27, dtype=F).reshape(3, 3, 3)
    pw, pq = hits.points_world(posed, qs)
    t = posed[1][1]
    assert np.array_equal(pw[0], (t[0] + F(0.25) * (t[1] - t[0])) + F(0.5) * (t[2] - t[0])) and np.array_equal(pw[2], posed[0][0][0])
    assert np.array_equal(pq[0], (qs[0, 0] + F(0.5) * (qs[0, 1] - qs[0, 0])) + F(0.25) * (qs[0, 2] - qs[0, 0]))
    assert np.isnan(pw[1]).all() and np.isnan(pq[1]).all()
    with pytest.raises(ValueError):
        psm.QueryTriHits(rec).points_world(posed, qs)


# What each kernel reaches with the Makefile's flags, as ceilings: VGPRs, the waves per SIMD its
# __launch_bounds__ ask for (what the unforced figure gives: 512 / VGPRs rounded up to 8), no scratch, no spills, no lane writes,
# the LDS of the 16-entry stack.
WORLD_CLEARANCE_KERNELS = {"world_query_tri_closest": (142, 3), "world_query_tri_within": (171, 2)}


def test_world_clearance_kernels_codegen():
    asm = csrc_asm("world_tri_dist.hip")
    assert asm.count(".amdhsa_kernel ") == 3                                   # the two walks and the empty world's fill
    src = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "world_tri_dist.hip")).read()
    bounds = re.search(r"WORLD_TRI_DIST_WAVES = (\d+), WORLD_TRI_DIST_WITHIN_WAVES = (\d+)", src)
    assert [int(x) for x in bounds.groups()] == [v[1] for v in WORLD_CLEARANCE_KERNELS.values()]
    for name, (vgprs, waves) in WORLD_CLEARANCE_KERNELS.items():
        blk, body = kernel_asm(asm, "_ZN3psm%d%sENS_9WorldArgsE" % (len(name), name))

        def meta(key):
            return kernel_meta(blk, key)
        assert meta("vgpr_count") <= vgprs, (name, meta("vgpr_count"))
        assert 512 // ((vgprs + 7) // 8 * 8) == waves, name                    # the bound asks for what the registers give
        assert meta("vgpr_spill_count") == 0 and meta("sgpr_spill_count") == 0, name
        assert meta("private_segment_fixed_size") == 0 and "scratch_" not in body, name
        assert "v_writelane_b32" not in body, name
        assert meta("group_segment_fixed_size") == 16 * 64 * 4, name          # the stack
        assert "v_div_fixup_f32" in body and "v_sqrt_f32" in body and "v_pk_" not in body, name


def test_posed_clearance_test_on_the_host_is_the_model(tmp_path):
    """fwd_point / fwd_vec of psm_world_box_dev.h and tri_dist of psm_tri_dist_dev.h as world_tri_dist.hip's leaf() joins them,
    as a stand-alone host program with its own main, built with -ffp-contract=off and the address and undefined-behaviour
    sanitizers and run as a process of its own on the CPU: d2 and the four weights of every record are model (a)'s bit for bit"""
    hipcc = "/opt/rocm/bin/hipcc"
    exe, fin, fout = (str(tmp_path / x) for x in ("world_tri_dist_host", "records.bin", "out.bin"))
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "prismarine-core_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "world_tri_dist_host.cpp"), "-o", exe])
    rec = WTT._host_records()
    assert rec.shape[1] == 30 and rec.shape[0] >= 5000
    rec.tofile(fin)
    done = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode(errors="replace")
    got = np.fromfile(fout, F).reshape(-1, 5)
    want = np.zeros((rec.shape[0], 5), F)
    _, first, inverse = np.unique(rec[:, :12], axis=0, return_index=True, return_inverse=True)
    with np.errstate(all="ignore"):
        for g, f in enumerate(first):                                       # the model poses per pose: the records grouped by it
            rows = np.nonzero(inverse.reshape(-1) == g)[0]
            pose = rec[f, :12].reshape(3, 4)
            v0, e1, e2 = WB.fwd_point(pose, rec[rows, 12:15]), WB.fwd_vec(pose, rec[rows, 15:18]), WB.fwd_vec(pose, rec[rows, 18:21])
            want[rows] = np.stack(TD.tri_dist(v0, e1, e2, rec[rows, 21:24], rec[rows, 24:27], rec[rows, 27:30]), axis=1)
    assert got.shape == want.shape
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    bad = np.nonzero(~same.all(axis=1))[0]
    assert bad.size == 0, "%d differ, first %d: %s got %s want %s" % (bad.size, bad[0], rec[bad[0]], got[bad[0]], want[bad[0]])
    assert (want[:, 0] == 0).sum() > 100 and (want[:, 0] > 0).sum() > 1000 and np.isnan(want[:, 0]).any()
