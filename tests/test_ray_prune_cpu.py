"""CPU tests (no GPU) of the ray queries' prune against the well-posed rule (tests/ray_prune_model.py): on the
oracle's build of every hierarchy, under every build matrix and for every class of rays, a well-posed accepted hit passes the
slab interval of its own leaf box (ray_axis / slab of psm_query_dev.h restated in float32), so the walk cannot lose it; the flat
classes do hold hits that are not well-posed and that the interval excludes (the rule is not vacuous); and the rays the rule
leaves to two-sided bounds are few (the rule cannot hide failures). The sparse sets the GPU tests hold the kernels to are the
brute-force models' (query_model, kbest_query_model, inside_query_model)."""
import functools

import numpy as np
import pytest

import inside_query_model as IQ
import kbest_query_model as KQ
import query_model as Q
import ray_prune_model as RP
from test_gpu_fuzz import fuzz_case, fuzz_opt
from test_gpu_point_query import ROT_SCALE, SHEAR

F = np.float32

MATRICES = [("identity", None), ("rotate_scale", ROT_SCALE), ("shear", SHEAR)] + [
    ("fuzz_opt%d" % s, fuzz_opt(np.random.RandomState(5000 + s))) for s in range(4)]
HIERARCHIES = ["sponza_like", "cornell", "deep"] + ["fuzz%d" % s for s in range(8)]


def _camera_rays(oracle, scenes, sc, w, h, time=7):
    cam = scenes.camera_matrices(sc["eye"], sc["view"], w, h)
    rays, *_ = oracle.camera(oracle.make_cfg(w, h), cam[0], cam[1], time)
    return rays["origin"].copy(), rays["direct"].copy()


def hierarchy(name, oracle, scenes):
    """(tris [T, 3, 3], own origins, own directions) of a named hierarchy: a scene with its camera rays, the deep fixture and the
    fuzz soups with their own"""
    if name == "sponza_like":
        sc = scenes.sponza_like(3001)
        return (sc["tris"].reshape(-1, 3, 3),) + _camera_rays(oracle, scenes, sc, 64, 32)
    if name == "cornell":
        sc = scenes.cornell()
        return (sc["tris"].reshape(-1, 3, 3),) + _camera_rays(oracle, scenes, sc, 64, 32)
    if name == "deep":
        return Q.deep_fixture(rays=2048)
    tris, o, d, _ = fuzz_case(int(name[4:]))
    return tris, o, d


@functools.lru_cache(maxsize=None)
def _pairs(name, oracle, scenes):
    """the hierarchy and, per class of rays, the accepted pairs: they depend on neither the build matrix nor the window"""
    tris, oo, od = hierarchy(name, oracle, scenes)
    n = 2048 if tris.shape[0] <= 5000 else 512
    rng = np.random.RandomState(77 + HIERARCHIES.index(name))
    return tris, {c: RP.accepted_pairs(tris, o, d) for c, (o, d) in RP.ray_classes(rng, tris, oo, od, n).items()}


@functools.lru_cache(maxsize=None)
def study(name, mname, oracle, scenes):
    """One hierarchy under one matrix: per class the RaySets of the default window and, over ALL accepted pairs of the leaves
    (whatever their t: a window can hold any of them), whether each passes the interval of its own leaf box."""
    tris, pairs = _pairs(name, oracle, scenes)
    b = oracle.build_scene(tris, dict(MATRICES)[mname])
    ids, boxes = RP.leaf_boxes(b["leafs"])
    row = np.full(tris.shape[0], -1, np.int64)
    row[ids] = np.arange(ids.size)
    out = {}
    for c, p in pairs.items():
        S = RP.RaySets(tris, ids, b["M"], None, None, -np.inf, np.inf, pairs=p)
        near, far = RP.leaf_interval(b["M"], boxes[row[S.tri]], p["o"][S.r], p["dn"][S.r])
        # The walk keeps a box iff (near <= far) & (near <= limit) & (far >= tmin), limit = tmax or the best t so far. For every
        # window and limit that admit t (tmin <= t <= limit) that follows from near <= far, near <= t, far >= t -- and the last is
        # needed as it stands: a window may be tmin = tmax = t itself.
        passes = (near <= far) & (near <= S.t) & (far >= S.t)
        out[c] = (S, passes, RP.RaySets(tris, ids, b["M"], None, None, 0.0, np.inf, pairs=p))
    return out


@pytest.mark.parametrize("name", HIERARCHIES)
def test_the_prune_keeps_every_well_posed_hit(oracle, scenes, name):
    """The leaf's own box suffices: every ancestor's box is a superset of it (refit's half2 min / max of the children), and each
    slab distance is one fmaf of a box plane with the ray's constants -- monotone in the plane -- so an interval that admits t at
    the leaf admits it at every ancestor."""
    for mname, opt in MATRICES:
        for c, (S, passes, _) in study(name, mname, oracle, scenes).items():
            bad = np.nonzero(S.wp & ~passes)[0]
            assert bad.size == 0, (name, mname, c, bad.size, S.r[bad[:4]], S.tri[bad[:4]], S.t[bad[:4]], S.excess[bad[:4]])


def test_a_box_plane_at_one_needs_the_constant_margin(oracle, scenes):
    """What the margin's constant 2^-12 is for: a leaf at the top of the scene has its padded corner in
    [1, 1 + PZERO), where fp16's half-ulp is 2^-11 and the rounding can take all but 1.2e-5 of the padding. On the deep fixture
    under the third random matrix the margin without the constant loses a well-posed hit at such a plane; with it, none."""
    tris, pairs = _pairs("deep", oracle, scenes)
    b = oracle.build_scene(tris, dict(MATRICES)["fuzz_opt2"])
    ids, boxes = RP.leaf_boxes(b["leafs"])
    row = np.full(tris.shape[0], -1, np.int64)
    row[ids] = np.arange(ids.size)
    p = pairs["tilt1e-5"]
    S = RP.RaySets(tris, ids, b["M"], None, None, -np.inf, np.inf, pairs=p)
    box = boxes[row[S.tri]]
    lost = {}
    for grow in (0.0, 2.0 ** -12):
        near, far = RP.leaf_interval(b["M"], box, p["o"][S.r], p["dn"][S.r], grow=grow)
        lost[grow] = np.nonzero(S.wp & ~((near <= far) & (near <= S.t) & (far >= S.t)))[0]
    assert lost[0.0].size >= 1 and lost[2.0 ** -12].size == 0
    assert (box[lost[0.0], 3:] == F(1.0)).any(axis=1).all()


def test_the_rule_is_not_vacuous(oracle, scenes):
    """over the two flattest classes on sponza_like(3001), some accepted hit is not well-posed and fails its leaf's interval"""
    for mname, opt in MATRICES[:3]:
        st = study("sponza_like", mname, oracle, scenes)
        lost = sum(int((~st[c][0].wp & ~st[c][1]).sum()) for c in ("tilt1e-7", "tilt0"))
        assert lost >= 1, (mname, lost)


@pytest.mark.parametrize("name", HIERARCHIES)
def test_the_rule_leaves_few_rays_out(oracle, scenes, name):
    for mname, opt in MATRICES:
        for c, (_, _, S) in study(name, mname, oracle, scenes).items():
            if (name, c) in RP.NO_SHARE:   # (a class that is degenerate on this hierarchy: listed there with its reason)
                continue
            if c in RP.SHARE_CAP:
                RP.check_shares(S, RP.SHARE_CAP[c], "%s %s %s" % (name, mname, c))
            elif name == "sponza_like":
                RP.check_shares(S, RP.FLAT_CAP[c], "%s %s %s" % (name, mname, c), at_least=1)


def test_the_sparse_sets_are_the_brute_force_models(oracle, scenes):
    """RaySets' closest hit, first hits and |A| are query_model.query, kbest_query_model.first_hits and inside_query_model.count"""
    tris, oo, od = hierarchy("cornell", oracle, scenes)
    rng = np.random.RandomState(3)
    o, d = (np.concatenate(x) for x in zip((oo[:300], od[:300]), RP.grazing_rays(rng, tris, 300, 0.0), RP.box_rays(rng, tris, 300)))
    d[5], o[6] = [0, 0, 0], [np.nan, 0, 0]
    tmin = rng.uniform(-2, 400, o.shape[0]).astype(F)
    tmax = (tmin + rng.uniform(-10, 600, o.shape[0])).astype(F)
    tmax[::7], tmin[::5], tmin[11] = np.inf, -np.inf, np.nan
    b = oracle.build_scene(tris)
    cand = b["leafs"]["pdata"][:, 3]
    S = RP.RaySets(tris, cand, b["M"], o, d, tmin, tmax)
    exp, anyh = Q.query(tris, cand, o, d, tmin, tmax)
    assert np.array_equal(S.closest().view(np.uint32), exp.view(np.uint32)) and np.array_equal(S.nA > 0, anyh)
    rows, count = KQ.first_hits(tris, cand, o, d, 4, tmin, tmax)
    mine, mcount = S.first_hits(4)
    assert np.array_equal(mine.view(np.uint32), rows.view(np.uint32)) and np.array_equal(mcount, count)
    assert np.array_equal(S.nA, IQ.count(tris, cand, o, d, tmin, tmax))
    # ... and the contract accepts the models' own answers, and refuses an invented hit, a missed one and a wrong count
    RP.check_intersect(S, exp)
    RP.check_occluded(S, anyh)
    RP.check_count(S, S.nA)
    RP.check_first_hits(S, 4, rows, count)
    hit = np.nonzero(anyh & S.full)[0][0]
    wrong = exp.copy()
    wrong[hit] = RP._miss_rows((1,))
    for fn, arg in ((RP.check_intersect, wrong), (RP.check_occluded, np.where(np.arange(o.shape[0]) == hit, False, anyh)),
                    (RP.check_count, S.nA + (np.arange(o.shape[0]) == hit))):
        with pytest.raises(AssertionError):
            fn(S, arg)


def test_well_posed_is_the_stated_rule():
    """a point HEADROOM outside the normalised box on one axis is well-posed, the next double is not; a NaN point is not"""
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], F)
    M = np.array([[0.5, 0, 0, 0.25], [0, 0.5, 0, 0.25], [0, 0, 0.5, 0.25], [0, 0, 0, 1]], F)
    o, dn = np.array([[0.25, 0.25, -1.0]]), np.array([[0.0, 0.0, 1.0]])
    t_edge = 1.0 + RP.HEADROOM / 0.5
    assert RP.well_posed(tri, M, o, dn, np.array([1.0]), np.array([0]))[0]
    assert RP.well_posed(tri, M, o, dn, np.array([t_edge * (1 - 1e-12)]), np.array([0]))[0]
    assert not RP.well_posed(tri, M, o, dn, np.array([t_edge * (1 + 1e-9)]), np.array([0]))[0]
    assert not RP.well_posed(tri, M, o, dn, np.array([np.inf]), np.array([0]))[0]
    assert RP.HEADROOM == float(Q.PZERO) / 2 and abs(RP.HEADROOM - 2.5e-4) < 1e-10
