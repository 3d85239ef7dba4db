"""CPU tests (no GPU) of the scene queries (psm_scene_*_dev, query.hip; QueryScene): the combination rules in numpy
(tests/scene_query_model.py) against the single-mesh models over the concatenated mesh, the tie cases, the library's new exports
and host-side refusals, the kernels' code generation and the header layer."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import inside_query_model as IQ
import point_query_model as PQ
import query_model as Q
import scene_query_model as SQ
from util import QUERY_VGPRS, check_query_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = np.uint32
# the package's mirror of PSM_SCENE_MAX_GEOMETRIES (tests/conftest.py has put the repository on the path): a package without the
# scene queries has no such name, and this module does not import
MAX_GEOMETRIES = importlib.import_module("prismarine-core_amd").SCENE_MAX_GEOMETRIES
SCENE_EXPORTS = ("psm_scene_intersect_dev", "psm_scene_occluded_dev", "psm_scene_count_hits_dev", "psm_scene_closest_point_dev",
                 "psm_scene_within_dev", "psm_scene_inside_dev", "psm_scene_signed_distance_dev")


def _soup(seed, n):
    rng = np.random.RandomState(seed)
    c = rng.uniform(-1, 1, (n, 1, 3))
    return (c + rng.uniform(-0.25, 0.25, (n, 3, 3))).astype(F)


def _geoms(parts):
    return [(t, np.arange(t.shape[0])) for t in parts]


def _rays(rng, n):
    return rng.uniform(-1.2, 1.2, (n, 3)).astype(F), rng.normal(size=(n, 3)).astype(F)


@pytest.mark.parametrize("sizes", [(100,), (1, 70), (50, 1, 7, 90, 3, 3, 20)], ids=["2", "3", "8"])
def test_scene_model_equals_the_single_mesh_model_over_the_concatenation(sizes):
    """a mesh cut into consecutive parts (unequal, one of a single triangle): every scene answer is the unsplit mesh's -- floats by
    their bits, ids by the part's offset, counts and votes exactly. (geom, tri) in lexicographic order is the concatenation's id
    order, so the tie rules agree too: the mesh holds duplicated triangles that land in different parts."""
    tris = np.concatenate([IQ.icosphere(1), _soup(3, 160)])
    tris[150:170] = tris[5:25]                 # duplicates across the parts: bit-equal t and d2 with different ids
    parts, offs = SQ.split(tris, sizes)
    assert len(parts) == len(sizes) + 1 and sum(p.shape[0] for p in parts) == tris.shape[0]
    geoms, all_ids = _geoms(parts), np.arange(tris.shape[0])
    rng = np.random.RandomState(11)
    o, d = _rays(rng, 1500)
    o[0], d[1], d[2] = [np.nan, 0, 0], 0, [np.inf, 0, 0]
    tmin = rng.uniform(-1, 0.5, 1500).astype(F)
    tmax = (tmin + rng.uniform(0, 2, 1500)).astype(F)
    tmin[3], tmax[4] = 2, np.nan
    for lo, hi in ((F(0), F(np.inf)), (tmin, tmax), (F(-np.inf), F(np.inf))):
        hits, geom, anyh = SQ.intersect(geoms, o, d, lo, hi)
        exp, exp_any = Q.query(tris, all_ids, o, d, lo, hi)
        assert np.array_equal(SQ.merged_ids(hits, geom, offs).view(U), exp.view(U))
        assert np.array_equal(anyh, exp_any) and np.array_equal(geom >= 0, anyh)
        assert np.array_equal(SQ.count(geoms, o, d, lo, hi), IQ.count(tris, all_ids, o, d, lo, hi))
    assert (geom[:3] == -1).all()
    p = rng.uniform(-1.3, 1.3, (1200, 3)).astype(F)
    p[0] = [0, np.inf, 0]
    r = rng.uniform(0, 0.4, 1200).astype(F)
    r[1:5] = [np.nan, -1, 0, np.inf]
    for rm in (F(np.inf), r):
        hits, geom, wi = SQ.closest_point(geoms, p, rm)
        exp, exp_wi = PQ.query(tris, all_ids, p, rm)
        assert np.array_equal(SQ.merged_ids(hits, geom, offs).view(U), exp.view(U))
        assert np.array_equal(wi, exp_wi)
        for s in (1, 3, 5):
            sd, sgeom = SQ.signed_distance(geoms, p, rm, s)
            assert np.array_equal(SQ.merged_ids(sd, sgeom, offs).view(U), IQ.signed_distance(tris, all_ids, p, rm, s).view(U))
            assert np.array_equal(sgeom, geom)
    assert np.array_equal(SQ.parities(geoms, p, 5), IQ.parities(tris, all_ids, p, 5))
    for s in (1, 3, 5):
        assert np.array_equal(SQ.inside(geoms, p, s), IQ.inside(tris, all_ids, p, s))


def test_a_duplicated_geometry_answers_with_the_lower_index():
    tris = _soup(5, 120)
    g = (tris, np.arange(120))
    rng = np.random.RandomState(2)
    o, d = _rays(rng, 800)
    hits, geom, _ = SQ.intersect([g, g], o, d)
    one, _ = Q.query(tris, g[1], o, d)
    assert np.array_equal(hits.view(U), one.view(U)) and (geom >= 0).sum() > 100
    assert np.array_equal(geom, np.where(one.view(np.int32)[:, 3] >= 0, 0, -1))
    ph, pgeom, _ = SQ.closest_point([g, g, g], o)
    assert np.array_equal(ph.view(U), PQ.query(tris, g[1], o)[0].view(U)) and (pgeom == 0).all()
    # counted once per entry; the parity of a doubled surface is even everywhere
    assert np.array_equal(SQ.count([g, g], o, d), 2 * IQ.count(tris, g[1], o, d))
    assert not SQ.inside([g, g], o, 3).any()


def test_coplanar_duplicates_across_geometries_lowest_geom_then_lowest_tri():
    """the same triangle at id 7 of geometry 0 and at ids 0 and 2 of geometry 1: a bit-equal t and d2. Geometry 0 wins although
    its id is the highest; with the geometries swapped, geometry 0 (the former 1) wins with its lowest id, 0."""
    t = np.array([[[-1, -1, 1], [1, -1, 1], [0, 1, 1]]], F)
    far = _soup(8, 7) + F([0, 0, 5])
    a = np.concatenate([far, t])                # the triangle at id 7
    b = np.concatenate([t, far[:1], t])         # ... at ids 0 and 2
    o = np.array([[0, 0, 0], [0.1, -0.2, 0]], F)
    d = np.array([[0, 0, 1], [0, 0, 1]], F)
    ga, gb = (a, np.arange(8)), (b, np.arange(3))
    for geoms, tri in (([ga, gb], 7), ([gb, ga], 0)):
        hits, geom, _ = SQ.intersect(geoms, o, d)
        assert (geom == 0).all() and (hits.view(np.int32)[:, 3] == tri).all() and (hits[:, 2] == 1).all()
        ph, pgeom, _ = SQ.closest_point(geoms, o)
        assert (pgeom == 0).all() and (ph.view(np.int32)[:, 3] == tri).all() and (ph[:, 2] == 1).all()
    # a leaf the build dropped is no candidate: without id 0, geometry `b` answers with id 2
    hits, geom, _ = SQ.intersect([(b, np.array([1, 2])), ga], o, d)
    assert (geom == 0).all() and (hits.view(np.int32)[:, 3] == 2).all()


def test_equal_d2_across_geometries_and_strictly_smaller_later():
    """mirror images about x = 0 and a point on that plane: the two d2 are bit-equal (a sign flip is exact), geometry 0 wins in
    either order; a strictly nearer triangle in a later geometry wins"""
    t = np.array([[[0.5, -1, -1], [0.5, 1, -1], [0.75, 0, 1]]], F)
    m = (t * F([-1, 1, 1])).astype(F)
    p = np.array([[0, 0.1, 0.2], [0, -0.3, 0.1]], F)
    gt, gm = (t, np.arange(1)), (m, np.arange(1))
    dt, dm = SQ.d2_of(t, p, PQ.query(t, gt[1], p)[0]), SQ.d2_of(m, p, PQ.query(m, gm[1], p)[0])
    assert np.array_equal(dt.view(U), dm.view(U))
    for geoms in ([gt, gm], [gm, gt]):
        _, geom, _ = SQ.closest_point(geoms, p)
        assert (geom == 0).all()
    near = (t * F([0.5, 1, 1])).astype(F)
    hits, geom, _ = SQ.closest_point([gt, gm, (near, np.arange(1))], p)
    assert (geom == 2).all() and (hits[:, 2] < np.sqrt(dt)).all()


def test_window_and_radius_edges_hold_over_the_whole_scene():
    a = np.array([[[-1, -1, 1], [1, -1, 1], [0, 1, 1]]], F)
    b = (a + F([0, 0, 1])).astype(F)            # z = 2
    geoms = [(b, np.arange(1)), (a, np.arange(1))]
    o, d = np.zeros((1, 3), F), np.array([[0, 0, 1]], F)
    for lo, hi, geom, n in ((0, np.inf, 1, 2), (1, 1, 1, 1), (2, 2, 0, 1), (1.5, 2, 0, 1), (0, 0.99, -1, 0), (np.nextafter(F(1), F(2)), 2, 0, 1),
                            (2.01, np.inf, -1, 0), (2, 1, -1, 0), (np.nan, 2, -1, 0)):
        hits, g, anyh = SQ.intersect(geoms, o, d, F(lo), F(hi))
        assert g[0] == geom and anyh[0] == (geom >= 0) and SQ.count(geoms, o, d, F(lo), F(hi))[0] == n, (lo, hi)
        assert hits[0, 2] == {1: 1, 0: 2, -1: np.inf}[geom]
    for rm, geom in ((np.inf, 1), (1, 1), (np.nextafter(F(1), F(0)), -1), (0, -1), (-1, -1), (np.nan, -1)):
        hits, g, wi = SQ.closest_point(geoms, o, F(rm))
        assert g[0] == geom and wi[0] == (geom >= 0), rm
        sd, sg = SQ.signed_distance(geoms, o, F(rm), 3)
        assert sg[0] == geom and np.array_equal(np.abs(sd).view(U), np.abs(hits).view(U))


def test_invalid_queries_miss_every_geometry():
    geoms = _geoms([IQ.cube() - F(0.5), IQ.icosphere(1)])
    o = np.zeros((8, 3), F)
    d = np.tile(F([0.3, 0.5, 0.8]), (8, 1))
    d[1], d[2], d[3], o[4], o[5], d[6] = [np.nan, 0, 1], [np.inf, 0, 0], 0, [np.nan, 0, 0], [-np.inf, 0, 0], [1e-30, 0, 0]
    tmin = np.zeros(8, F)
    tmin[7] = np.nan
    hits, geom, anyh = SQ.intersect(geoms, o, d, tmin)
    assert list(geom) == [0] + [-1] * 7 and list(anyh) == [True] + [False] * 7
    assert list(SQ.count(geoms, o, d, tmin)) == [2] + [0] * 7
    miss = hits[1:]
    assert np.isposinf(miss[:, 2]).all() and (miss.view(np.int32)[:, 3] == -1).all() and not miss[:, :2].any()
    pts = np.array([[0, 0, 0], [3, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]], F)
    assert list(SQ.inside(geoms, pts, 3)) == [False, False, False, False]    # inside both bodies: an even parity
    assert list(SQ.inside(geoms[:1], pts, 3)) == [True, False, False, False]
    _, pgeom, wi = SQ.closest_point(geoms, pts, F([np.inf, 0.1, np.inf, np.inf]))
    assert list(pgeom) == [0, -1, -1, -1] and list(wi) == [True, False, False, False]


@pytest.mark.parametrize("case", [0, 1, 3], ids=["icosphere", "torus", "shell"])
def test_model_inside_of_a_split_closed_surface_is_the_analytic_answer(case):
    """a closed surface cut by triangle index into three geometries: the parity summed over them gives the analytic inside on
    every seeded point for 3 and 5 rays (no exceptions, as the unsplit model), and no single part does"""
    name, tris, p, truth, _, _ = IQ.geometry_cases()[case]
    p, truth = p[:3000], truth[:3000]
    n = tris.shape[0]
    parts, _ = SQ.split(tris, (n // 3, n // 2 - n // 3))
    geoms = _geoms(parts)
    par = SQ.parities(geoms, p, 5)
    for s in (3, 5):
        assert np.array_equal(IQ.vote(par, s), truth), (name, s)
    for g in geoms:
        assert (IQ.inside(g[0], g[1], p, 3) != truth).any()


def test_library_exports_the_scene_queries(psm):
    lib = psm.lib()
    for s in SCENE_EXPORTS:
        assert hasattr(lib, s) and s in psm.EXPORTS
    for m in ("intersect", "occluded", "countHits", "closestPoint", "within", "inside", "signedDistance"):
        assert callable(getattr(psm.QueryScene, m))
    hdr = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    assert int(re.search(r"#define PSM_SCENE_MAX_GEOMETRIES (\d+)", hdr).group(1)) == psm.SCENE_MAX_GEOMETRIES == MAX_GEOMETRIES == 32
    assert psm.QueryHits(np.zeros((2, 4), F)).geom is None
    for n in (0, MAX_GEOMETRIES + 1):
        with pytest.raises(ValueError):
            psm.QueryScene(None, [None] * n)


def test_scene_queries_refuse_bad_lists_without_a_device(psm):
    """what is refused before any context or device is looked at: a NULL list, a count of 0 or 33, a list of NULL entries --
    whatever n and the data pointers are"""
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nulls = (ctypes.c_void_p * 33)()
    u32, three = ctypes.c_uint32, ctypes.c_uint32(3)
    for n in (ctypes.c_size_t(1), ctypes.c_size_t(0)):
        for lst, count in ((None, 1), (nulls, 0), (nulls, 33), (nulls, 1), (nulls, 2), (nulls, 32)):
            for d_in, d_out in ((p, p), (None, None)):
                assert lib.psm_scene_intersect_dev(lst, u32(count), d_in, n, d_out, d_out) == -1
                assert lib.psm_scene_closest_point_dev(lst, u32(count), d_in, n, d_out, d_out) == -1
                assert lib.psm_scene_signed_distance_dev(lst, u32(count), d_in, n, three, d_out, d_out) == -1
                assert lib.psm_scene_inside_dev(lst, u32(count), d_in, n, three, d_out) == -1
                for fn in (lib.psm_scene_occluded_dev, lib.psm_scene_within_dev, lib.psm_scene_count_hits_dev):
                    assert fn(lst, u32(count), d_in, n, d_out) == -1


def test_scene_query_kernels_codegen():
    """the seven scene kernels, and the seven single-hierarchy kernels still at their ceilings"""
    names = [k for k in QUERY_VGPRS if not k.startswith("inst_")]
    assert len(names) == 14
    check_query_kernels(names)


def test_scene_query_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "scene_query_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "scene_query_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)
