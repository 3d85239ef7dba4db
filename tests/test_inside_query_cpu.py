"""CPU tests (no GPU) of the hit-count, inside / outside and signed-distance queries (psm_bvh_count_hits_dev / psm_bvh_inside_dev /
psm_bvh_signed_distance_dev, query.hip): the numpy model the GPU tests hold the kernels to (tests/inside_query_model.py) against
geometry (closed meshes with an analytic inside) and against the ray queries' model, the direction table in its three places, the
library's new exports, the kernels' code generation and the header layer."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import inside_query_model as IQ
import point_query_model as PQ
import query_model as Q
from util import QUERY_VGPRS, check_query_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@functools.lru_cache(maxsize=None)
def _cases():
    return IQ.geometry_cases()


@pytest.mark.parametrize("case", range(5), ids=["icosphere", "torus", "cube_grid", "shell", "shell_flipped"])
def test_model_inside_equals_the_analytic_answer(case):
    """Points kept clear of the surface by more than the polyhedron's distance from the smooth shape: the votes of 3 and of 5
    rays equal the analytic inside on every point (a cap of zero disagreements). One ray alone is reported, not asserted: a
    ray within 1e-5 of a shared edge is counted by both triangles, which is what the vote is for."""
    name, tris, p, truth, clearance, gap = _cases()[case]
    assert gap < clearance, (name, gap, clearance)   # the truth of the smooth shape is the polyhedron's on these points
    assert truth.sum() > 1000 and (~truth).sum() > 1000
    par = IQ.parities(tris, np.arange(tris.shape[0]), p, 5)
    print("%s: %d triangles, %d points (%d inside); wrong by direction %s, by one ray %d" % (
        name, tris.shape[0], p.shape[0], truth.sum(), [int((par[k] != truth).sum()) for k in range(5)],
        int((IQ.vote(par, 1) != truth).sum())))
    for samples in (3, 5):
        bad = np.nonzero(IQ.vote(par, samples) != truth)[0]
        assert bad.size == 0, (name, samples, bad.size, p[bad[:4]])
    assert np.array_equal(IQ.inside(tris, np.arange(tris.shape[0]), p[:500], 3), IQ.vote(par[:, :500], 3))


def test_closed_meshes_are_watertight():
    """every edge of the generated meshes is shared by exactly two triangles, once in each direction where the winding is
    consistent (the meshes parity is promised for)"""
    for tris in (IQ.icosphere(3), IQ.torus(), IQ.cube(), IQ.icosphere(2, 0.5, flip=True)):
        _, idx = np.unique(tris.reshape(-1, 3).view([("", F)] * 3), return_inverse=True)
        f = idx.reshape(-1, 3)
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        directed, n = np.unique(e, axis=0, return_counts=True)
        assert (n == 1).all()
        assert np.array_equal(directed, np.unique(e[:, ::-1], axis=0))


def _rays(rng, tris, n):
    p = tris.reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    return rng.uniform(lo, hi, (n, 3)).astype(F), rng.normal(size=(n, 3)).astype(F)


def test_count_model_against_the_ray_query_model():
    rng = np.random.RandomState(5)
    tris = np.concatenate([IQ.icosphere(2), rng.uniform(-1, 1, (200, 3, 3)).astype(F)])
    cand = np.arange(tris.shape[0])[::-1].copy()
    o, d = _rays(rng, tris, 3000)
    tmin = rng.uniform(-1, 0.5, 3000).astype(F)
    tmax = (tmin + rng.uniform(0, 2, 3000)).astype(F)
    for lo, hi in ((F(0), F(np.inf)), (tmin, tmax), (F(-np.inf), F(np.inf))):
        hits, anyh = Q.query(tris, cand, o, d, lo, hi)
        n = IQ.count(tris, cand, o, d, lo, hi)
        assert n.dtype == np.uint32 and np.array_equal(n > 0, anyh)
        # a window shrunk to the closest hit's own t still holds it
        t = hits[:, 2]
        found = hits.view(np.int32)[:, 3] >= 0
        again = IQ.count(tris, cand, o[found], d[found], t[found], t[found])
        assert (again >= 1).all()
    assert n.max() >= 4   # an unbounded line through a soup: several crossings
    # windows that exclude everything: beyond the farthest point of the scene, before the origin with tmax < 0 away from it
    far = F(1e3)
    assert not IQ.count(tris, cand, o, d, far, F(np.inf)).any()
    assert not IQ.count(tris, cand, o, d, F(-np.inf), -far).any()
    assert not IQ.count(tris, cand, o, d, F(1), F(0.5)).any()      # tmin > tmax
    assert not IQ.count(tris, np.zeros(0, np.int64), o, d).any()   # no leaves
    # the candidates are the leaves: a triangle that is not one is not counted
    assert np.array_equal(IQ.count(tris, cand[:-1], o, d) + IQ.count(tris, cand[-1:], o, d), IQ.count(tris, cand, o, d))


def test_count_model_invalid_rays_count_nothing():
    tris = IQ.cube() - F(0.5)
    cand = np.arange(12)
    o = np.zeros((8, 3), F)
    d = np.tile(F([0.3, 0.5, 0.8]), (8, 1))
    d[1] = [np.nan, 0, 1]
    d[2] = [np.inf, 0, 0]
    d[3] = 0
    o[4] = [np.nan, 0, 0]
    o[5] = [-np.inf, 0, 0]
    d[6] = [1e-30, 0, 0]          # normalises to NaN (its square underflows)
    tmin = np.zeros(8, F)
    tmin[7] = np.nan
    n = IQ.count(tris, cand, o, d, tmin, F(np.inf))
    assert list(n) == [1, 0, 0, 0, 0, 0, 0, 0]
    assert list(IQ.count(tris, cand, o[:1], d[:1], F(-np.inf), F(np.inf))) == [2]
    pts = np.array([[0, 0, 0], [2, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]], F)
    for s in (1, 3, 5):
        assert list(IQ.inside(tris, cand, pts, s)) == [True, False, False, False]


def test_signed_distance_model_is_the_closest_point_with_a_sign():
    tris = IQ.icosphere(2)
    cand = np.arange(tris.shape[0])
    rng = np.random.RandomState(6)
    p = rng.uniform(-1.3, 1.3, (2000, 3)).astype(F)
    p[-1] = [np.nan, 0, 0]
    rad = np.linalg.norm(p[:-1].astype(np.float64), axis=1)
    for rmax in (F(np.inf), F(0.1)):
        plain, _ = PQ.query(tris, cand, p, rmax)
        sd = IQ.signed_distance(tris, cand, p, rmax, 3)
        assert np.array_equal(sd.view(np.uint32)[:, [0, 1, 3]], plain.view(np.uint32)[:, [0, 1, 3]])
        assert np.array_equal(np.abs(sd[:, 2]).view(np.uint32), plain[:, 2].view(np.uint32))
        found = plain.view(np.int32)[:, 3] >= 0
        assert found.any() and not found[-1] and (found[:-1].all() or not np.isinf(rmax))
        miss = sd[~found]
        assert np.isposinf(miss[:, 2]).all() and (miss.view(np.int32)[:, 3] == -1).all() and not miss[:, :2].any()
        clear = found[:-1] & (np.abs(rad - 1.0) > 0.03)
        assert np.array_equal(np.signbit(sd[:-1, 2])[clear], (rad < 1.0)[clear])
    assert (~found).sum() > 500   # the band left most of the box out


def _header_directions():
    src = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    body = src[src.index("#define PSM_INSIDE_DIRECTIONS"):]
    body = body[:body.index("/*")]
    vals = [float(x) for x in re.findall(r"(-?\d+\.\d+(?:[eE]-?\d+)?)f", body)]
    return np.array(vals, F).reshape(-1, 3)


def test_direction_table_in_its_three_places(psm):
    """the header's literals, the package's mirror and the model's restatement are the same floats; the rows are unit to float
    rounding, none near an axis, and are the normalised square roots the header names"""
    hdr = _header_directions()
    assert hdr.shape == (5, 3)
    assert np.array_equal(hdr.view(np.uint32), IQ.INSIDE_DIRECTIONS.view(np.uint32))
    assert psm.INSIDE_DIRECTIONS.dtype == F and np.array_equal(psm.INSIDE_DIRECTIONS.view(np.uint32), hdr.view(np.uint32))
    src = np.sqrt(np.array([[1, 2, 3], [5, 1, 2], [3, 7, 1], [2, 3, 11], [7, 1, 5]], np.float64)) * \
        np.array([[1, 1, 1], [-1, 1, 1], [1, -1, 1], [-1, -1, -1], [1, 1, -1]])
    src /= np.linalg.norm(src, axis=1, keepdims=True)
    assert np.abs(hdr - src).max() < 1e-7
    assert (np.abs(hdr) > 0.25).all()


def test_library_exports_the_inside_queries(psm):
    lib = psm.lib()
    for s in ("psm_bvh_count_hits_dev", "psm_bvh_inside_dev", "psm_bvh_signed_distance_dev"):
        assert hasattr(lib, s) and s in psm.EXPORTS
    for m in ("countHits", "inside", "signedDistance"):
        assert callable(getattr(psm.TriangleHierarchy, m))


def test_inside_queries_reject_null_without_device(psm):
    if psm.lib().psm_device_count() > 0:
        pytest.skip("a GPU is present")
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    one, none = ctypes.c_size_t(1), ctypes.c_size_t(0)
    assert lib.psm_bvh_count_hits_dev(None, p, one, p) == -1
    assert lib.psm_bvh_count_hits_dev(None, None, none, None) == -1
    for fn in (lib.psm_bvh_inside_dev, lib.psm_bvh_signed_distance_dev):
        assert fn(None, p, one, ctypes.c_uint32(3), p) == -1
        assert fn(None, None, none, ctypes.c_uint32(3), None) == -1


def test_inside_query_kernels_codegen():
    """the count, inside and sign kernels, and the four earlier kernels still at their ceilings"""
    check_query_kernels(k for k in QUERY_VGPRS if k.startswith("bvh_"))


def test_inside_query_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "inside_query_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "inside_query_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)
