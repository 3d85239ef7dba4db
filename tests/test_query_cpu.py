"""CPU tests (no GPU) of the ray queries (psm_bvh_intersect_dev / psm_bvh_occluded_dev, query.hip): the numpy model the GPU
tests hold the kernels to (tests/query_model.py) against the oracle's brute force, the deep fixture the pipeline's stack cannot
answer, the library's new exports, the kernels' code generation and the header layer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import query_model as Q
from util import bits, check_query_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _camera_rays(oracle, scenes, sc, w, h, time=7):
    cam = scenes.camera_matrices(sc["eye"], sc["view"], w, h)
    rays, *_ = oracle.camera(oracle.make_cfg(w, h), cam[0], cam[1], time)
    return rays["origin"].copy(), rays["direct"].copy()


def _odd_rays(rng, n, lo, hi):
    """random rays inside the box plus NaN, inf, zero, negative-zero and axis-aligned directions"""
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    k = n // 8
    d[:k] = 0.0
    d[:k, 0] = np.where(np.arange(k) % 2 == 0, 1.0, -1.0)               # axis-aligned
    d[k:2 * k] = np.float32(-0.0)
    d[k:2 * k, 1] = np.where(np.arange(k) % 2 == 0, 1.0, -1.0)          # axis-aligned with -0 components
    d[2 * k:2 * k + 4] = 0.0                                              # zero
    d[2 * k + 4, 0] = np.nan
    d[2 * k + 5, 2] = np.inf
    d[2 * k + 6] = [np.inf, 1.0, 0.0]
    o[2 * k + 7, 1] = np.nan
    d[2 * k + 8] = [1e-30, 0.0, 0.0]                                      # normalises to NaN (its square underflows)
    return o, d


def _assert_clamped_model_is_oracle(oracle, tris, o, d):
    found, model = Q.brute_force_clamped(tris, o, d)
    for i in range(o.shape[0]):
        f, best = oracle.brute_force(tris, o[i], d[i])
        assert f == bool(found[i]), i
        assert bits(np.float32(best["t"])) == bits(model["t"][i]), (i, best, model[i])
        assert int(best["tri"]) == int(model["tri"][i]), (i, best, model[i])
        assert bits(np.float32(best["u"])) == bits(model["u"][i]) and bits(np.float32(best["v"])) == bits(model["v"][i]), i


def test_clamped_model_equals_oracle_brute_force_cornell(oracle, scenes):
    sc = scenes.cornell()
    tris = sc["tris"].reshape(-1, 3, 3)
    o, d = _camera_rays(oracle, scenes, sc, 32, 24)
    _assert_clamped_model_is_oracle(oracle, tris, o, d)
    rng = np.random.RandomState(11)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    o, d = _odd_rays(rng, 512, lo, hi)
    _assert_clamped_model_is_oracle(oracle, tris, o, d)


def test_clamped_model_equals_oracle_brute_force_sponza_like(oracle, scenes):
    sc = scenes.sponza_like(30011)
    tris = sc["tris"].reshape(-1, 3, 3)
    o, d = _camera_rays(oracle, scenes, sc, 24, 16)
    _assert_clamped_model_is_oracle(oracle, tris, o, d)
    rng = np.random.RandomState(12)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    o, d = _odd_rays(rng, 96, lo, hi)
    _assert_clamped_model_is_oracle(oracle, tris, o, d)


def test_unclamped_model_is_clamped_model_where_det_is_large():
    """1 / det and 1 / (max(|det|, 1e-6) sign(det)) are the same float where |det| >= 1e-6: the two tests agree bit for bit there"""
    rng = np.random.RandomState(3)
    tris = rng.uniform(-1, 1, (200, 3, 3)).astype(np.float32)
    tris[:50] *= np.float32(1e-4)                                    # small triangles: |det| below 1e-6 for many rays
    o = rng.uniform(-2, 2, (300, 3)).astype(np.float32)
    d = Q.normalize3(rng.normal(size=(300, 3)).astype(np.float32))
    tc, uc, vc, okc = Q.tri_test(tris, o, d, clamp=True)
    tq, uq, vq, okq = Q.tri_test(tris, o, d, clamp=False)
    big = np.abs(Q.dot3(tris[None, :, 1] - tris[None, :, 0], Q.cross3(d[:, None], tris[None, :, 2] - tris[None, :, 0]))) >= np.float32(1e-6)
    assert big.sum() > 1000 and (~big).sum() > 1000
    assert np.array_equal(okc[big], okq[big])
    sel = big & okc
    for a, b in ((tc, tq), (uc, uq), (vc, vq)):
        assert np.array_equal(a[sel].view(np.int32), b[sel].view(np.int32))


def test_query_model_windows_and_ties():
    """the window is tmin <= t <= tmax as floats; bit-equal t goes to the lowest id; a miss is (0, 0, +inf, -1)"""
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], np.float32)
    tris = np.concatenate([tri, tri, tri + np.float32([1, 0, 0])])
    o = np.zeros((6, 3), np.float32)
    d = np.tile(np.float32([1, 0, 0]), (6, 1))
    tmin = np.float32([0, 1, 1.5, 0, 2, np.nan])
    tmax = np.float32([np.inf, 1, 3, 0.5, 1, np.inf])
    hits, anyh = Q.query(tris, [2, 1, 0], o, d, tmin, tmax)
    tri = hits.view(np.int32)[:, 3]
    assert list(tri) == [0, 0, 2, -1, -1, -1]
    assert list(anyh) == [True, True, True, False, False, False]
    assert hits[0, 2] == 1.0 and hits[2, 2] == 2.0 and np.isinf(hits[3, 2]) and hits[3, 0] == 0 and hits[3, 1] == 0
    hits, anyh = Q.query(tris, [1, 2], o, d)   # candidates are the leaves: triangle 0 is not one
    assert hits.view(np.int32)[0, 3] == 1


def test_deep_fixture_defeats_the_pipeline_stack(oracle):
    """The fixture the GPU test runs the queries on: deeper than 16 levels, the reference traversal drops subtrees on its rays,
    and its answer then differs from the exact closest hit on some of them."""
    tris, o, d = Q.deep_fixture()
    b = oracle.build_scene(tris)
    assert b["levels"] > 16
    hits, counts, ctr = oracle.traverse(b["nodes"], tris, b["M"], o, d)
    assert ctr.stack_drops > 0
    exact, anyh = Q.query(tris, b["leafs"]["pdata"][:, 3], o, d)
    assert anyh.sum() > o.shape[0] // 2
    head = np.where(counts > 0, hits[:, 0]["tri"], -1)
    assert (head != exact.view(np.int32)[:, 3]).sum() > 0


def test_library_exports_the_queries(psm):
    lib = psm.lib()
    for s in ("psm_bvh_intersect_dev", "psm_bvh_occluded_dev"):
        assert hasattr(lib, s) and s in psm.EXPORTS
    assert psm.QUERY_RAY_DT.itemsize == 32 and psm.HIT_DT.itemsize == 16


def test_queries_reject_null_without_device(psm):
    if psm.lib().psm_device_count() > 0:
        pytest.skip("a GPU is present")
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    for fn in (lib.psm_bvh_intersect_dev, lib.psm_bvh_occluded_dev):
        assert fn(None, ctypes.cast(buf, ctypes.c_void_p), ctypes.c_size_t(1), ctypes.cast(buf, ctypes.c_void_p)) == -1
        assert fn(None, None, ctypes.c_size_t(0), None) == -1


def test_query_kernels_codegen():
    check_query_kernels(["bvh_query_closest", "bvh_query_any"])


def test_query_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "query_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "query_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)
