"""CPU tests (no GPU) of the k-best queries (psm_bvh_first_hits_dev / psm_bvh_nearest_dev, kbest.hip; TriangleHierarchy.firstHits /
nearest): the brute-force model (tests/kbest_query_model.py) at k = 1 is the closest-hit / closest-point model bit
for bit, its rows are prefixes of one another and its counts are min(k, brute count); the library exports both entry points, the
two kernels compile within their ceilings, and the header layer compiles against the new methods. The largest k of every test is
the library's own limit (the kmax fixture)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import inside_query_model as IQ
import kbest_query_model as KQ
import point_query_model as PQ
import query_model as Q
from util import ROOT, csrc_asm, kernel_asm, kernel_meta

F = np.float32
U = np.uint32


@pytest.fixture(scope="module")
def kmax(psm):
    """PSM_QUERY_K_MAX as the package states it, once the library is known to hold both entry points"""
    lib = psm.lib()
    assert hasattr(lib, "psm_bvh_first_hits_dev") and hasattr(lib, "psm_bvh_nearest_dev")
    return psm.QUERY_K_MAX


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    if a.dtype == np.float32:
        a, b = a.view(U), b.view(U)
    bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, "%s: %d differ, first %d: %s against %s" % (what, bad.size, bad[0], a[bad[0]], b[bad[0]])


def ray_fixtures():
    """(tris, cand, o, d, tmin, tmax): the windows-and-ties fixture of test_query_cpu, the deep fixture, a random soup"""
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    tris = np.concatenate([tri, tri, tri + F([1, 0, 0])])
    o = np.zeros((6, 3), F)
    d = np.tile(F([1, 0, 0]), (6, 1))
    yield tris, [2, 1, 0], o, d, F([0, 1, 1.5, 0, 2, np.nan]), F([np.inf, 1, 3, 0.5, 1, np.inf])
    yield tris, [1, 2], o, d, 0.0, np.inf
    tris, o, d = Q.deep_fixture(rays=64)
    yield tris, np.arange(tris.shape[0]), o, d, 0.0, np.inf
    rng = np.random.RandomState(12)
    tris = rng.uniform(-1, 1, (300, 3, 3)).astype(F)
    o = rng.uniform(-2, 2, (200, 3)).astype(F)
    d = (rng.uniform(-0.5, 0.5, (200, 3)).astype(F) - o).astype(F)
    yield tris, rng.permutation(300)[:280], o, d, rng.uniform(-1, 1, 200).astype(F), rng.uniform(1, 4, 200).astype(F)


def point_fixtures():
    """(tris, cand, p, rmax): the rmax-ties-and-invalid fixture of test_point_query_cpu, its random triangles, a cube's centre"""
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], F)
    tris = np.concatenate([tri, tri, tri + F([0, 0, 2])])
    p = np.array([[0.25, 0.25, 1]] * 6 + [[np.nan, 0, 0], [np.inf, 0, 0]], F)
    yield tris, [2, 1, 0], p, np.array([np.inf, 1, np.nextafter(F(1), F(0)), 0, -1, np.nan, np.inf, np.inf], F)
    yield tris, [1, 2], p[:1], np.inf
    rng = np.random.RandomState(4)
    tris = rng.uniform(-1, 1, (64, 3, 3)).astype(F)
    yield tris, np.arange(64), rng.uniform(-1.5, 1.5, (500, 3)).astype(F), np.inf
    cube = IQ.cube()
    yield cube, np.arange(cube.shape[0]), np.concatenate([cube.reshape(-1, 3).mean(0)[None], cube.reshape(-1, 3)[:3]]).astype(F), np.inf


def test_model_at_k_1_is_the_closest_hit_and_closest_point_model(kmax):
    for tris, cand, o, d, lo, hi in ray_fixtures():
        rows, count = KQ.first_hits(tris, cand, o, d, 1, lo, hi)
        hits, anyh = Q.query(tris, cand, o, d, lo, hi)
        _same(rows[:, 0], hits, "first hits, k = 1")
        assert np.array_equal(count > 0, anyh)
        _same(KQ.first_hits(tris, cand, o, d, kmax, lo, hi)[0][:, 0], hits, "first hits, slot 0 of k = %d" % kmax)
    for tris, cand, p, rmax in point_fixtures():
        rows, count = KQ.nearest(tris, cand, p, 1, rmax)
        hits, within = PQ.query(tris, cand, p, rmax)
        _same(rows[:, 0], hits, "nearest, k = 1")
        assert np.array_equal(count > 0, within)
        _same(KQ.nearest(tris, cand, p, kmax, rmax)[0][:, 0], hits, "nearest, slot 0 of k = %d" % kmax)


def test_model_rows_are_prefixes_and_sorted(kmax):
    for tris, cand, o, d, lo, hi in ray_fixtures():
        big, nbig = KQ.first_hits(tris, cand, o, d, kmax, lo, hi)
        for k in (1, 2, 3, kmax - 1):
            rows, count = KQ.first_hits(tris, cand, o, d, k, lo, hi)
            _same(rows, big[:, :k], "first hits prefix k = %d" % k)
            assert np.array_equal(count, np.minimum(nbig, k))
        t, tri = big[:, :, 2], big.view(np.int32)[:, :, 3].astype(np.int64) & 0xffffffff
        live = np.arange(kmax)[None, 1:] < nbig[:, None]
        with np.errstate(invalid="ignore"):
            asc = (t[:, :-1] < t[:, 1:]) | ((t[:, :-1] == t[:, 1:]) & (tri[:, :-1] < tri[:, 1:]))
        assert (asc | ~live).all()
    for tris, cand, p, rmax in point_fixtures():
        big, nbig = KQ.nearest(tris, cand, p, kmax, rmax)
        for k in (1, 2, 3, kmax - 1):
            rows, count = KQ.nearest(tris, cand, p, k, rmax)
            _same(rows, big[:, :k], "nearest prefix k = %d" % k)
            assert np.array_equal(count, np.minimum(nbig, k))
        live = np.arange(kmax)[None, 1:] < nbig[:, None]
        assert ((big[:, :-1, 2] <= big[:, 1:, 2]) | ~live).all()   # (dist: two d2 may share a sqrtf, so <=)


def test_model_count_is_min_k_and_the_brute_count(kmax):
    for tris, cand, o, d, lo, hi in ray_fixtures():
        c = IQ.count(tris, cand, o, d, lo, hi)
        for k in (1, 3, kmax):
            rows, count = KQ.first_hits(tris, cand, o, d, k, lo, hi)
            assert np.array_equal(count, np.minimum(c, k))
            tri = rows.view(np.int32)[:, :, 3]
            assert np.array_equal(tri >= 0, np.arange(k)[None] < count[:, None])
            assert np.isin(tri[tri >= 0], np.asarray(cand)).all()
            dead = tri < 0
            assert np.isinf(rows[:, :, 2][dead]).all() and not rows[:, :, :2][dead].any()
    tris, cand, p, _ = list(point_fixtures())[2]
    v0, e1, e2 = PQ._split(tris)
    _, _, d2 = PQ.closest_on_tris(v0[None], e1[None], e2[None], p[:, None, :])
    for rmax in (F(0.3), F(0.6)):
        c = (np.sqrt(d2) <= rmax).sum(axis=1)
        for k in (1, 3, kmax):
            assert np.array_equal(KQ.nearest(tris, cand, p, k, rmax)[1], np.minimum(c, k))
    assert (c > kmax).any() and (c < 3).any()


def test_model_ties_are_listed_by_id(kmax):
    """the same triangle five times: bit-equal t and d2, the ids decide, and k = 3 cuts inside the group; -0 and +0 are one value"""
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    tris = np.concatenate([tri] * 5 + [tri + F([1, 0, 0])])
    o, d = np.zeros((1, 3), F), F([[1, 0, 0]])
    rows, count = KQ.first_hits(tris, [5, 3, 4, 1, 0, 2], o, d, kmax)
    assert count[0] == 6 and list(rows.view(np.int32)[0, :6, 3]) == [0, 1, 2, 3, 4, 5]
    rows, count = KQ.first_hits(tris, [5, 3, 4, 1, 0, 2], o, d, 3)
    assert count[0] == 3 and list(rows.view(np.int32)[0, :, 3]) == [0, 1, 2]
    rows, count = KQ.nearest(tris, [5, 3, 4, 1, 0], np.zeros((1, 3), F), 3)
    assert count[0] == 3 and list(rows.view(np.int32)[0, :, 3]) == [0, 1, 3]
    # a ray that starts on the plane of two coincident triangles of opposite winding: t = +0 and -0, the lower id first
    flip = tri[:, [0, 2, 1]]
    rows, count = KQ.first_hits(np.concatenate([flip, tri]), [0, 1], F([[1, 0, 0]]), d, 2, -1.0, 1.0)
    assert count[0] == 2 and list(rows.view(np.int32)[0, :, 3]) == [0, 1] and (rows[0, :, 2] == 0).all()


def test_library_exports_the_kbest_queries(psm, kmax):
    lib = psm.lib()
    header = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    for s in ("psm_bvh_first_hits_dev", "psm_bvh_nearest_dev"):
        assert hasattr(lib, s) and s in psm.EXPORTS and re.search(r"\b%s\(" % s, header), s
    assert "#define PSM_QUERY_K_MAX %d" % kmax in header and kmax == 16
    assert callable(psm.TriangleHierarchy.firstHits) and callable(psm.TriangleHierarchy.nearest)
    lists = psm.QueryHitLists(np.zeros((3, 4, 4), F), np.zeros(3, U))
    assert lists.t.shape == (3, 4) and lists.tri.dtype == np.int32 and len(lists) == 3
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for fn in (lib.psm_bvh_first_hits_dev, lib.psm_bvh_nearest_dev):   # no hierarchy: refused before anything is touched
        assert fn(None, p, ctypes.c_size_t(1), ctypes.c_uint32(1), p, p) == -1
        assert fn(None, None, ctypes.c_size_t(0), ctypes.c_uint32(0), None, None) == -1


# The VGPRs each kernel may reach with the Makefile's flags and the LDS it declares (the 16-entry stack; the list is dynamic, k x
# 512 B, and does not show here). __launch_bounds__(64, 7): DESIGN.md 4.12 says why not 8; 64 VGPRs keep 8 waves per SIMD open.
KBEST_VGPRS = {"bvh_query_first_hits": 60, "bvh_query_nearest": 62}


def test_kbest_kernels_codegen(kmax):
    asm = csrc_asm("kbest.hip")
    for name, ceiling in KBEST_VGPRS.items():
        blk, body = kernel_asm(asm, "_ZN3psm%d%sENS_9QueryArgsE" % (len(name), name))

        def meta(key):
            return kernel_meta(blk, key)
        assert meta("vgpr_count") <= ceiling <= 64, (name, meta("vgpr_count"))
        assert meta("vgpr_spill_count") == 0 and meta("sgpr_spill_count") == 0, name
        assert meta("private_segment_fixed_size") == 0 and "scratch_" not in body, name
        assert "v_writelane_b32" not in body, name                            # no SGPR parked in a VGPR lane either
        assert meta("group_segment_fixed_size") == 16 * 64 * 4, name          # the stack; the list is the launch's k x 64 x 8 B
        assert "ds_read_b64" in body and "ds_write_b64" in body, name         # the list's keys: one 8-byte access per slot
        if name == "bvh_query_first_hits":
            assert "v_fma_mix_f32" in body, name
    # the most LDS a launch asks for fits a workgroup's 64 KB many times over: stack + kmax slots
    assert 16 * 64 * 4 + kmax * 64 * 8 == 12288


def test_kbest_header_layer_compiles_and_links(tmp_path, kmax):
    exe = str(tmp_path / "kbest_query_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "kbest_query_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)
