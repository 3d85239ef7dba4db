"""CPU tests (no GPU) of the box queries (psm_bvh_box_overlaps_dev / psm_bvh_box_count_dev / psm_bvh_box_triangles_dev, box.hip;
TriangleHierarchy.boxOverlaps / boxCount / boxTriangles): the float32 model (tests/box_query_model.py) against the
same formulas in float64, closedness and degenerate triangles on the lattice, the rows' order and prefixes, the prune's margin in
float64, the exports and the refusals, what box.hip compiles to, the header layer, and the id list under the sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import box_query_model as BQ
from point_query_model import _split
from util import ROOT, csrc_asm, kernel_asm, kernel_meta

F = np.float32
D = np.float64
U = np.uint32


def _f64_reading(tris, lo, hi):
    """pair i = (triangle i, box i): the float32 answer, the float64 answer of the same formulas on the same stored (v0, e1, e2),
    and the float64 gap on the deciding axis in length units (the largest gap / axis length over the axes that have a length)"""
    v0, e1, e2 = _split(tris)
    got = BQ.box_tri(v0, e1, e2, lo, hi)
    with np.errstate(all="ignore"):
        sep, gap, length = BQ.axes(*(x.astype(D) for x in (v0, e1, e2, lo, hi)))
        decide = np.where(length > 0, gap / length, -np.inf).max(axis=0)
    return got, ~sep.any(axis=0), decide


def _soup(seed, n):
    rng = np.random.RandomState(seed)
    c = rng.uniform(-1, 1, (n, 1, 3))
    tris = c + rng.uniform(-0.3, 0.3, (n, 3, 3))
    bc = c[:, 0] + rng.uniform(-0.4, 0.4, (n, 3))
    half = rng.uniform(0, 0.3, (n, 3))
    return tris, bc - half, bc + half


def _lattice(seed, n):
    """vertices and box corners on the 1/8 lattice of [-1, 1]^3: every operation of box_tri is exact in float32"""
    rng = np.random.RandomState(seed)
    tris = rng.randint(-8, 9, (n, 3, 3)) / 8.0
    tris[: n // 2, 1:] = np.clip(tris[: n // 2, :1] * 8 + rng.randint(-2, 3, (n // 2, 2, 3)), -8, 8) / 8.0   # half of them small
    a, b = rng.randint(-8, 9, (n, 3)), rng.randint(-8, 9, (n, 3))
    return tris.astype(F), (np.minimum(a, b) / 8.0).astype(F), (np.maximum(a, b) / 8.0).astype(F)


def test_model_on_the_lattice_is_the_float64_answer():
    """all arithmetic exact: equal for every pair, none left out; a good part of the pairs touch exactly"""
    tris, lo, hi = _lattice(1, 200000)
    got, want, decide = _f64_reading(tris, lo, hi)
    assert np.array_equal(got, want)
    assert 0.2 < want.mean() < 0.8 and (decide == 0).sum() > 2000


@pytest.mark.parametrize("shift", [0.0, 1000.0], ids=["soup", "soup_moved_by_1000"])
def test_model_on_a_random_soup_is_the_float64_answer_outside_the_band(shift):
    """equal for every pair whose float64 gap on the deciding axis exceeds 1e-5 length units; at most 2 % of the pairs may lie
    inside that band (measured: 0.0025 % and 0.009 %, and no pair differs at all)"""
    tris, lo, hi = _soup(2, 200000)
    tris, lo, hi = ((x.astype(F) + F(shift)).astype(F) for x in (tris, lo, hi))
    got, want, decide = _f64_reading(tris, lo, hi)
    band = np.abs(decide) <= 1e-5
    print("pairs %d, differ %d, in the band %.4f %%, overlap %.1f %%" % (got.size, (got != want).sum(), 100 * band.mean(), 100 * want.mean()))
    assert band.mean() <= 0.02
    assert np.array_equal(got[~band], want[~band])
    assert 0.1 < want.mean() < 0.5


def _counts(tri, lo, hi):
    v0, e1, e2 = _split(np.asarray(tri, F).reshape(1, 3, 3))
    return bool(BQ.box_tri(v0, e1, e2, np.asarray(lo, F).reshape(1, 3), np.asarray(hi, F).reshape(1, 3))[0])


def test_model_is_closed_and_handles_degenerate_triangles():
    tri = [[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]]                       # in the plane z = 0
    assert _counts(tri, [0, 0, -0.25], [0.5, 0.5, 0]) and _counts(tri, [0, 0, 0], [0.5, 0.5, 0.25])          # a shared face: both cells
    assert _counts(tri, [-0.25, -0.25, 0], [0, 0.5, 0.25]) and _counts(tri, [0.5, -0.5, -0.5], [1, 0, 0])    # an edge, a corner
    assert _counts(tri, [0.25, 0.25, -0.5], [1, 1, 0.5])                                                     # the hypotenuse through a box edge
    assert not _counts(tri, [0.375, 0.25, -0.5], [1, 1, 0.5])                                                # ... and one lattice step past it
    assert not _counts(tri, [0, 0, 0.125], [0.5, 0.5, 0.25]) and not _counts(tri, [0.625, -0.5, -0.5], [1, 0, 0])
    for p in ([0, 0, 0], [0.5, 0, 0], [0.25, 0.25, 0], [0.25, 0, 0], [0.125, 0.125, 0]):                     # point boxes: vertex, edge, interior
        assert _counts(tri, p, p), p
    for p in ([0.125, 0.125, 0.125], [0.125, 0.125, -0.125], [0.375, 0.25, 0], [-0.125, 0, 0]):              # one step off the plane / the edge
        assert not _counts(tri, p, p), p
    # degenerate triangles on the lattice: the float64 answer of the same formulas, and what geometry says of a segment / a point
    rng = np.random.RandomState(3)
    n = 30000
    a, b = rng.randint(-8, 9, (n, 3)), rng.randint(-3, 4, (n, 3))
    t = rng.randint(-2, 3, (n, 1))
    two_equal = np.stack([a, a, a + b], axis=1)
    collinear = np.stack([a, a + b, a + t * b], axis=1)
    point = np.stack([a, a, a], axis=1)
    for tris in (two_equal, two_equal[:, [2, 0, 1]], two_equal[:, [0, 2, 1]], collinear, point):
        tris = (tris / 8.0).astype(F)
        c, d = rng.randint(-8, 9, (n, 3)), rng.randint(-8, 9, (n, 3))
        lo, hi = (np.minimum(c, d) / 8.0).astype(F), (np.maximum(c, d) / 8.0).astype(F)
        got, want, _ = _f64_reading(tris, lo, hi)
        assert np.array_equal(got, want) and got.any() and not got.all()
    pt = (point / 8.0).astype(F)
    got, _, _ = _f64_reading(pt, lo, hi)
    assert np.array_equal(got, ((pt[:, 0] >= lo) & (pt[:, 0] <= hi)).all(axis=1))      # a point triangle counts iff it is in the box


def test_model_rows_are_sorted_prefixes_and_counts_agree():
    rng = np.random.RandomState(4)
    c = rng.uniform(-1, 1, (300, 1, 3))
    tris = (c + rng.uniform(-0.2, 0.2, (300, 3, 3))).astype(F)
    cand = rng.permutation(300)[:280]
    centre = rng.uniform(-1, 1, (500, 3))
    half = rng.uniform(0, 0.6, (500, 3))
    lo, hi = (centre - half).astype(F), (centre + half).astype(F)
    lo[0, 0], hi[1, 1], lo[2], hi[3, 2] = np.nan, np.inf, -np.inf, 0.0
    lo[3, 2] = 0.5
    flag, count, big, nbig = BQ.query(tris, cand, lo, hi, 16)
    ok, ids = BQ.counts_matrix(tris, cand, lo, hi)
    assert np.array_equal(count, ok.sum(axis=1)) and np.array_equal(flag, count > 0) and (count[:4] == 0).all()
    assert (count > 16).any() and ((count > 0) & (count < 16)).any() and (count == 0).sum() > 4
    for k in (1, 2, 3, 8, 16):
        f, c_, rows, nrows = BQ.query(tris, cand, lo, hi, k)
        assert np.array_equal(rows, big[:, :k]) and np.array_equal(nrows, np.minimum(count, k)) and np.array_equal(c_, count)
        assert np.array_equal(rows >= 0, np.arange(k)[None] < nrows[:, None]) and np.array_equal(nrows > 0, f)
        assert np.isin(rows[rows >= 0], cand).all()
        assert ((rows[:, :-1] < rows[:, 1:]) | (rows[:, 1:] < 0)).all()
    for i in np.nonzero(count)[0][:50]:                                 # the k lowest ids that count, by a sort
        assert list(big[i, :nbig[i]]) == sorted(ids[ok[i]])[:16]


# ---- the prune's margin ---------------------------------------------------------------------------------------

def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def _fit_like(rng, tris, kind):
    """a fit transform as the build makes them, as float32: the vertices' image lies in [0, 1]^3. kind 0: the plain fit (diagonal,
    the bounds of each axis to [0, 1]); kind 1: a rotation; kind 2: rotate-and-scale with condition number up to 16 (ray_axis's
    range) -- for both the image is scaled uniformly into the unit cube, which keeps the condition number"""
    v = tris.reshape(-1, 3).astype(D)
    if kind == 0:
        A = np.eye(3)
    else:
        s = np.ones(3) if kind == 1 else np.array([1.0, rng.uniform(1, 16), 16.0])[rng.permutation(3)]
        A = _rotation(rng) @ np.diag(s) @ _rotation(rng)
    y = v @ A.T
    lo, ext = y.min(0), y.max(0) - y.min(0)
    if kind != 0:
        ext = np.full(3, ext.max())
    M = np.zeros((3, 4))
    M[:, :3] = A / ext[:, None]
    M[:, 3] = -lo / ext
    return M.astype(F)


def _prune_figures(M, tris, lo, hi):
    """For triangle / box arrays that broadcast against each other ([..., 3, 3] and [..., 3]): which pairs count (float32), whether
    the kernel's float32 prune keeps the triangle's exact image (a leaf box with no padding at all), and per normalised axis
    the observed distance of the exact images, the bound claimed for it, and the margin granted"""
    v0, e1, e2 = _split(tris)
    v0, e1, e2 = (x.reshape(tris.shape[:-2] + (3,)) for x in (v0, e1, e2))
    counts = BQ.box_tri(v0, e1, e2, lo, hi)
    Md = M.astype(D)
    V = np.stack([v0.astype(D), v0.astype(D) + e1.astype(D), v0.astype(D) + e2.astype(D)], axis=-2)   # the stored triangle
    img = V @ Md[:, :3].T + Md[:, 3]
    tmin, tmax = img.min(axis=-2), img.max(axis=-2)
    pa, pb = lo.astype(D)[..., None, :] * Md[:, :3], hi.astype(D)[..., None, :] * Md[:, :3]           # [..., axis, j]
    elo, ehi = np.minimum(pa, pb).sum(-1) + Md[:, 3], np.maximum(pa, pb).sum(-1) + Md[:, 3]
    S = np.maximum(np.abs(pa), np.abs(pb)).sum(-1) + np.abs(Md[:, 3])
    observed = np.maximum(0, np.maximum(tmin - ehi, elo - tmax))
    lam = np.sqrt((Md[:, :3] ** 2).sum(axis=1))
    size = np.abs(np.concatenate([e1, e2], axis=-1).astype(D)).max(axis=-1)
    bound = lam * 2.0 ** -20 * size[..., None]                       # |row| x 16 eps x the triangle's size (eps = 2^-24)
    granted = (2 + S) * 2.0 ** -16 - 4 * 2.0 ** -24 * S              # h less the rounding of the float32 image (4 operations)
    # the prune as box.hip's box_row computes it, in float32
    fa, fb = lo[..., None, :] * M[:, :3], hi[..., None, :] * M[:, :3]
    mn, mx, ab = np.minimum(fa, fb), np.maximum(fa, fb), np.maximum(np.abs(fa), np.abs(fb))
    ilo = ((mn[..., 0] + mn[..., 1]) + mn[..., 2]) + M[:, 3]
    ihi = ((mx[..., 0] + mx[..., 1]) + mx[..., 2]) + M[:, 3]
    h = (F(2) + (((ab[..., 0] + ab[..., 1]) + ab[..., 2]) + np.abs(M[:, 3]))) * F(2.0 ** -16)
    assert ilo.dtype == F and h.dtype == F
    kept = (~(tmax < (ilo - h).astype(D)) & ~(tmin > (ihi + h).astype(D))).all(axis=-1)
    return counts, kept, observed, np.broadcast_to(bound, observed.shape), np.broadcast_to(granted, observed.shape)


def _touching_boxes(rng, tris, scale, per):
    """`per` boxes for each triangle that touch it or miss it by a few ulps: a corner, an edge or a face of the box through a
    vertex, a point of an edge or an interior point, the box reaching away from the triangle, moved by -8 .. 8 ulps"""
    t = np.repeat(tris.astype(D), per, axis=0)
    n = t.shape[0]
    w = rng.uniform(0, 1, (n, 3))
    kind = rng.randint(0, 3, n)
    w[kind == 0] = np.eye(3)[rng.randint(0, 3, (kind == 0).sum())]
    w[kind == 1, rng.randint(0, 3, (kind == 1).sum())] = 0
    w /= w.sum(axis=1, keepdims=True)
    q = (t * w[:, :, None]).sum(axis=1)
    away = -np.sign(t.mean(axis=1) - q)
    away[away == 0] = 1
    ext = 10.0 ** rng.uniform(-3, 0.5, (n, 3)) * scale
    back = np.where(rng.uniform(size=(n, 3)) < 0.3, rng.uniform(0, 1, (n, 3)) * ext, 0)      # these axes straddle the point
    nudge = rng.randint(-8, 9, (n, 1)) * np.spacing(np.abs(q).astype(F)).astype(D)
    a, b = q + away * (nudge - back), q + away * (nudge + ext)
    return np.repeat(tris, per, axis=0), np.minimum(a, b).astype(F), np.maximum(a, b).astype(F)


def test_prune_margin_covers_every_triangle_that_counts():
    """DESIGN.md 4.15's chain, in float64, over plain, rotating and rotate-and-scale (condition number up to 16) fit transforms
    and six decades of magnitude: for every pair that counts in float32, on every normalised axis,
        the distance of the exact images <= |row| 16 eps size(triangle) <= h less the image's rounding,
    and box.hip's float32 interval keeps the triangle's exact image even with no leaf padding at all."""
    rng = np.random.RandomState(5)
    worst, total, conds = 0.0, 0, []
    for mag in range(-3, 4):
        scale = 10.0 ** mag
        for kind in (0, 1, 2):
            c = rng.uniform(-1, 1, (250, 1, 3))
            tris = ((c + rng.uniform(-0.2, 0.2, (250, 3, 3)) * rng.uniform(0.02, 1, (250, 1, 1))) * scale).astype(F)
            M = _fit_like(rng, tris, kind)
            conds.append(np.linalg.cond(M[:, :3].astype(D)))
            centre = rng.uniform(-1.1, 1.1, (250, 3)) * scale
            half = 10.0 ** rng.uniform(-3, 0, (250, 3)) * scale
            pairs = [(tris[None], (centre - half).astype(F)[:, None], (centre + half).astype(F)[:, None])]      # every box x every triangle
            pairs.append(_touching_boxes(rng, tris, scale, 12))                                                # and the close calls
            for t, lo, hi in pairs:
                counts, kept, observed, bound, granted = _prune_figures(M, t, lo, hi)
                assert counts.any() and kept[counts].all(), (mag, kind)
                assert (observed[counts] <= bound[counts]).all(), (mag, kind, (observed[counts] / bound[counts]).max())
                assert (bound <= granted).all(), (mag, kind, (bound / granted).max())
                worst = max(worst, (observed[counts] / bound[counts]).max())
                total += counts.sum()
    print("pairs that count: %d; the largest observed / bound: %.3g; condition numbers up to %.1f" % (total, worst, max(conds)))
    assert max(conds) > 12 and total > 20000


# ---- the library, the headers, the kernels ---------------------------------------------------------------------------------------

BOX_ENTRIES = ("psm_bvh_box_overlaps_dev", "psm_bvh_box_count_dev", "psm_bvh_box_triangles_dev")


def test_library_exports_the_box_queries(psm):
    lib = psm.lib()
    header = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    for s in BOX_ENTRIES:
        assert hasattr(lib, s) and s in psm.EXPORTS and re.search(r"\b%s\(" % s, header), s
    assert "#define PSM_QUERY_K_MAX %d" % psm.QUERY_K_MAX in header and psm.QUERY_K_MAX == 16 == BQ.K_MAX
    assert re.search(r"float lo\[3\], pad0;\s+float hi\[3\], pad1;\s+} psm_box_query;", header) and psm.BOX_QUERY_DT.itemsize == 32
    assert "box queries against a built hierarchy" in header
    for m in ("boxOverlaps", "boxCount", "boxTriangles"):
        assert callable(getattr(psm.TriangleHierarchy, m)), m
        assert not hasattr(psm.QueryScene, m) and not hasattr(psm.InstanceWorld, m), m     # a single hierarchy's only
    lists = psm.QueryTriLists(np.full((3, 4), -1, np.int32), np.zeros(3, U))
    assert lists.tri.shape == (3, 4) and len(lists) == 3
    hpp = open(os.path.join(ROOT, "include", "Prismarine", "TriangleHierarchy.hpp")).read()
    inl = open(os.path.join(ROOT, "include", "Prismarine", "TriangleHierarchy.inl")).read()
    for m, s in zip(("boxOverlaps", "boxCount", "boxTriangles"), BOX_ENTRIES):
        assert re.search(r"int %s\(const psm_box_query \*" % m, hpp) and "TriangleHierarchy::%s(" % m in inl and s + "(bvh," in inl


def test_box_refusals_without_a_hierarchy(psm):
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for fn in (lib.psm_bvh_box_overlaps_dev, lib.psm_bvh_box_count_dev):   # no hierarchy: refused before anything is touched
        assert fn(None, p, ctypes.c_size_t(1), p) == -1
        assert fn(None, None, ctypes.c_size_t(0), None) == -1
    assert lib.psm_bvh_box_triangles_dev(None, p, ctypes.c_size_t(1), ctypes.c_uint32(1), p, p) == -1
    assert lib.psm_bvh_box_triangles_dev(None, None, ctypes.c_size_t(0), ctypes.c_uint32(0), None, None) == -1
    assert not any(buf)

    class NoCall:   # the Python layer refuses k = 0 and k > 16 before any call: a hierarchy that cannot make one
        ctx = None
        _scene = False

        def _launch_np(self, *a):
            raise AssertionError("a launch was made")
        _box_query = psm.TriangleHierarchy._box_query
        boxTriangles = psm.TriangleHierarchy.boxTriangles
    lo = np.zeros((2, 3), F)
    for k in (0, 17, 1 << 20):
        with pytest.raises(psm.PsmError, match="k must be 1 .. 16"):
            NoCall().boxTriangles(lo, lo, k)
    with pytest.raises(ValueError):
        NoCall().boxTriangles(lo, lo, 2.5)
    with pytest.raises(AssertionError, match="a launch was made"):
        NoCall().boxTriangles(lo, lo, 16)


# The VGPRs each kernel reaches with the Makefile's flags, as ceilings, and the LDS it declares (the 16-entry stack; the id list is
# dynamic, k x 256 B, and does not show here). __launch_bounds__(64, 8): 64 VGPRs keep 8 waves per SIMD open.
BOX_VGPRS = {"bvh_query_box_any": 54, "bvh_query_box_count": 53, "bvh_query_box_tris": 62}


def test_box_kernels_codegen():
    asm = csrc_asm("box.hip")
    assert asm.count(".amdhsa_kernel ") == 3
    for name, ceiling in BOX_VGPRS.items():
        blk, body = kernel_asm(asm, "_ZN3psm%d%sENS_9QueryArgsE" % (len(name), name))

        def meta(key):
            return kernel_meta(blk, key)
        assert meta("vgpr_count") <= ceiling <= 64, (name, meta("vgpr_count"))
        assert meta("vgpr_spill_count") == 0 and meta("sgpr_spill_count") == 0, name
        assert meta("private_segment_fixed_size") == 0 and "scratch_" not in body, name
        assert "v_writelane_b32" not in body, name                            # no SGPR parked in a VGPR lane either
        assert meta("group_segment_fixed_size") == 16 * 64 * 4, name          # the stack; the list is the launch's k x 64 x 4 B
        assert "v_rcp_f32" not in body and "v_sqrt_f32" not in body and "v_div_" not in body, name   # no division, no square root
        assert "v_fma_f32" not in body and "v_fmac_f32" not in body, name     # nothing contracted: one rounding per operation
        assert ("ds_read_b32" in body and "ds_write_b32" in body) or name != "bvh_query_box_tris", name
    # the most LDS a launch asks for: stack + 16 slots
    assert 16 * 64 * 4 + BQ.K_MAX * 64 * 4 == 8192


def test_box_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "box_query_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "box_query_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)


def test_the_id_list_against_std_sort_under_the_sanitizers(tmp_path):
    """the kernel's own list (psm_box_list.h) as a stand-alone host program with its own main, built with the address and
    undefined-behaviour sanitizers and run as a process of its own on the CPU: k = 1 .. 16, ids with the top bit set, a list of
    exactly k slots"""
    exe = str(tmp_path / "box_list_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-I", os.path.join(ROOT, "prismarine-core_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "box_list_host.cpp"), "-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0 and b" 0 bad" in done.stdout, done.stdout.decode(errors="replace")
