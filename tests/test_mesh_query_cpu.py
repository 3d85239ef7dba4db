"""CPU tests (no GPU) of the mesh queries (psm_bvh_mesh_overlaps_dev / psm_bvh_mesh_count_dev / psm_bvh_mesh_triangles_dev,
mesh.hip; TriangleHierarchy.meshOverlaps / meshCount / meshTriangles): the model (tests/mesh_query_model.py) --
its rows' order and prefixes, the refused poses, the self-query --, psm_mesh_dev.h itself on the host under the sanitizers
against the model record for record, the exports, the header text, the Python surface and the refusals that need no hierarchy,
what mesh.hip compiles to, and the header layer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_query_model as MQ
import tri_query_model as TQ
from point_query_model import _split
from util import ROOT, csrc_asm, kernel_asm, kernel_meta

F = np.float32
D = np.float64
U = np.uint32
KS = (1, 2, 3, 8, 16)


def lattice_soup(seed, count):
    """triangles with vertices on the 1/8 lattice of [-1, 1]^3 (tests/test_gpu_tri_query.py's)"""
    rng = np.random.RandomState(seed)
    a = rng.randint(-8, 9, (count, 1, 3))
    a[count // 2:] = rng.randint(0, 5, (count - count // 2, 1, 3))
    return (np.clip(a + rng.randint(-1, 2, (count, 3, 3)), -8, 8) / 8.0).astype(F)


def _leaves(tris):
    """the triangles a build keeps, as far as these tests' inputs go: all but those with three equal vertices"""
    t = np.asarray(tris).reshape(-1, 3, 3)
    return np.nonzero(~((t[:, 0] == t[:, 1]).all(axis=1) & (t[:, 0] == t[:, 2]).all(axis=1)))[0]


def _rotation(rng, reflect=False):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if (np.linalg.det(q) < 0) != reflect:
        q[:, 0] = -q[:, 0]
    return q


def _pose(r, t):
    return np.concatenate([np.asarray(r, D), np.asarray(t, D).reshape(3, 1)], axis=1)


SIGNED_PERMUTATIONS = [np.eye(3), np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]]), np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]]),
                       np.array([[-1, 0, 0], [0, 1, 0], [0, 0, 1]]), np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]]),
                       np.array([[0, 0, -1], [0, -1, 0], [-1, 0, 0]])]


# ---- the model ---------------------------------------------------------------------------------------------------------------------

def test_model_rows_are_ascending_prefixes_and_counts_agree():
    tris = lattice_soup(41, 300)
    other = np.concatenate([lattice_soup(51, 60), np.repeat(F([[[0.25, 0.25, 0.25]]]), 3, axis=1)])
    poses = [_pose(r, t) for r, t in zip(SIGNED_PERMUTATIONS, ([0, 0, 0], [0.125, 0, -0.25], [3, 3, 3], [0, 0.5, 0], [-0.375, 0, 0.125], [0.25, 0.25, 0]))]
    leaves, oleaves = _leaves(tris), _leaves(other)
    assert oleaves.size == 60 and other.shape[0] == 61
    flag, count, rows, rcount = MQ.query(tris, leaves, other, oleaves, poses, 16)
    assert flag.shape == (6,) and count.shape == (6, 61) and rows.shape == (6, 61, 16) and rcount.shape == (6, 61)
    assert flag.any() and not flag.all() and (count > 16).any()
    assert np.array_equal(flag, (count > 0).any(axis=1)) and np.array_equal(rcount, np.minimum(count, 16))
    assert (count[:, 60] == 0).all() and (rows[:, 60] == -1).all()                # the dropped triangle, at every pose
    filled = rows >= 0
    assert np.array_equal(filled, np.arange(16)[None, None] < rcount[:, :, None])
    assert (np.diff(rows, axis=2)[filled[:, :, 1:]] > 0).all() and np.isin(rows[filled], leaves).all()
    for k in KS:
        f, c, r, rc = MQ.query(tris, leaves, other, oleaves, poses, k)
        assert np.array_equal(f, flag) and np.array_equal(c, count) and np.array_equal(r, rows[:, :, :k])
        assert np.array_equal(rc, np.minimum(count, k))
    # one pose alone answers as its row of the batch; a 4 x 4 matrix is the 3 x 4 one
    m44 = np.concatenate([poses[4], [[0, 0, 0, 1]]])
    f, c, r, _ = MQ.query(tris, leaves, other, oleaves, m44, 16)
    assert f[0] == flag[4] and np.array_equal(c[0], count[4]) and np.array_equal(r[0], rows[4])
    # the contract's own statement: the answers of the triangle queries for the posed triangles
    q = MQ.posed(other, poses)
    _, c2, r2, _ = TQ.query(tris, leaves, q[:, oleaves].reshape(-1, 3, 3), 16)
    assert np.array_equal(c2.reshape(6, 60), count[:, oleaves]) and np.array_equal(r2.reshape(6, 60, 16), rows[:, oleaves])


def test_model_refuses_poses_that_are_not_finite_or_not_rigid():
    tris = lattice_soup(41, 20)
    good = _pose(np.eye(3), [0, 0, 0])
    for bad in (np.nan, np.inf):
        m = good.copy()
        m[1, 2] = bad
        with pytest.raises(ValueError):
            MQ.query(tris, _leaves(tris), tris, _leaves(tris), [good, m])
    with pytest.raises(ValueError):
        MQ.query(tris, _leaves(tris), tris, _leaves(tris), [good, _pose(np.eye(3) * 1.01, [0, 0, 0])])
    MQ.query(tris, _leaves(tris), tris, _leaves(tris), [good, _pose(np.eye(3) * (1 + 1e-6), [0, 0, 0])])
    f, c, r, rc = MQ.query(tris, _leaves(tris), tris, _leaves(tris), np.zeros((0, 3, 4)))
    assert f.shape == (0,) and c.shape == (0, 20) and r.shape == (0, 20, 16) and rc.shape == (0, 20)


def test_model_identity_self_query_counts_every_leaf():
    """at the identity the query is the stored triangle: a = v0 exactly, so A = 0 and no axis separates, whatever fl(v0 + e1) is"""
    rng = np.random.RandomState(3)
    tris = np.concatenate([lattice_soup(7, 100), (rng.uniform(-1, 1, (200, 1, 3)) + rng.uniform(-0.1, 0.1, (200, 3, 3))).astype(F),
                           (rng.uniform(-1e3, 1e3, (50, 1, 3)) + rng.uniform(-1e-3, 1e-3, (50, 3, 3))).astype(F)])
    leaves = _leaves(tris)
    q = MQ.posed(tris, np.eye(4))[0]
    v0, e1, e2 = _split(tris)
    assert np.array_equal(q[:, 0], v0) and np.array_equal(q[:, 1], v0 + e1) and np.array_equal(q[:, 2], v0 + e2)
    assert (q[:, 1] != tris[:, 1]).any()                                          # the stored triangle, not the loaded one
    _, count, rows, _ = MQ.query(tris, leaves, tris, leaves, np.eye(3, 4), 16)
    assert (count[0, leaves] >= 1).all()
    few = leaves[count[0, leaves] <= 16]
    assert few.size > 100 and (rows[0, few] == few[:, None]).any(axis=1).all()


# ---- psm_mesh_dev.h on the host ----------------------------------------------------------------------------------------------------

def _host_records():
    """(pose m[12], other's stored v0, e1, e2, the candidate's stored v0, e1, e2) float32 [n, 30]: lattice poses on lattice soups
    (exact), general rotations and reflections over six decades of size, each with candidates that touch the posed triangle (built
    on its float64 image: a shared vertex, a crossing) and with random ones, and some records with NaN and inf"""
    rng = np.random.RandomState(61)
    recs = []

    def add(m, src, cand):
        s, c = _split(src), _split(cand)
        recs.append(np.concatenate([np.broadcast_to(np.asarray(m, D).reshape(1, 12), (src.shape[0], 12)), *s, *c], axis=1))

    for r in SIGNED_PERMUTATIONS:                                                  # the lattice: every operation exact
        m = _pose(r, rng.randint(-4, 5, 3) / 8.0)
        src = lattice_soup(rng.randint(1 << 20), 150)
        img = (src.astype(D) @ m[:, :3].T + m[:, 3]).astype(F)
        add(m, src, img)                                                           # the image itself: coincident
        add(m, src, img[rng.permutation(150)])
        add(m, src, lattice_soup(rng.randint(1 << 20), 150))
        touching = img.copy()
        touching[:, 1:] = np.clip(img[:, :1] + rng.randint(-2, 3, (150, 2, 3)) / 8.0, -2, 2)   # shares v0, the rest elsewhere
        add(m, src, touching.astype(F))
    for mag in range(-3, 3):                                                       # general poses, six decades of size
        scale = 10.0 ** mag
        for reflect in (False, True):
            m = _pose(_rotation(rng, reflect), rng.normal(size=3) * scale * 10.0 ** rng.uniform(-1, 2))
            src = ((rng.uniform(-1, 1, (200, 1, 3)) + rng.uniform(-0.2, 0.2, (200, 3, 3))) * scale).astype(F)
            img = src.astype(D) @ m[:, :3].T + m[:, 3]
            add(m, src, img.astype(F))                                             # near-coincident
            cross = img.mean(axis=1, keepdims=True) + rng.normal(size=(200, 3, 3)) * scale * 0.2
            add(m, src, cross.astype(F))                                           # through the interior
            share = img.copy()
            share[:, 1:] = img[:, :1] + rng.normal(size=(200, 2, 3)) * scale * 0.2
            add(m, src, share.astype(F))                                           # touching at a vertex, as rounding decides
            add(m, src, ((rng.uniform(-1, 1, (200, 1, 3)) + rng.uniform(-0.5, 0.5, (200, 3, 3))) * scale + m[:, 3]).astype(F))
    rec = np.concatenate(recs).astype(F)
    rec[::97, 14] = np.nan                                                         # other's v0.z
    rec[1::97, 16] = np.inf                                                        # other's e1.y
    rec[2::97, 29] = -np.inf                                                       # the candidate's e2.z
    rec[3::97, 3] = np.float32(3e38)                                               # a translation next to overflow
    rec[3::97, 12] = np.float32(3e38)
    return rec


def test_posed_query_triangle_on_the_host_is_the_model(tmp_path):
    """mesh_query_tri and mesh_split of psm_mesh_dev.h and tri_tri of psm_tri_dev.h as a stand-alone host program with its own
    main, built with -ffp-contract=off and the address and undefined-behaviour sanitizers and run as a process of its own on the
    CPU: the query triangle of every record is the model's bit for bit, its flag is the model's, and mesh_split is the division"""
    hipcc = "/opt/rocm/bin/hipcc"
    exe, fin, fout, fposed = (str(tmp_path / x) for x in ("mesh_pose_host", "records.bin", "flags.bin", "posed.bin"))
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "prismarine-core_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "mesh_pose_host.cpp"), "-o", exe])
    rec = _host_records()
    assert rec.shape[1] == 30 and rec.shape[0] >= 8000
    rec.tofile(fin)
    done = subprocess.run([exe, fin, fout, fposed], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode(errors="replace")
    got = np.fromfile(fout, np.uint8).astype(bool)
    got_q = np.fromfile(fposed, F).reshape(-1, 3, 3)
    want_q = MQ.pose_records(rec[:, :12], rec[:, 12:15], rec[:, 15:18], rec[:, 18:21])
    assert got_q.shape == want_q.shape
    bad = np.nonzero((got_q.view(U) != want_q.view(U)).reshape(-1, 9).any(axis=1))[0]
    assert bad.size == 0, "%d query triangles differ, first %d: %s against %s" % (bad.size, bad[0], got_q[bad[0]], want_q[bad[0]])
    want = TQ.tri_tri(rec[:, 21:24], rec[:, 24:27], rec[:, 27:30], want_q[:, 0], want_q[:, 1], want_q[:, 2])
    bad = np.nonzero(got != want)[0] if got.shape == want.shape else np.zeros(1, int)
    assert got.shape == want.shape and bad.size == 0, "%d flags differ, first %d: %s" % (bad.size, bad[0], rec[bad[0]])
    assert 0.2 < want.mean() < 0.9 and (~np.isfinite(want_q).reshape(-1, 9).all(axis=1)).sum() > 100
    assert not want[~np.isfinite(want_q).reshape(-1, 9).all(axis=1)].any()        # a non-finite image meets nothing


# ---- the library, the headers, the kernels ---------------------------------------------------------------------------------------

MESH_ENTRIES = ("psm_bvh_mesh_overlaps_dev", "psm_bvh_mesh_count_dev", "psm_bvh_mesh_triangles_dev")
MESH_METHODS = ("meshOverlaps", "meshCount", "meshTriangles")


def test_library_exports_the_mesh_queries(psm):
    lib = psm.lib()
    header = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    for s in MESH_ENTRIES:
        assert hasattr(lib, s) and s in psm.EXPORTS and re.search(r"\b%s\(psm_bvh\* bvh, psm_bvh\* other, const float\* poses, size_t p," % s, header), s
    section = header[header.index("/* mesh queries against a built hierarchy"):header.index("int psm_bvh_mesh_overlaps_dev(")]
    for text in ("a = fwd_point(m, v0),  b = a + fwd_vec(m, e1),  c = a + fwd_vec(m, e2)", "BIT FOR BIT", "fl(v0 + e1)", "HOST memory",
                 "its build dropped", "non-finite", "other == bvh is allowed", "the caller discounts", "mesh query before build",
                 "different contexts", "named by its index", "p == 0 returns PSM_OK and touches nothing", "other without leaves",
                 "bvh without leaves", "not covered: a mesh against a world"):
        assert text in section, text
    for m in MESH_METHODS:
        assert callable(getattr(psm.TriangleHierarchy, m)), m
        for other in (psm.QueryScene, psm.InstancedScene, psm.InstanceWorld):                  # a single hierarchy's only
            assert not hasattr(other, m), (other, m)
    hpp = open(os.path.join(ROOT, "include", "Prismarine", "TriangleHierarchy.hpp")).read()
    inl = open(os.path.join(ROOT, "include", "Prismarine", "TriangleHierarchy.inl")).read()
    for m, s in zip(MESH_METHODS, MESH_ENTRIES):
        assert re.search(r"int %s\(TriangleHierarchy \* other, const glm::mat4 \* poses, size_t p," % m, hpp)
        assert "TriangleHierarchy::%s(" % m in inl and s + "(bvh," in inl
    makefile = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "Makefile")).read()
    assert " mesh.hip " in re.search(r"^SRC := (.*)$", makefile, re.M).group(1) and re.search(r"^mesh\.o: psm_mesh_dev\.h .*psm_tri_dev\.h", makefile, re.M)


def test_mesh_refusals_without_a_hierarchy(psm):
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    one = ctypes.c_size_t(1)
    for fn in (lib.psm_bvh_mesh_overlaps_dev, lib.psm_bvh_mesh_count_dev):        # no hierarchy: refused before anything is touched
        assert fn(None, None, p, one, p) == -1
        assert fn(None, None, None, ctypes.c_size_t(0), None) == -1               # ... before p == 0 is answered, too
    assert lib.psm_bvh_mesh_triangles_dev(None, None, p, one, ctypes.c_uint32(1), p, p) == -1
    assert lib.psm_bvh_mesh_triangles_dev(None, None, None, ctypes.c_size_t(0), ctypes.c_uint32(0), None, None) == -1
    assert not any(buf)

    class NoCall(psm.TriangleHierarchy):   # the Python layer refuses k and the poses before any call
        def __init__(self):
            self.ctx, self._h, self.triangleCount = None, None, 5

    th = NoCall()
    eye = np.eye(3, 4)
    for k in (0, 17, 1 << 20):
        with pytest.raises(psm.PsmError, match="k must be 1 .. 16"):
            th.meshTriangles(th, eye, k)
    with pytest.raises(ValueError):
        th.meshTriangles(th, eye, 2.5)
    scaled = eye.copy()
    scaled[:, :3] *= 1.01
    nan = eye.copy()
    nan[0, 3] = np.nan
    for bad in (scaled, nan, [eye, scaled], np.eye(3), np.zeros((2, 2, 3, 4))):
        for call in (lambda m: th.meshOverlaps(th, m), lambda m: th.meshCount(th, m), lambda m: th.meshTriangles(th, m, 4)):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(TypeError):
        th.meshCount(object(), eye)


# The VGPRs each kernel reaches with the Makefile's flags, as ceilings, what its launch bound allocates, and the LDS it declares
# (the 16-entry stack; the id list is dynamic, k x 256 B, and does not show here) -- DESIGN.md 4.21.
MESH_VGPRS = {"bvh_query_mesh_any": (72, 72), "bvh_query_mesh_count": (72, 72), "bvh_query_mesh_tris": (80, 80)}


def test_mesh_kernels_codegen():
    asm = csrc_asm("mesh.hip")
    assert asm.count(".amdhsa_kernel ") == 3
    for name, (ceiling, allocated) in MESH_VGPRS.items():
        blk, body = kernel_asm(asm, "_ZN3psm%d%sENS_8MeshArgsE" % (len(name), name))

        def meta(key):
            return kernel_meta(blk, key)
        assert meta("vgpr_count") <= ceiling <= allocated, (name, meta("vgpr_count"))
        assert meta("vgpr_spill_count") == 0 and meta("sgpr_spill_count") == 0, name
        assert meta("private_segment_fixed_size") == 0 and "scratch_" not in body, name
        assert "v_writelane_b32" not in body, name                            # no SGPR parked in a VGPR lane either
        assert meta("group_segment_fixed_size") == 16 * 64 * 4, name          # the stack; the list is the launch's k x 64 x 4 B
        assert not re.search(r"v_rcp_|v_rsq_|v_sqrt_|v_div_", body), name     # no division (the lane mapping's either), no square root
        assert "v_fma_f32" not in body and "v_fmac_f32" not in body, name     # nothing contracted: one rounding per operation
        assert ("ds_read_b32" in body and "ds_write_b32" in body) or name != "bvh_query_mesh_tris", name
    src = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "mesh.hip")).read()
    assert "asm(" not in src and "asm volatile" not in src                    # plain C++ throughout
    # the list kernel's dynamic LDS is the launch's: k x 64 lanes x 4 B, on that kernel alone; the id column strides by the wave
    assert re.search(r"bvh_query_mesh_tris<<<grid, QUERY_BLOCK, \(size_t\)k \* QUERY_BLOCK \* sizeof\(uint32_t\), c->stream>>>", src)
    assert len(re.findall(r"bvh_query_mesh_(?:any|count)<<<grid, QUERY_BLOCK, 0, c->stream>>>", src)) == 2
    assert "BoxIdList<QUERY_BLOCK>(mesh_id_column(), m.q.samples)" in src and "m.leaf_tri = o->d_leaftri" in src


def test_mesh_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "mesh_query_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "mesh_query_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)
