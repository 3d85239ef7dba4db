"""The HIP kernels against the second readings of the GLSL (tests/independent_*.py) -- no oracle in the comparison.

Everywhere else the GPU suite holds the kernels to oracle/, bit for bit; the oracle is held to the second readings on the CPU
(tests/test_oracle_cpu.py). Here the two ends meet directly, in the branches where a line mis-read by both the oracle and the
kernels would show nowhere else: rt_shade on equal-distance chains with inactive hits, on textures and normal maps and under an
equirect sky; rt_camera in 360-degree mode; rt_traverse on a chain that arrives from an earlier hierarchy; the mesh loader. The
readings are fed the GPU's own downloaded rays and hits, so each stage is compared on its own. Sizes are the smallest that take
every branch (the readings are scalar Python).

Bounds: what a reading and the oracle are held to on the CPU, for the kernels compute what the oracle computes: discrete values
exactly; shading floats 2e-5 (relative to the largest magnitude, at least 1), per-texel radiance 1e-5 / 1e-6 (the atomics' sum
order, as test_shade_rounds_bit_exact_queues); camera and loader floats 2e-6 x max(1, largest coordinate); chains bit for bit.
"""
import numpy as np
import pytest

from test_gpu_parity import _load, _setup_frame
from test_oracle_cpu import (LOADER_CASES, chain_case, chain_kinds, compare_loaded, compare_shade_round, loader_case, merge_stats,
                             second_reading_scene)
from util import bits, canonical_nodes

pytestmark = pytest.mark.gpu

NODE_DT = np.dtype([("box", "<u4", 4), ("pdata", "<i4", 4)])
SKY = (0.5, 0.7, 1.0)


def _sun(psm):
    """the reference's one light (Pipeline.inl:93-98)"""
    L = np.zeros(1, psm.LIGHT_DT)
    L[0]["lightColor"] = (np.float32(255.0) / np.float32(255.0) * np.float32(150.0), np.float32(250.0) / np.float32(255.0) * np.float32(150.0),
                          np.float32(244.0) / np.float32(255.0) * np.float32(150.0), 40.0)
    L[0]["lightVector"] = (0.3, 1.0, 0.1, 400.0)
    return L


@pytest.mark.parametrize("name,w,h", [("decals", 32, 32), ("cornell_open+tex", 32, 32), ("cornell_open+sky", 32, 18)])
def test_rt_shade_against_the_second_reading(psm, ctx, scenes, name, w, h):
    """Two bounce rounds of rt_shade against independent_shade.shade_round fed the GPU's own rays and hit chains: the queue --
    count, order, bitfield, texel, path key -- and the deposit counts exactly, origin / direction / colour within 2e-5, per-texel
    sums within 1e-5 / 1e-6. decals: every branch of rayshading.comp:60-116 (inactive hits, composite, early stop) and both of
    getNormalMapping; +tex: every texture part; +sky: readEnv."""
    import independent_shade as ind
    scene, skybox = second_reading_scene(scenes, name)
    th, rt, ms, cam = _setup_frame(psm, ctx, scenes, scene, w, h)
    off = scene.get("material_offset", 0)
    ms.setLoadingOffset(off)
    lights = _sun(psm)
    rt.setLights(lights)
    rt.setSky(SKY)
    if skybox is not None:
        rt.setSkybox(skybox)
    mats = scenes.materials_array(scene["materials"])
    rt.camera_matrices(cam[0], cam[1], time=99)
    rt.applyMaterials(ms)
    compared = excluded = 0
    taken = {}
    for rnd in range(2):
        n = rt.raycountCache
        assert rt.getRayCount() == n > 0
        rays = rt.download_rays()
        assert rt.intersection(th) == 1
        gh, gc = rt.download_hits(n)
        before, _, _ = rt.download_texels()
        t = 1000 + rnd
        rt.shade(time=t)
        out = rt.download_rays()
        after, _, _ = rt.download_texels()
        stats = {}
        got, tex = ind.shade_round(scene["tris"], scene["normals"], scene["mats"], mats, off, lights, SKY, t, rays, gh, gc,
                                   texcoords=scene.get("texcoords"), textures=scene.get("textures"), skybox=skybox, stats=stats)
        k, ex, dev = compare_shade_round(ind, got, tex, stats, out, after, 2e-5, 1e-5, "%s round %d" % (name, rnd), base=before)
        print(name, "round", rnd, "rays", k, "excluded", ex, "largest deviations", dev)
        compared, excluded = compared + k, excluded + ex
        merge_stats(taken, stats)
    print(name, "branches", taken)
    assert compared > 250 and excluded <= 0.005 * compared
    if name == "decals":
        for branch in ("first_inactive_later_active", "none_active", "composite_partial", "early_stop", "inactive_skipped",
                       "height_map", "normal_map"):
            assert taken[branch] >= 20, (branch, taken)
    if skybox is not None:
        assert taken["sky_lookup"] >= 100, taken
        rt.setSkybox(None)
    rt.close()
    th.close()


def test_rt_camera_360_against_the_second_reading(psm, ctx, scenes):
    """rt_camera in 360-degree mode, 32 x 16 at three `time` values, against independent_camera_sampler.camera_rays(enable360=True):
    jittered texel coordinates and bitfields exactly, origins / directions within 2e-6 x max(1, largest coordinate)."""
    import independent_camera_sampler as ind
    scene = scenes.cornell(open_top=True)
    w, h = 32, 16
    th, rt, ms, cam = _setup_frame(psm, ctx, scenes, scene, w, h)
    rt.switchMode()
    for time in (0, 77, 123456):
        rt.camera_matrices(cam[0], cam[1], time=time)
        rays = rt.download_rays()
        _, coord, _ = rt.download_texels()
        o, d, c, bf = ind.camera_rays(cam[0], cam[1], w, h, time, enable360=True)
        assert rays.shape[0] == w * h and np.array_equal(bits(c), bits(coord))
        t = rays["texel"]
        assert np.array_equal(np.sort(t), np.arange(w * h)) and np.array_equal(bf[t], rays["bitfield"])
        scale = max(1.0, float(np.abs(o).max()))
        print("time", time, "largest deviation: origin", float(np.abs(o[t] - rays["origin"]).max()) / scale, "direction",
              float(np.abs(d[t] - rays["direct"]).max()))
        np.testing.assert_allclose(o[t], rays["origin"], rtol=0, atol=2e-6 * scale)
        np.testing.assert_allclose(d[t], rays["direct"], rtol=0, atol=2e-6)
    rt.switchMode()
    rt.close()
    th.close()


def _canonical(psm, th):
    """the built tree as the canonical node array the traversal reading walks, and the build's transform"""
    info = th.info()
    n = info.leaf_count
    link = th.download(psm.BVH_LINK, np.int32, 2 * (n - 1)).reshape(n - 1, 2)
    pb = th.download(psm.BVH_PAIR_BOX, np.uint32, 8 * (n - 1)).reshape(n - 1, 8)
    rg = th.download(psm.BVH_RANGE, np.int32, 2 * (n - 1)).reshape(n - 1, 2)
    return canonical_nodes(info.root, link, pb, rg, NODE_DT), np.array(info.transform, np.float32)


def test_rt_traverse_chain_against_the_second_reading(psm, ctx, scenes):
    """rt_traverse over two hierarchies, 512 of the CPU test's rays: the first hierarchy's chains against the reading's fresh
    traversal, then the second's against traverse(chain_in = the GPU's own first chains, tri_base = object 1's id bits) -- chain
    length and triangle ids exactly, t, u, v bit for bit."""
    import independent_traverse as ind
    a, b, origin, direct = chain_case(scenes)
    n = 512
    origin, direct = np.ascontiguousarray(origin[:n]), np.ascontiguousarray(direct[:n])
    ths = []
    for tris in (a, b):
        th = _load(psm, ctx, {"tris": tris, "normals": scenes.prepare_normals(tris), "mats": np.zeros(tris.shape[0], np.int32)})
        th.build()
        ths.append(th)
    rays = np.zeros(n, psm.RAY_DT)
    rays["origin"], rays["direct"], rays["color"] = origin, direct, 1.0
    rays["bitfield"] = 1 | (3 << 8)
    rays["texel"] = np.arange(n) % 100
    rays["pkey"] = np.arange(n)
    rt = psm.Pipeline(ctx)
    rt.resizeBuffers(32, 16)
    rt.upload_rays(rays)
    assert rt.intersection(ths[0]) == 1
    h0, c0 = rt.download_hits(n)
    assert rt.intersection(ths[1]) == 1
    h1, c1 = rt.download_hits(n)
    base = 1 << 27                                   # download_hits reports tri | object sequence << 27
    seen = {"grown": 0, "nearer": 0, "tail_kept": 0, "cap": 0}

    def same(chain, hits, count, i):
        assert len(chain) == count[i], i
        for k, (tri, tt, u, vv) in enumerate(chain):
            assert tri == hits["tri"][i, k], (i, k)
            assert bits(np.float32([tt, u, vv])).tolist() == bits(np.float32([hits["t"][i, k], hits["u"][i, k], hits["v"][i, k]])).tolist(), (i, k)
    (nodes_a, m_a), (nodes_b, m_b) = _canonical(psm, ths[0]), _canonical(psm, ths[1])
    for i in range(n):
        first, _, _ = ind.traverse(nodes_a, a, m_a, origin[i], direct[i])
        same(first, h0, c0, i)
        cin = [(int(h0["tri"][i, k]), h0["t"][i, k], h0["u"][i, k], h0["v"][i, k]) for k in range(c0[i])]
        chain, _, _ = ind.traverse(nodes_b, b, m_b, origin[i], direct[i], chain_in=cin, tri_base=base)
        same(chain, h1, c1, i)
        for k, v in chain_kinds(ind, cin, chain, base).items():
            seen[k] += v
    print("chained traversal:", seen)
    assert seen["grown"] >= 50 and seen["nearer"] >= 50 and seen["tail_kept"] >= 10 and seen["cap"] >= 5
    rt.close()
    for th in ths:
        th.close()


@pytest.mark.parametrize("kw", LOADER_CASES, ids=lambda kw: "-".join(sorted(kw)) or "plain")
def test_load_mesh_against_the_second_reading(psm, ctx, scenes, kw):
    """psm_bvh_load_mesh against independent_loader.load (vertex/loader.comp:32-152): triangle count and material ids exactly,
    positions / normals / texcoords within 2e-6 x max(1, largest coordinate)."""
    import independent_loader as il
    mesh = loader_case(scenes, kw)
    want = il.load(mesh)
    n = want[0].shape[0]
    th = psm.TriangleHierarchy(ctx)
    th.allocate(n)
    th.loadMesh(mesh)
    assert th.triangleCount == n
    got = [th.download(w, np.float32, k * n).reshape(n, k) for w, k in ((psm.BVH_POSITIONS, 9), (psm.BVH_NORMALS, 9))]
    got += [th.download(psm.BVH_MATERIALS, np.int32, n), th.download(psm.BVH_TEXCOORDS, np.float32, 6 * n).reshape(n, 6)]
    print(kw, "largest deviation / scale", compare_loaded(got, want, kw))
    th.close()
