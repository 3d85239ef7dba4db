"""rt_shade's precomputed terms: the per-triangle shading record (geometric normal | material id), the baked
material constants, the light centres and the wave-level queue locator must leave every queue slot and every deposit what the
oracle's per-hit evaluation gives -- through every path that writes a triangle, a material id, the material table or the lights,
and for every shape of segmented queue the locator can meet. Small scenes: a 512-triangle Cornell box at 64 x 36 texels, at
most three bounce rounds per case; the comparators are the ones of test_gpu_parity.test_shade_rounds_bit_exact_queues."""
import numpy as np
import pytest

from test_gpu_parity import _hits_equal, _rays_equal

pytestmark = pytest.mark.gpu

W, H = 64, 36


def _subdivide(tris, normals, mats, levels=2):
    """every triangle into four, `levels` times (vertex normals and material ids follow)"""
    for _ in range(levels):
        def mid(a, i, j):
            return (a[:, i] + a[:, j]) * np.float32(0.5)

        def split(a):
            m01, m12, m20 = mid(a, 0, 1), mid(a, 1, 2), mid(a, 2, 0)
            parts = [np.stack(p, 1) for p in ((a[:, 0], m01, m20), (m01, a[:, 1], m12), (m20, m12, a[:, 2]), (m01, m12, m20))]
            return np.ascontiguousarray(np.stack(parts, 1).reshape(-1, 3, 3).astype(np.float32))
        tris, normals, mats = split(tris), split(normals), np.repeat(mats, 4)
    return tris, normals, np.ascontiguousarray(mats, np.int32)


def _box_scene(scenes, open_top=False):
    sc = dict(scenes.cornell(open_top=open_top))
    sc["tris"], sc["normals"], sc["mats"] = _subdivide(sc["tris"], sc["normals"], sc["mats"])
    assert sc["tris"].shape[0] == 512
    return sc


class _Frame:
    """One hierarchy, one Pipeline and the oracle's copy of the frame; round() advances both and compares them."""

    def __init__(self, psm, ctx, oracle, scenes, scene, lights=None, time=17, build=True):
        self.psm, self.oracle, self.scenes = psm, oracle, scenes
        self.tris, self.normals, self.tri_mats = scene["tris"], scene["normals"], scene["mats"]
        self.th = psm.TriangleHierarchy(ctx)
        self.th.allocate(self.tris.shape[0])
        if build:
            self.th.loadTriangles(self.tris, self.normals, self.tri_mats)
            self.th.build()
            self.ob = oracle.build_scene(self.tris)
        self.rt = psm.Pipeline(ctx)
        self.rt.resizeBuffers(W, H)
        self.rt.resize(W, H)
        self.cam = scenes.camera_matrices(scene["eye"], scene["view"], W, H)
        self.lights = oracle.default_lights(1) if lights is None else lights
        self.set_materials(scene["materials"])
        self.rounds = 0
        self.new_frame(time)

    def new_frame(self, time):
        self.rt.camera_matrices(self.cam[0], self.cam[1], time=time)
        self.orays, _, self.osum, self.oflag = self.oracle.camera(self.cfg, self.cam[0], self.cam[1], time)

    def set_materials(self, materials, offset=0):
        ms = self.psm.MaterialSet()
        for m in materials:
            ms.addSubmat(m)
        ms.setLoadingOffset(offset)
        self._keep = getattr(self, "_keep", []) + [ms]     # (applyMaterials keys its cache on the set's identity)
        self.mats = self.scenes.materials_array(materials)
        self.cfg = self.oracle.make_cfg(W, H, lights=len(self.lights), material_count=len(self.mats), material_offset=offset)
        self.rt.applyMaterials(ms)

    def set_lights(self, lights):
        self.lights = lights
        self.cfg.light_count = len(lights)
        self.rt.setLights(lights)

    def round(self, t, force=False):
        o, n = self.oracle, self.orays.shape[0]
        assert self.rt.raycountCache == n
        assert self.rt.intersection(self.th, force=force) == 1
        oh, oc, _ = o.traverse(self.ob["nodes"], self.tris, self.ob["M"], self.orays["origin"], self.orays["direct"], 8)
        gh, gc = self.rt.download_hits(n)
        _hits_equal(gh, gc, oh, oc)
        self.shade(t, oh, oc, force)
        return oh, oc

    def shade(self, t, oh, oc, force=False):
        self.rt.shade(time=t, force=force)
        self.orays = self.oracle.shade(self.cfg, self.lights, self.mats, self.tri_mats, self.tris, self.normals, t, self.orays, oh, oc,
                                       self.osum, self.oflag)
        assert self.rt.raycountCache == self.orays.shape[0], self.rounds
        _rays_equal(self.rt.download_rays(), self.orays)          # the next queue, slot for slot
        s, _, _ = self.rt.download_texels()
        assert np.array_equal(s[:, 3], self.osum[:, 3])           # deposit counts
        np.testing.assert_allclose(s[:, :3], self.osum[:, :3], rtol=1e-5, atol=1e-6)
        self.rounds += 1

    def reload(self, tris, normals, tri_mats, refit, pieces=None):
        """the triangles again -- whole, or in `pieces` (index arrays, loaded one after the other: every piece but the first is a
        partial upload with first > 0) -- then a refit of the built tree or a rebuild"""
        self.th.clearTribuffer()
        for ix in (pieces or [np.arange(tris.shape[0])]):
            self.th.loadTriangles(tris[ix], normals[ix], tri_mats[ix])
        if refit:
            self.th.refit()
            self.ob = self.oracle.refit(self.ob, tris)
        else:
            self.th.markDirty()
            self.th.build()
            self.ob = self.oracle.build_scene(tris)
        self.tris, self.normals, self.tri_mats = tris, normals, tri_mats

    def close(self):
        self.rt.close()
        self.th.close()


# ---------------------------------------------------------------------------- geometry changes
def test_refit_that_flips_geometric_normals(psm, ctx, oracle, scenes):
    """Triangles reloaded for a refit with two corners exchanged (every third one): the geometric normal turns against the vertex
    normals, which stay -- sg = -1 for those hits. The shading record must follow the reload."""
    sc = _box_scene(scenes)
    f = _Frame(psm, ctx, oracle, scenes, sc)
    f.round(100)
    tris = sc["tris"].copy()
    flip = np.arange(0, tris.shape[0], 3)
    tris[flip] = tris[flip][:, [0, 2, 1]]
    rng = np.random.RandomState(2)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    tris = np.clip(tris + rng.normal(0, 0.01, tris.shape), lo, hi).astype(np.float32)   # (inside the build's bounds)
    f.reload(tris, sc["normals"], sc["mats"], refit=True)
    for rnd in range(2):
        f.round(101 + rnd)
    assert f.orays.shape[0] > 32
    f.close()


def test_partial_reload_refreshes_its_own_range_only(psm, ctx, oracle, scenes):
    """The second loadTriangles of a reload starts at first > 0: its triangles (moved, other materials) get new records, the
    first piece's (reloaded unchanged) keep theirs."""
    sc = _box_scene(scenes)
    f = _Frame(psm, ctx, oracle, scenes, sc)
    f.round(200)
    n = sc["tris"].shape[0]
    cut = 301                                                        # no multiple of a workgroup of the loader
    tris, mats = sc["tris"].copy(), sc["mats"].copy()
    tris[cut:] = tris[cut:][:, [0, 2, 1]]
    mats[cut:] = (mats[cut:] + 1) % 4
    f.reload(tris, sc["normals"], mats, refit=False, pieces=[np.arange(0, cut), np.arange(cut, n)])
    for rnd in range(2):
        f.round(201 + rnd)
    f.close()


@pytest.mark.parametrize("order", ["ids_first", "positions_first"])
def test_material_ids_before_and_after_the_positions(psm, ctx, oracle, scenes, order):
    """The material-id array and the positions change in two separate reloads, in either order: the record holds both."""
    sc = _box_scene(scenes)
    f = _Frame(psm, ctx, oracle, scenes, sc)
    f.round(300)
    moved = sc["tris"][:, [0, 2, 1]].copy()
    other = ((sc["mats"] + 2) % 4).astype(np.int32)
    if order == "ids_first":
        f.reload(sc["tris"], sc["normals"], other, refit=True)
        f.round(301)
        f.reload(moved, sc["normals"], other, refit=True)
    else:
        f.reload(moved, sc["normals"], sc["mats"], refit=True)
        f.round(301)
        f.reload(moved, sc["normals"], other, refit=True)
    f.round(302)
    f.close()


def _not_ordinary(materials):
    """a table psm_rt_set_materials does not call `ordinary` (a diffuse above 1): rt_shade then builds both lobes of every hit"""
    return [materials[0], dict(materials[1], diffuse=(1.5, 0.2, 0.1, 1.0))] + list(materials[2:])


def test_opposed_and_zero_vertex_normals(psm, ctx, oracle, scenes):
    """Vertex normals that oppose the face (sg = -1) and vertex normals of zero (nn = NaN, sg = 0; the oracle carries the NaN into
    the rays' directions as well). The queues are compared under a table that is not `ordinary`, where both lobes of a hit are
    built: a NaN normal gives the shadow ray a NaN weight, createRay keeps a NaN colour, and the one-lobe kernel of an ordinary
    table -- before this record came as after it -- does not build the shadow ray of the lobe the pick dropped (api.hip, the
    `ordinary` rule: it speaks of materials, not of normals)."""
    sc = _box_scene(scenes)
    normals = sc["normals"].copy()
    normals[0::5] *= np.float32(-1.0)
    normals[2::7] = 0.0
    sc["normals"] = normals
    sc["materials"] = _not_ordinary(sc["materials"])
    f = _Frame(psm, ctx, oracle, scenes, sc)
    for rnd in range(3):
        f.round(400 + rnd)
    assert np.isnan(f.orays["direct"]).any()
    f.close()


def test_opposed_vertex_normals_with_an_ordinary_table(psm, ctx, oracle, scenes):
    """sg = -1 through the kernel the benchmark runs (one lobe per hit)."""
    sc = _box_scene(scenes)
    normals = sc["normals"].copy()
    normals[0::5] *= np.float32(-1.0)
    sc["normals"] = normals
    f = _Frame(psm, ctx, oracle, scenes, sc)
    for rnd in range(3):
        f.round(450 + rnd)
    f.close()


# ---------------------------------------------------------------------------- materials
def test_materials_replaced_between_frames(psm, ctx, oracle, scenes):
    """A second table without reloading geometry: shorter (material id 3 is out of range now: an inactive hit, the ray goes on
    through the current-ray slot), with a diffuse above 1 and a black full-metal material (not `ordinary`: the BOTH kernels)."""
    sc = _box_scene(scenes)
    f = _Frame(psm, ctx, oracle, scenes, sc, time=21)
    for rnd in range(2):
        f.round(500 + rnd)
    m = sc["materials"]
    table = [dict(m[0], diffuse=(0.0, 0.0, 0.0, 1.0), specular=(0.0, 0.3, 1.0, 0.0)), dict(m[1], diffuse=(1.5, 0.2, 0.1, 1.0)), m[2]]
    f.set_materials(table)
    assert (sc["mats"] == 3).any()
    n = sc["mats"].shape[0]
    f.new_frame(22)
    through = 0
    for rnd in range(3):
        oh, oc = f.round(510 + rnd)
        through += int(((oc > 0) & (sc["mats"][np.clip(oh["tri"][:, 0], 0, n - 1)] == 3)).sum())
    assert through > 50                                               # rays did meet the out-of-range material
    # ... and an ordinary table again, with a loading offset that puts id 0 out of range on the low side
    f.set_materials([m[1], m[2], m[3]], offset=1)
    f.new_frame(23)
    for rnd in range(2):
        f.round(520 + rnd)
    f.close()


# ---------------------------------------------------------------------------- lights
@pytest.mark.parametrize("count,zero", [(1, None), (3, 1), (16, 5)], ids=["1", "3-zero1", "16-zero5"])
def test_lights_replaced_between_rounds(psm, ctx, oracle, scenes, count, zero):
    """setLights after the first round: the rounds that follow test their direct-light rays against the new centres and aim the
    new shadow rays at light 0's. A light vector of zero has a NaN centre, here as in the oracle."""
    sc = _box_scene(scenes, open_top=True)
    f = _Frame(psm, ctx, oracle, scenes, sc)
    f.round(600)
    L = oracle.default_lights(count)
    for i in range(count):
        L[i]["lightVector"] = (0.3 - 0.11 * i, 1.0 if i % 3 else -0.4, 0.1 + 0.07 * i, 30.0 + 25.0 * i)
        L[i]["lightColor"] = (40.0 + i, 10.0 + 2 * i, 5.0, 3.0 + i)
        L[i]["lightOffset"] = (0.2 * (i % 2), 0.0, -0.3, 0.0)
    L[0]["lightVector"] = (0.3, 1.0, 0.1, 400.0)
    L[0]["lightColor"][3] = 40.0
    if zero is not None:
        L[zero]["lightVector"] = (0.0, 0.0, 0.0, 10.0)
    f.set_lights(L)
    for rnd in range(2):
        f.round(601 + rnd)
    f.close()


# ---------------------------------------------------------------------------- two hierarchies in one queue
def test_two_untextured_hierarchies_in_one_queue(psm, ctx, oracle, scenes):
    """intersection() with two hierarchies before shade(): the MULTI instantiation without textures reads each hit's record
    through its object's pointer."""
    sc = _box_scene(scenes)
    n = sc["tris"].shape[0]
    parts = [np.arange(0, 200), np.arange(200, n)]
    f = _Frame(psm, ctx, oracle, scenes, sc, build=False)
    ths, obs = [], []
    for ix in parts:
        th = psm.TriangleHierarchy(ctx)
        th.allocate(ix.size)
        th.loadTriangles(sc["tris"][ix], sc["normals"][ix], sc["mats"][ix])
        th.build()
        ths.append(th)
        obs.append(oracle.build_scene(sc["tris"][ix]))
    for rnd in range(3):
        o = f.orays
        oh, oc, _ = oracle.traverse(obs[0]["nodes"], sc["tris"][parts[0]], obs[0]["M"], o["origin"], o["direct"], 8)
        oracle.traverse_chain(obs[1]["nodes"], sc["tris"][parts[1]], obs[1]["M"], o["origin"], o["direct"], oh, oc, int(parts[1][0]), 8)
        for th in ths:
            assert f.rt.intersection(th) == 1
        assert ((oh["tri"][:, 0] >= 200) & (oc > 0)).any() and ((oh["tri"][:, 0] < 200) & (oc > 0)).any()
        f.shade(700 + rnd, oh, oc)
    f.close()
    for th in ths:
        th.close()


# ---------------------------------------------------------------------------- wave-level locator
def test_queue_with_empty_segments(psm, ctx, oracle, scenes):
    """A camera that mostly sees sky: most shading workgroups of round 1 emit nothing, so the bases of the next queue repeat."""
    sc = _box_scene(scenes, open_top=True)
    sc["eye"], sc["view"] = np.asarray((3.5, 0.0, 3.5), np.float32), np.asarray((0.0, 1.6, 3.0), np.float32)
    f = _Frame(psm, ctx, oracle, scenes, sc)
    primary = f.orays
    slot_of_texel = np.full(W * H, -1, np.int64)
    slot_of_texel[primary["texel"]] = np.arange(primary.shape[0])
    f.round(800)
    blocks = np.unique(slot_of_texel[f.orays["texel"]] // 256)
    nb = (primary.shape[0] + 255) // 256
    assert 32 < f.orays.shape[0] and 0 < blocks.size < nb - blocks.size   # most workgroups emitted nothing ...
    assert blocks.min() > 0 and blocks.max() - blocks.min() + 1 > blocks.size and blocks.max() < nb - 1   # ... in front of, between and behind the ones that did
    for rnd in range(2):
        if f.orays.shape[0] < 1:
            break
        f.round(801 + rnd, force=True)
    f.close()


@pytest.mark.parametrize("count", [1, 63, 64, 65, 1023, 1025])
def test_ray_counts_around_wave_and_workgroup_edges(psm, ctx, oracle, scenes, count):
    """psm_rt_set_ray_count on a segmented queue: the first `count` rays of it, slot for slot."""
    sc = _box_scene(scenes)
    f = _Frame(psm, ctx, oracle, scenes, sc)
    f.round(900)
    assert f.orays.shape[0] > 1025
    f.rt.set_ray_count(count)
    f.orays = f.orays[:count].copy()
    f.round(901, force=True)
    f.close()


def test_ray_count_above_the_queue_total_is_clamped(psm, ctx, oracle, scenes):
    sc = _box_scene(scenes)
    f = _Frame(psm, ctx, oracle, scenes, sc)
    f.round(1000)
    n = f.orays.shape[0]
    assert 32 < n < 4 * W * H - 777
    f.rt.set_ray_count(n + 777)
    f.rt.raycountCache = n                     # what the device clamps it to
    f.round(1001, force=True)
    f.close()


def test_round_cut_at_the_ray_limit(psm, ctx, oracle, scenes):
    """A full queue in a closed box emits more rays than currentRayLimit holds: the next round reads the first `limit` rays of a
    queue whose segments hold more (count < bases[nb])."""
    sc = _box_scene(scenes)
    f = _Frame(psm, ctx, oracle, scenes, sc, time=1100)
    limit = 4 * W * H
    parts = [oracle.camera(f.cfg, f.cam[0], f.cam[1], 1100 + q) for q in range(4)]
    f.orays = np.concatenate([p[0] for p in parts])
    assert f.orays.shape[0] == limit == f.cfg.ray_limit
    f.orays["pkey"] = np.arange(limit)
    f.osum, f.oflag = parts[0][2], parts[0][3]
    f.rt.upload_rays(f.orays)
    cut = 0
    for rnd in range(3):
        f.round(1101 + rnd)
        cut += int(f.orays.shape[0] == limit)
    assert cut >= 1
    f.close()
