"""prismarine-core_amd -- MI355X-native path-tracing core (hot path of EngineWorld/prismarine-core).

Python host-side mirror of the reference's header-only API (Include/Prismarine/*.hpp) over the
C ABI of include/psm_hip.h.  The compute lives in libpsm_hip.so (hand-written gfx950 HIP kernels,
prismarine-core_amd/csrc); this package is plumbing: ctypes signatures and the call order of
psm::RadixSort / psm::TriangleHierarchy / psm::Pipeline.

There is no CPU fallback: importing works anywhere (so the library's exports can be checked), but
every compute entry point needs a gfx950 device and raises PsmError otherwise.

The directory name contains a hyphen; import it with
    importlib.import_module("prismarine-core_amd")
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PSM_HIP_LIB") or os.path.join(_HERE, "libpsm_hip.so")  # override: A/B builds of the same ABI

EXPORTS = [
    "psm_device_count", "psm_ctx_create", "psm_ctx_create_on_stream", "psm_ctx_destroy", "psm_ctx_sync", "psm_ctx_copy_bandwidth", "psm_ctx_stream", "psm_last_error",
    "psm_buf_alloc", "psm_buf_free", "psm_buf_upload", "psm_buf_download", "psm_buf_ptr",
    "psm_sort_u64_u32", "psm_sort_u64_u32_dev", "psm_sort_set_algorithm", "psm_sort_get_algorithm",
    "psm_bvh_create", "psm_bvh_destroy", "psm_bvh_clear", "psm_bvh_load_triangles", "psm_bvh_set_texcoords", "psm_bvh_load_mesh", "psm_bvh_build", "psm_bvh_set_build_graph", "psm_bvh_refit",
    "psm_bvh_get_info", "psm_bvh_stage_bounds", "psm_bvh_stage_morton", "psm_bvh_stage_sort",
    "psm_bvh_stage_emit", "psm_bvh_download", "psm_bvh_intersect_dev", "psm_bvh_occluded_dev",
    "psm_bvh_closest_point_dev", "psm_bvh_within_dev", "psm_bvh_count_hits_dev", "psm_bvh_inside_dev", "psm_bvh_signed_distance_dev",
    "psm_bvh_first_hits_dev", "psm_bvh_nearest_dev",
    "psm_bvh_box_overlaps_dev", "psm_bvh_box_count_dev", "psm_bvh_box_triangles_dev",
    "psm_bvh_sweep_sphere_dev", "psm_bvh_sweep_occluded_dev",
    "psm_bvh_tri_overlaps_dev", "psm_bvh_tri_count_dev", "psm_bvh_tri_triangles_dev",
    "psm_bvh_tri_closest_dev", "psm_bvh_tri_within_dev",
    "psm_bvh_mesh_overlaps_dev", "psm_bvh_mesh_count_dev", "psm_bvh_mesh_triangles_dev",
    "psm_bvh_mesh_closest_dev", "psm_bvh_mesh_within_dev", "psm_bvh_mesh_clearance_dev",
    "psm_scene_intersect_dev", "psm_scene_occluded_dev", "psm_scene_count_hits_dev", "psm_scene_closest_point_dev", "psm_scene_within_dev",
    "psm_scene_inside_dev", "psm_scene_signed_distance_dev",
    "psm_instances_intersect_dev", "psm_instances_occluded_dev", "psm_instances_count_hits_dev", "psm_instances_closest_point_dev",
    "psm_instances_within_dev", "psm_instances_inside_dev", "psm_instances_signed_distance_dev",
    "psm_world_create", "psm_world_destroy", "psm_world_set_instances", "psm_world_set_transforms", "psm_world_count",
    "psm_world_intersect_dev", "psm_world_occluded_dev", "psm_world_count_hits_dev", "psm_world_closest_point_dev", "psm_world_within_dev",
    "psm_world_inside_dev", "psm_world_signed_distance_dev", "psm_world_first_hits_dev", "psm_world_nearest_dev",
    "psm_world_box_overlaps_dev", "psm_world_box_count_dev", "psm_world_box_triangles_dev",
    "psm_world_sweep_sphere_dev", "psm_world_sweep_occluded_dev",
    "psm_world_tri_overlaps_dev", "psm_world_tri_count_dev", "psm_world_tri_triangles_dev",
    "psm_world_tri_closest_dev", "psm_world_tri_within_dev",
    "psm_world_mesh_overlaps_dev", "psm_world_mesh_count_dev", "psm_world_mesh_triangles_dev",
    "psm_world_mesh_closest_dev", "psm_world_mesh_within_dev", "psm_world_mesh_clearance_dev",
    "psm_grid_surface_dev", "psm_grid_counts_dev", "psm_grid_solid_dev", "psm_grid_brick_count",
    "psm_grid_distance_dev", "psm_grid_signed_distance_dev",
    "psm_grid_sparse_surface_bricks_dev", "psm_grid_sparse_distance_bricks_dev", "psm_grid_sparse_surface_dev",
    "psm_grid_sparse_distance_dev", "psm_grid_sparse_signed_distance_dev",
    "psm_grid_world_surface_dev", "psm_grid_world_counts_dev", "psm_grid_world_instances_dev", "psm_grid_world_solid_dev",
    "psm_grid_world_distance_dev", "psm_grid_world_signed_distance_dev",
    "psm_rt_create", "psm_rt_destroy", "psm_rt_resize_buffers", "psm_rt_resize", "psm_rt_set_tile", "psm_rt_set_tile_interleaved", "psm_rt_set_tile_weighted",
    "psm_rt_set_lights", "psm_rt_set_sky", "psm_rt_set_skybox", "psm_rt_set_texture", "psm_rt_set_materials", "psm_rt_camera", "psm_rt_set_camera_mode", "psm_rt_ray_count",
    "psm_rt_traverse", "psm_rt_set_traverse_mode", "psm_rt_set_traverse_phases", "psm_rt_set_traverse_adaptive", "psm_rt_set_traverse_solo", "psm_rt_reset_hits", "psm_rt_shade", "psm_rt_sample", "psm_rt_sample_from", "psm_lanes_render", "psm_lanes_run_sharded", "psm_rt_clear_sampler", "psm_rt_snap",
    "psm_rt_get_texels_dev", "psm_rt_set_texels_dev", "psm_rt_tile_texels", "psm_rt_pack_texels_dev",
    "psm_rt_unpack_texels_dev", "psm_rt_unpack_tiles_dev", "psm_rt_ray_count_dev", "psm_rt_set_ray_count", "psm_rt_download_rays", "psm_rt_download_hits",
    "psm_rt_upload_rays", "psm_rt_download_texels",
    "psm_stats_enable", "psm_stats_reset", "psm_stats_get", "psm_stats_reference", "psm_stats_traverse_intervals",
    "psm_dist_unique_id", "psm_dist_init", "psm_dist_prepare", "psm_dist_connect", "psm_dist_connect_transport", "psm_dist_connect_hoststaged",
    "psm_dist_transport_name", "psm_dist_agree", "psm_dist_destroy", "psm_dist_rank", "psm_dist_world", "psm_dist_comm_ranks", "psm_dist_gather_tiles",
    "psm_dist_allgather_i32", "psm_dist_barrier", "psm_dist_decide", "psm_dist_render_batch", "psm_dist_render_frames", "psm_dist_emulate_tile", "psm_dist_set_band_weights",
]

TRAVERSE_AUTO, TRAVERSE_WHOLE, TRAVERSE_PHASED, TRAVERSE_ADAPTIVE = range(4)
TRAVERSE_MODES = {"auto": TRAVERSE_AUTO, "whole": TRAVERSE_WHOLE, "phased": TRAVERSE_PHASED, "adaptive": TRAVERSE_ADAPTIVE}

(BVH_KEYS, BVH_INDICES, BVH_LEAF_BOX, BVH_LEAF_TRI, BVH_PAIR_BOX, BVH_LINK, BVH_RANGE,
 BVH_SORTED_TRI, BVH_POSITIONS, BVH_NORMALS, BVH_MATERIALS, BVH_TEXCOORDS, BVH_NODE32) = range(13)

RAY_DT = np.dtype([("origin", "<f4", 3), ("direct", "<f4", 3), ("color", "<f4", 3),
                   ("bitfield", "<i4"), ("texel", "<i4"), ("pkey", "<u4")])
HIT_DT = np.dtype([("u", "<f4"), ("v", "<f4"), ("t", "<f4"), ("tri", "<i4")])
QUERY_RAY_DT = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("direct", "<f4", 3), ("tmax", "<f4")])   # psm_query_ray
POINT_QUERY_DT = np.dtype([("p", "<f4", 3), ("rmax", "<f4")])   # psm_point_query
BOX_QUERY_DT = np.dtype([("lo", "<f4", 3), ("pad0", "<f4"), ("hi", "<f4", 3), ("pad1", "<f4")])   # psm_box_query
SWEEP_QUERY_DT = np.dtype([("origin", "<f4", 3), ("radius", "<f4"), ("direct", "<f4", 3), ("tmax", "<f4")])   # psm_sweep_query
TRI_QUERY_DT = np.dtype([("a", "<f4", 3), ("pad0", "<f4"), ("b", "<f4", 3), ("pad1", "<f4"), ("c", "<f4", 3), ("pad2", "<f4")])   # psm_tri_query
TRI_DIST_QUERY_DT = np.dtype([("a", "<f4", 3), ("rmax", "<f4"), ("b", "<f4", 3), ("pad0", "<f4"), ("c", "<f4", 3), ("pad1", "<f4")])   # psm_tri_dist_query
TRI_HIT_DT = np.dtype([("u", "<f4"), ("v", "<f4"), ("dist", "<f4"), ("tri", "<i4"), ("s", "<f4"), ("t", "<f4"), ("zero0", "<f4"), ("zero1", "<f4")])   # psm_tri_hit
MESH_HIT_DT = np.dtype([("u", "<f4"), ("v", "<f4"), ("dist", "<f4"), ("tri", "<i4"), ("s", "<f4"), ("t", "<f4"), ("other", "<i4"), ("zero", "<f4")])   # psm_mesh_hit
QUERY_K_MAX = 16   # psm_hip.h PSM_QUERY_K_MAX
SCENE_MAX_GEOMETRIES = 32   # psm_hip.h PSM_SCENE_MAX_GEOMETRIES
WORLD_MAX_INSTANCES = 65536   # psm_hip.h PSM_WORLD_MAX_INSTANCES
INSTANCE_DT = np.dtype([("bvh", "<u8"), ("world_from_object", "<f4", 12)])   # psm_instance
# PSM_INSIDE_DIRECTIONS (include/psm_hip.h): ray k of TriangleHierarchy.inside / .signedDistance goes along row k
INSIDE_DIRECTIONS = np.array([[0.4082483, 0.57735026, 0.70710677], [-0.7905694, 0.35355338, 0.5],
                              [0.52223295, -0.797724, 0.30151135], [-0.35355338, -0.4330127, -0.8291562],
                              [0.7337994, 0.2773501, -0.6201737]], np.float32)
LIGHT_DT = np.dtype([("lightVector", "<f4", 4), ("lightColor", "<f4", 4),
                     ("lightOffset", "<f4", 4), ("lightAmbient", "<f4", 4)])


class PsmError(RuntimeError):
    pass


class BvhInfo(C.Structure):
    _fields_ = [("triangle_count", C.c_uint32), ("leaf_count", C.c_uint32), ("root", C.c_int32),
                ("transform", C.c_float * 16), ("bounds_min", C.c_float * 4), ("bounds_max", C.c_float * 4)]


class Grid(C.Structure):
    """psm_grid: origin, cell and dims of a voxel grid (host memory, read during the call)"""
    _fields_ = [("origin", C.c_float * 3), ("cell", C.c_float * 3), ("dims", C.c_uint32 * 3)]


class Instance(C.Structure):
    """psm_instance: a built hierarchy and its pose, world_from_object a row-major 3 x 4 [R | T]"""
    _fields_ = [("bvh", C.c_void_p), ("world_from_object", C.c_float * 12)]


class Accessor(C.Structure):
    _fields_ = [("offset4", C.c_int32), ("components", C.c_int32), ("buffer_view", C.c_int32)]


class BufferView(C.Structure):
    _fields_ = [("offset4", C.c_int32), ("stride4", C.c_int32)]


class MeshDesc(C.Structure):
    _fields_ = [("d_vertices", C.c_void_p), ("vertex_floats", C.c_size_t), ("d_indices", C.c_void_p),
                ("index_words", C.c_size_t), ("accessors", C.c_void_p), ("accessor_count", C.c_uint32),
                ("views", C.c_void_p), ("view_count", C.c_uint32), ("vertex_accessor", C.c_int32),
                ("normal_accessor", C.c_int32), ("texcoord_accessor", C.c_int32), ("modifier_accessor", C.c_int32),
                ("transform", C.c_float * 16), ("transform_inv", C.c_float * 16), ("material_id", C.c_int32),
                ("is_indexed", C.c_int32), ("index16", C.c_int32), ("node_count", C.c_int32),
                ("primitive_type", C.c_int32), ("loading_offset", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("rays_traced", C.c_uint64), ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64),
                ("stack_drops", C.c_uint64), ("iter_caps", C.c_uint64), ("baked_drops", C.c_uint64),
                ("chain_pool_drops", C.c_uint64), ("ray_limit_drops", C.c_uint64),
                ("traverse_launches", C.c_uint32), ("traverse_ms", C.c_float), ("build_ms", C.c_float),
                ("sort_ms", C.c_float), ("shade_ms", C.c_float), ("camera_ms", C.c_float),
                ("sample_ms", C.c_float), ("rounds", C.c_uint32), ("bounds_ms", C.c_float), ("morton_ms", C.c_float),
                ("emit_ms", C.c_float), ("wave_clock_ticks", C.c_uint64), ("wave_real_ticks", C.c_uint64),
                ("wave_steps", C.c_uint64), ("waves", C.c_uint64), ("handover_launches", C.c_uint32), ("handover_ms", C.c_float)]


_lib = None


def lib():
    """Load libpsm_hip.so (built by __graft_entry__.build()). Fails loudly when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PsmError("libpsm_hip.so is missing at %s -- run `make -C prismarine-core_amd/csrc` "
                           "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.psm_last_error.restype = C.c_char_p
        _lib.psm_ctx_stream.restype = C.c_void_p
        _lib.psm_world_create.restype = C.c_void_p
        _lib.psm_world_count.restype = C.c_uint32
        _lib.psm_grid_brick_count.restype = C.c_uint64
        for name in EXPORTS:
            getattr(_lib, name)  # AttributeError if an export is missing
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """One GPU, one in-order stream (the reference's single GL context, Viewer.cpp:371)."""

    def __init__(self, device=0, stream=None):
        """stream: an existing hipStream_t (int), e.g. torch.cuda.current_stream().cuda_stream, so kernels
        and RCCL collectives are ordered on one stream without host synchronisation."""
        self._h = C.c_void_p()
        if stream is None:
            rc = lib().psm_ctx_create(C.c_int(device), C.byref(self._h))
        else:
            rc = lib().psm_ctx_create_on_stream(C.c_int(device), C.c_void_p(stream), C.byref(self._h))
        if rc != 0:
            raise PsmError("psm_ctx_create(device=%d) failed with %d: a gfx950 (MI355X) device is required; "
                           "there is no CPU fallback" % (device, rc))
        self.device = device

    def check(self, rc, what=""):
        if rc != 0:
            msg = lib().psm_last_error(self._h)
            raise PsmError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))

    def sync(self):
        self.check(lib().psm_ctx_sync(self._h), "psm_ctx_sync")

    @property
    def stream(self):
        return lib().psm_ctx_stream(self._h)

    def copy_bandwidth(self, nbytes=1 << 30, reps=5):
        """Measured device-to-device copy rate in GB/s of traffic (read + write): the box's achievable HBM ceiling."""
        v = C.c_double()
        self.check(lib().psm_ctx_copy_bandwidth(self._h, C.c_size_t(nbytes), C.c_int(reps), C.byref(v)), "psm_ctx_copy_bandwidth")
        return v.value

    def stats_enable(self, timing=True, counting=False):
        """timing: False / True (HIP events around every launch) / 2 (traversal launches only: light, for frames in flight)"""
        self.check(lib().psm_stats_enable(self._h, C.c_int(int(timing)), C.c_int(int(counting))), "psm_stats_enable")

    def stats_reference(self, origin=None):
        """time origin of traverse_intervals(): recorded now on this context's stream, or shared with `origin`'s"""
        self.check(lib().psm_stats_reference(self._h, (origin or self)._h), "psm_stats_reference")

    def traverse_intervals(self):
        """(start, end) in ms after the reference of every traversal launch timed since the last reset"""
        n = C.c_uint32()
        self.check(lib().psm_stats_traverse_intervals(self._h, None, C.c_uint32(0), C.byref(n)), "psm_stats_traverse_intervals")
        buf = (C.c_float * (2 * max(n.value, 1)))()
        self.check(lib().psm_stats_traverse_intervals(self._h, buf, C.c_uint32(n.value), C.byref(n)), "psm_stats_traverse_intervals")
        return [(buf[2 * i], buf[2 * i + 1]) for i in range(n.value)]

    def stats_reset(self):
        self.check(lib().psm_stats_reset(self._h), "psm_stats_reset")

    def stats(self):
        s = Stats()
        self.check(lib().psm_stats_get(self._h, C.byref(s)), "psm_stats_get")
        return s

    def close(self):
        if self._h:
            lib().psm_ctx_destroy(self._h)
            self._h = C.c_void_p()

    # buffers (the GLuint names the header layer passes around, Utils.hpp:140-150)
    def buf_alloc(self, nbytes):
        h = C.c_uint32()
        self.check(lib().psm_buf_alloc(self._h, C.c_size_t(nbytes), C.byref(h)), "psm_buf_alloc")
        return h.value

    def buf_free(self, h):
        self.check(lib().psm_buf_free(self._h, C.c_uint32(h)), "psm_buf_free")

    def buf_ptr(self, h):
        p, n = C.c_void_p(), C.c_size_t()
        self.check(lib().psm_buf_ptr(self._h, C.c_uint32(h), C.byref(p), C.byref(n)), "psm_buf_ptr")
        return p.value, n.value

    def buf_upload(self, h, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        self.check(lib().psm_buf_upload(self._h, C.c_uint32(h), C.c_size_t(offset), _p(arr), C.c_size_t(arr.nbytes)),
                   "psm_buf_upload")

    def buf_download(self, h, dtype, count, offset=0):
        out = np.zeros(count, dtype)
        self.check(lib().psm_buf_download(self._h, C.c_uint32(h), C.c_size_t(offset), _p(out), C.c_size_t(out.nbytes)),
                   "psm_buf_download")
        return out


class RadixSort:
    """psm::RadixSort (Include/Prismarine/Radix.hpp:27-74)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def setAlgorithm(self, algorithm):
        """2 (default): hybrid -- two global passes over the top sixteen key bits, the rest in LDS; 0: histogram / scan /
        scatter kernels for all eight passes; 1: one-sweep histograms + look-back scatter."""
        self.ctx.check(lib().psm_sort_set_algorithm(self.ctx._h, C.c_int(algorithm)), "psm_sort_set_algorithm")

    def getAlgorithm(self):
        """(asked, effective): they differ once a hybrid sort has overflowed a chunk and the context fell back to 0."""
        a, e = C.c_int(0), C.c_int(0)
        self.ctx.check(lib().psm_sort_get_algorithm(self.ctx._h, C.byref(a), C.byref(e)), "psm_sort_get_algorithm")
        return a.value, e.value

    def sort(self, keys_handle, vals_handle, size=1, descending=0):
        # `descending` is accepted and ignored like the reference's shaders do (radix/includes.glsl:50-55)
        self.ctx.check(lib().psm_sort_u64_u32(self.ctx._h, C.c_uint32(keys_handle), C.c_uint32(vals_handle),
                                              C.c_uint32(size)), "psm_sort_u64_u32")

    def sort_arrays(self, keys, vals):
        """Convenience: host arrays in, sorted host arrays out."""
        keys = np.ascontiguousarray(keys, np.uint64)
        vals = np.ascontiguousarray(vals, np.uint32)
        n = keys.shape[0]
        hk = self.ctx.buf_alloc(max(n, 1) * 8)
        hv = self.ctx.buf_alloc(max(n, 1) * 4)
        try:
            if n:
                self.ctx.buf_upload(hk, keys)
                self.ctx.buf_upload(hv, vals)
            self.sort(hk, hv, n)
            return self.ctx.buf_download(hk, np.uint64, n), self.ctx.buf_download(hv, np.uint32, n)
        finally:
            self.ctx.buf_free(hk)
            self.ctx.buf_free(hv)


class TriangleHierarchy:
    """psm::TriangleHierarchy (Include/Prismarine/TriangleHierarchy.hpp:75-94)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self._h = C.c_void_p()
        self.triangleCount = 0
        self.materialID = 0
        self._dirty = False
        self.maxt = 0

    def allocate(self, count):
        if self._h:
            lib().psm_bvh_destroy(self._h)
            self._h = C.c_void_p()
        self.ctx.check(lib().psm_bvh_create(self.ctx._h, C.c_size_t(count), C.byref(self._h)), "psm_bvh_create")
        self.maxt = count
        self.clearTribuffer()

    def clearTribuffer(self):
        self.markDirty()
        self.ctx.check(lib().psm_bvh_clear(self._h), "psm_bvh_clear")
        self.triangleCount = 0

    def setMaterialID(self, mid):
        self.materialID = mid

    def loadTriangles(self, tris, normals=None, mats=None, texcoords=None):
        """loadMesh() reduced to its result: append world-space triangles (loader.comp:115-135);
        texcoords: float32 [n,3,2] (u,v per vertex) or None."""
        tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
        n = tris.shape[0]
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 9)
        mm = None if mats is None else np.ascontiguousarray(mats, np.int32)
        self.ctx.check(lib().psm_bvh_load_triangles(self._h, _p(tris), _p(nrm) if nrm is not None else None,
                                                    _p(mm) if mm is not None else None, C.c_size_t(n),
                                                    C.c_int32(self.materialID)), "psm_bvh_load_triangles")
        if texcoords is not None:
            tc = np.ascontiguousarray(texcoords, np.float32).reshape(-1, 6)
            if tc.shape[0] != n:
                raise ValueError("texcoords: expected %d triangles, got %d" % (n, tc.shape[0]))
            self.ctx.check(lib().psm_bvh_set_texcoords(self._h, C.c_size_t(self.triangleCount), _p(tc), C.c_size_t(n)),
                           "psm_bvh_set_texcoords")
        self.triangleCount += n
        self.markDirty()

    def loadMesh(self, mesh):
        """loadMesh(TriangleArrayInstance*) (TriangleHierarchy.inl:173-192): `mesh` is a dict with the
        fields of VertexInstance.hpp -- vertices (float pool), indices (uint32 words or None), accessors
        [(offset4, components, bufferView)], views [(offset4, stride4)], vertex_accessor, normal_accessor,
        texcoord_accessor (v is stored as 1 - v, loader.comp:97-99),
        transform / transform_inv (row-major 4x4), material_id, index16, node_count, primitive_type,
        loading_offset. The pools are uploaded to device buffers and resolved by the HIP gather kernel."""
        self.loadMeshes([mesh])

    def loadMeshes(self, meshes):
        """loadMesh for every description of `meshes`, in order. Descriptions that share a pool (the same numpy array: the
        primitives of one glTF buffer, gltf.read_gltf) share its upload, as the reference's primitives share a GL buffer
        (Viewer.cpp:133-139)."""
        pools = {}   # (address, bytes) -> (handle, contiguous array kept alive): float and word views of one buffer share an upload
        self.pool_uploads = 0   # device pools the last loadMeshes made: one per distinct stretch of memory, however many views name it

        def dev(a, dtype):
            c = np.ascontiguousarray(a, dtype)   # (a view of the right dtype comes back as itself: same memory, same key)
            key = (c.__array_interface__["data"][0], c.nbytes)   # (both pool types are 4-byte words: the bytes are the same)
            if key not in pools:
                h = self.ctx.buf_alloc(max(c.nbytes, 4))
                pools[key] = (h, c, a)
                self.ctx.buf_upload(h, c)
                self.pool_uploads += 1
            h, c, _ = pools[key]
            return self.ctx.buf_ptr(h)[0], c.size

        try:
            for mesh in meshes:
                idx = mesh.get("indices")
                acc = (Accessor * len(mesh["accessors"]))(*[Accessor(*a) for a in mesh["accessors"]])
                views = (BufferView * len(mesh["views"]))(*[BufferView(*v) for v in mesh["views"]])
                d = MeshDesc()
                d.d_vertices, d.vertex_floats = dev(mesh["vertices"], np.float32)
                d.d_indices, d.index_words = dev(idx, np.uint32) if idx is not None else (None, 0)
                d.accessors, d.accessor_count = C.cast(acc, C.c_void_p), len(mesh["accessors"])
                d.views, d.view_count = C.cast(views, C.c_void_p), len(mesh["views"])
                d.vertex_accessor, d.normal_accessor = mesh["vertex_accessor"], mesh.get("normal_accessor", -1)
                d.texcoord_accessor, d.modifier_accessor = mesh.get("texcoord_accessor", -1), -1
                t = np.ascontiguousarray(mesh["transform"], np.float32).reshape(16)
                ti = np.ascontiguousarray(mesh["transform_inv"], np.float32).reshape(16)
                for k in range(16):
                    d.transform[k], d.transform_inv[k] = t[k], ti[k]
                d.material_id, d.is_indexed, d.index16 = mesh.get("material_id", self.materialID), int(idx is not None), int(mesh.get("index16", 0))
                d.node_count, d.primitive_type = mesh["node_count"], mesh.get("primitive_type", 0)
                d.loading_offset = mesh.get("loading_offset", 0)
                self.ctx.check(lib().psm_bvh_load_mesh(self._h, C.byref(d)), "psm_bvh_load_mesh")
                self.triangleCount += mesh["node_count"] * (2 if mesh.get("primitive_type", 0) == 1 else 1)
                self.markDirty()
        finally:
            for h, _, _ in pools.values():
                self.ctx.buf_free(h)

    def isDirty(self):
        return self._dirty

    def markDirty(self):
        self._dirty = True

    def resolve(self):
        self._dirty = False

    def build(self, optimization=None):
        if self.triangleCount <= 0 or not self._dirty:  # TriangleHierarchy.inl:214
            return
        opt = None if optimization is None else np.ascontiguousarray(optimization, np.float64).reshape(16)
        self.ctx.check(lib().psm_bvh_build(self._h, _p(opt) if opt is not None else None), "psm_bvh_build")
        self.resolve()

    def refit(self):
        """psm_bvh_refit (not in the reference): the triangles were reloaded -- same count, same order, moved -- and only
        the boxes are recomputed; the tree is the last build's."""
        self.ctx.check(lib().psm_bvh_refit(self._h), "psm_bvh_refit")
        self.resolve()

    def intersect(self, origins, directions, tmin=0.0, tmax=np.inf):
        """Closest hit of every ray (psm_bvh_intersect_dev; not in the reference): origins, directions [n, 3], tmin / tmax scalars or
        per-ray [n]. numpy in: numpy out (staged through device buffers; synchronises). torch device tensors in: torch tensors out on
        the same device, no copy through the host, ordered against torch's current stream without synchronising. Returns QueryHits:
        t, u, v, tri (tri = -1, t = +inf on a miss) as views of one [n, 4] float32 buffer (u, v, t, tri as int32 bits)."""
        return self._query(origins, directions, tmin, tmax, "hits")

    def occluded(self, origins, directions, tmin=0.0, tmax=np.inf):
        """Any hit inside [tmin, tmax] per ray (psm_bvh_occluded_dev; not in the reference): a bool array / tensor. Arguments and
        placement as intersect()."""
        return self._query(origins, directions, tmin, tmax, "bool")

    def firstHits(self, origins, directions, k, tmin=0.0, tmax=np.inf):
        """The first k hits of every ray, in order (psm_bvh_first_hits_dev; not in the reference): of the triangles countHits()
        counts, the min(k, count) smallest in (t, tri) -- bit-equal t (coincident triangles, a shared edge) are all listed, by id.
        k: 1 .. QUERY_K_MAX. Returns QueryHitLists: u, v, t, tri [n, k] (slot 0 is intersect()'s record; the slots past count are
        misses: tri = -1, t = +inf) and count [n]. Arguments and placement as intersect(). QueryScene and InstancedScene have
        no such query; InstanceWorld has (InstanceWorld.firstHits)."""
        return self._query(origins, directions, tmin, tmax, "lists", "psm_bvh_first_hits_dev", k)

    def nearest(self, points, k, rmax=np.inf):
        """The k nearest triangles of every point within rmax (psm_bvh_nearest_dev; not in the reference): the min(k, count)
        smallest in (d2, tri). k: 1 .. QUERY_K_MAX. Returns QueryHitLists: t = the distance, and u, v as closestPoint()'s (slot 0
        is closestPoint()'s record). Arguments and placement as closestPoint()."""
        return self._point_query(points, rmax, "lists", "psm_bvh_nearest_dev", k=k)

    def boxOverlaps(self, lo, hi):
        """Whether some triangle overlaps each axis-aligned box [lo, hi] (psm_bvh_box_overlaps_dev; not in the reference): lo, hi
        [n, 3]; the box is closed (touching counts), a point (lo == hi) is a box, and a box with a non-finite number or lo > hi on
        an axis overlaps nothing. The test is the 13 separating axes of a triangle and a box in float32 (psm_hip.h "box queries").
        A bool array / tensor. numpy in: numpy out; torch device tensors in: torch tensors out on the same device, ordered against
        torch's current stream without synchronising (as intersect()). QueryScene and InstancedScene have no box queries;
        InstanceWorld has its own (overlapsBox / countInBox / trianglesInBox: the box in world space)."""
        return self._box_query(lo, hi, "bool", "psm_bvh_box_overlaps_dev")

    def boxCount(self, lo, hi):
        """The number of triangles that overlap each box (psm_bvh_box_count_dev; not in the reference): what boxOverlaps() asks
        "is there one?" about, counted. A uint32 array, or an int32 tensor for torch tensors. Arguments and placement as
        boxOverlaps()."""
        return self._box_query(lo, hi, "count", "psm_bvh_box_count_dev")

    def boxTriangles(self, lo, hi, k):
        """Which triangles overlap each box (psm_bvh_box_triangles_dev; not in the reference): of the triangles boxCount() counts,
        the min(k, count) lowest ids, ascending. k: 1 .. QUERY_K_MAX. Returns QueryTriLists: tri [n, k] int32 (-1 past count) and
        count [n]; with k >= boxCount() the row is the complete list. Arguments and placement as boxOverlaps()."""
        if not 1 <= _k(k, "psm_bvh_box_triangles_dev") <= QUERY_K_MAX:   # (refused here: no call is made)
            raise PsmError("psm_bvh_box_triangles_dev: k must be 1 .. %d" % QUERY_K_MAX)
        return self._box_query(lo, hi, "tris", "psm_bvh_box_triangles_dev", k)

    def _box_query(self, lo, hi, out, name, k=None):
        """lo, hi [n, 3] packed into psm_box_query records (the pads are 0) on the side the arguments live on"""
        extra = () if k is None else (C.c_uint32(int(k)),)
        if type(lo).__module__.split(".")[0] == "torch":
            import torch
            dev = lo.device
            if dev.type != "cuda" or getattr(hi, "device", None) != dev:
                raise ValueError("box queries: lo and hi must be tensors on the context's device")
            a, b = lo.reshape(-1, 3), hi.reshape(-1, 3)
            if a.shape[0] != b.shape[0]:
                raise ValueError("lo and hi: %d against %d boxes" % (a.shape[0], b.shape[0]))
            boxes = torch.zeros((a.shape[0], 8), dtype=torch.float32, device=dev)
            boxes[:, 0:3] = a
            boxes[:, 4:7] = b
            return _launch_torch(self, boxes, out, name, *extra)
        a = np.ascontiguousarray(lo, np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(hi, np.float32).reshape(-1, 3)
        if a.shape[0] != b.shape[0]:
            raise ValueError("lo and hi: %d against %d boxes" % (a.shape[0], b.shape[0]))
        boxes = np.zeros((a.shape[0], 8), np.float32)
        boxes[:, 0:3], boxes[:, 4:7] = a, b
        return self._launch_np(boxes, out, name, *extra)

    def voxelize(self, origin, cell, dims, solid=False, samples=3, as_torch=False):
        """The voxels of a regular grid that a triangle overlaps (psm_grid_surface_dev; not in the reference), or with solid=True
        those and the voxels whose centre inside() takes as inside with `samples` (1, 3 or 5) rays (psm_grid_solid_dev): the filled
        model of a closed mesh. origin: the corner of voxel (0, 0, 0); cell: the voxel size, a scalar or one per axis; dims: (nx,
        ny, nz). Voxel (ix, iy, iz) is the closed box voxel_boxes() states, and its bit is bit for bit what boxOverlaps() answers
        for that box: one call, no box records, 8 bytes of answer per 64 voxels. Returns VoxelGrid: bricks [nbz, nby, nbx] of 4 x 4
        x 4 voxels, a uint64 word each (with as_torch=True an int64 tensor of the same bits on the context's device, the launch
        ordered against torch's current stream by events, no host synchronisation); dense() and occupied() read them. An invalid
        grid raises ValueError before any call. QueryScene and InstancedScene have no grids; InstanceWorld has its own (voxelize /
        voxelCounts / voxelInstances: the grid in world space)."""
        g = _grid(origin, cell, dims)
        return _voxel_call(self.ctx, self._h, "psm_grid_", "solid" if solid else "surface", g, np.uint64, as_torch,
                           samples if solid else None)

    def voxelCounts(self, origin, cell, dims, as_torch=False):
        """How many triangles overlap each voxel of a regular grid (psm_grid_counts_dev; not in the reference): uint32 [nz, ny, nx]
        (an int32 tensor with as_torch=True, as boxCount()'s), each entry what boxCount() answers for the voxel's box. Arguments
        and placement as voxelize()."""
        g = _grid(origin, cell, dims)
        return _voxel_call(self.ctx, self._h, "psm_grid_", "counts", g, np.uint32, as_torch)

    def distanceField(self, origin, cell, dims, rmax=np.inf, signed=False, samples=3, nearest=True, as_torch=False):
        """The distance from every voxel centre of a regular grid to the nearest triangle (psm_grid_distance_dev; not in the
        reference), or with signed=True that distance with the sign of inside(centre, samples) (psm_grid_signed_distance_dev):
        a distance field for planners, collision margins, offset surfaces and narrow-band level sets in one call, with no point
        records to make, upload or read back. origin, cell, dims: the grid, as voxelize() takes it; the centres are
        voxel_centres()'s. rmax: the narrow band, >= 0 or inf; a voxel with no triangle within rmax holds +inf (and tri -1), and
        in a signed field casts no rays and keeps its sign bit clear. Every voxel is bit for bit what closestPoint() /
        signedDistance() answer for its centre with the same rmax and samples (t and tri; -0.0 can occur in a signed field); on
        a bit-equal squared distance the lowest triangle id wins. Returns DistanceGrid: dist float32 [nz, ny, nx] and tri int32
        [nz, ny, nx] (None with nearest=False: the ids are not stored); with as_torch=True torch tensors on the context's
        device, the launch ordered against torch's current stream by events, no host synchronisation. An invalid grid and a NaN
        or negative rmax raise ValueError before any call; samples other than 1, 3 or 5 are the library's to refuse. Not
        covered: distance fields over a QueryScene or an InstancedScene (an InstanceWorld has its own distanceField); u, v and
        the closest point per voxel
        (closestPoint() answers them for the voxels that need them); a per-voxel rmax; a sparse output; sweeping-based
        (approximate) distance transforms; graph capture of the signed call."""
        g, r = _grid(origin, cell, dims), _rmax(rmax)
        return _distance_call(self.ctx, self._h, "psm_grid_", g, r, signed, samples, nearest, as_torch)

    def sparseVoxelize(self, origin, cell, dims, bricks=None, as_torch=False):
        """voxelize()'s surface for the non-empty bricks alone (psm_grid_sparse_surface_bricks_dev / psm_grid_sparse_surface_dev;
        not in the reference): the ascending indices of the 4 x 4 x 4 bricks whose word is non-zero, and those words, bit for bit
        voxelize()'s. bricks=None: the call lists with capacity 0 and reads the count -- its one synchronisation --, lists into
        an array of exactly that size and fills it. bricks given (a numpy or torch array of uint32 brick indices (bz * nby +
        by) * nbx + bx; torch: int32 or uint32 holding those bits): only the fill, slot i answering bricks[i]; any order,
        duplicates allowed, an index at or above the brick count is an empty brick. Returns SparseVoxelGrid. Grid arguments and
        as_torch as voxelize(). Not covered: solid or counts in sparse form; an InstanceWorld's grids."""
        g = _grid(origin, cell, dims)
        return _sparse_call(self.ctx, self._h, g, None, False, None, False, bricks, as_torch)

    def sparseDistanceField(self, origin, cell, dims, rmax, signed=False, samples=3, nearest=True, bricks=None, as_torch=False):
        """distanceField()'s narrow band for the bricks it reaches alone (psm_grid_sparse_distance_bricks_dev /
        psm_grid_sparse_distance_dev / psm_grid_sparse_signed_distance_dev; not in the reference): the ascending indices of the
        4 x 4 x 4 bricks with a voxel centre within rmax of a triangle, and the (signed) distances and nearest triangles of
        their 64 voxels each, bit for bit distanceField()'s with the same rmax and samples; a voxel outside dims holds +inf /
        -1. Memory and time follow the band, not the grid. bricks: as sparseVoxelize() (None: list, one synchronisation, then
        fill; given: fill that list). Returns SparseDistanceGrid; tri is None with nearest=False. Not covered: an
        InstanceWorld's fields; dilating a list."""
        g, r = _grid(origin, cell, dims), _rmax(rmax)
        return _sparse_call(self.ctx, self._h, g, r, signed, samples, nearest, bricks, as_torch)

    def triOverlaps(self, tris):
        """Whether some triangle of the hierarchy meets each query triangle (psm_bvh_tri_overlaps_dev; not in the reference): tris
        [n, 3, 3] or [n, 9], the vertices a, b, c of each. Closed (touching counts); a segment or a point is a valid query
        triangle, one with a non-finite number meets nothing. The test is a separating-axis test over 20 axes in float32
        (psm_hip.h "triangle queries"). A bool array / tensor. numpy in: numpy out; torch device tensors in: torch tensors out on
        the same device, ordered against torch's current stream without synchronising (as intersect()). QueryScene and
        InstancedScene have no triangle queries; InstanceWorld has its own (overlapsTriangle / countOnTriangle /
        trianglesOnTriangle: the query triangle in world space)."""
        return self._tri_query(tris, "bool", "psm_bvh_tri_overlaps_dev")

    def triCount(self, tris):
        """The number of triangles that meet each query triangle (psm_bvh_tri_count_dev; not in the reference): what
        triOverlaps() asks "is there one?" about, counted. A uint32 array, or an int32 tensor for torch tensors. Arguments and
        placement as triOverlaps()."""
        return self._tri_query(tris, "count", "psm_bvh_tri_count_dev")

    def triTriangles(self, tris, k):
        """Which triangles meet each query triangle (psm_bvh_tri_triangles_dev; not in the reference): of the triangles
        triCount() counts, the min(k, count) lowest ids, ascending. k: 1 .. QUERY_K_MAX. Returns QueryTriLists: tri [n, k] int32
        (-1 past count) and count [n]; with k >= triCount() the row is the complete list. Arguments and placement as
        triOverlaps()."""
        if not 1 <= _k(k, "psm_bvh_tri_triangles_dev") <= QUERY_K_MAX:   # (refused here: no call is made)
            raise PsmError("psm_bvh_tri_triangles_dev: k must be 1 .. %d" % QUERY_K_MAX)
        return self._tri_query(tris, "tris", "psm_bvh_tri_triangles_dev", k)

    def _tri_query(self, tris, out, name, k=None):
        """tris [n, 3, 3] or [n, 9] packed into psm_tri_query records (the pads are 0) on the side the argument lives on"""
        extra = () if k is None else (C.c_uint32(int(k)),)
        if type(tris).__module__.split(".")[0] == "torch":
            import torch
            dev = tris.device
            if dev.type != "cuda":
                raise ValueError("triangle queries: tris must be a tensor on the context's device")
            t = tris.reshape(-1, 3, 3)
            packed = torch.zeros((t.shape[0], 3, 4), dtype=torch.float32, device=dev)
            packed[:, :, 0:3] = t
            return _launch_torch(self, packed.reshape(-1, 12), out, name, *extra)
        t = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
        packed = np.zeros((t.shape[0], 3, 4), np.float32)
        packed[:, :, 0:3] = t
        return self._launch_np(packed.reshape(-1, 12), out, name, *extra)

    def triClosest(self, tris, rmax=np.inf):
        """The nearest triangle of the hierarchy to each query triangle within rmax, its distance and the two nearest points
        (psm_bvh_tri_closest_dev; not in the reference): tris [n, 3, 3] or [n, 9], rmax a scalar or [n] (+inf: no limit; NaN
        or negative: a miss). Triangles that meet have distance 0; a segment or a point is a valid query triangle. The distance
        is the smallest of fifteen vertex-face and edge-edge features in float32 (psm_hip.h "clearance queries"); on a bit-equal
        squared distance the lowest id wins. Returns QueryTriHits: u, v, dist, tri, s, t (tri = -1, dist = +inf on a miss).
        numpy in: numpy out; torch device tensors in: torch tensors out on the same device, ordered against torch's current
        stream without synchronising (as intersect()). QueryScene and InstancedScene have no clearance queries; an
        InstanceWorld has closestToTriangle() / withinOfTriangle()."""
        return self._tri_dist_query(tris, rmax, "trihits", "psm_bvh_tri_closest_dev")

    def triWithin(self, tris, r):
        """Whether some triangle of the hierarchy is within r of each query triangle (psm_bvh_tri_within_dev; not in the
        reference): triClosest(tris, r).tri >= 0, with the walk ended at the first such triangle. A bool array / tensor.
        Arguments and placement as triClosest()."""
        return self._tri_dist_query(tris, r, "bool", "psm_bvh_tri_within_dev")

    def _tri_dist_query(self, tris, rmax, out, name):
        """tris [n, 3, 3] or [n, 9] and rmax packed into psm_tri_dist_query records (the pads are 0) on the side tris lives on"""
        if type(tris).__module__.split(".")[0] == "torch":
            import torch
            dev = tris.device
            if dev.type != "cuda":
                raise ValueError("clearance queries: tris must be a tensor on the context's device")
            t = tris.reshape(-1, 3, 3)
            packed = torch.zeros((t.shape[0], 3, 4), dtype=torch.float32, device=dev)
            packed[:, :, 0:3] = t
            packed[:, 0, 3] = torch.as_tensor(rmax, dtype=torch.float32, device=dev)
            return _launch_torch(self, packed.reshape(-1, 12), out, name)
        t = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
        packed = np.zeros((t.shape[0], 3, 4), np.float32)
        packed[:, :, 0:3] = t
        packed[:, 0, 3] = rmax
        return self._launch_np(packed.reshape(-1, 12), out, name)

    def meshOverlaps(self, other, poses, as_torch=False):
        """Whether `other`, another built TriangleHierarchy of this context, meets this one anywhere at each pose
        (psm_bvh_mesh_overlaps_dev; not in the reference). poses: one matrix or [p, 3, 4] / [p, 4, 4], each a rigid [R | T] that
        takes a point of other's object space into this hierarchy's (x' = R x + T), checked as an instance's pose is: a
        non-rigid one raises before any call. The query triangles are other's stored leaves posed in float32 on the device
        (psm_hip.h "mesh queries"); each is answered bit for bit as triOverlaps() answers it. A numpy bool [p]; with
        as_torch=True a torch bool tensor on the context's device, the launch ordered against torch's current stream by events
        (the call itself waits once for its pose upload, as InstanceWorld.setTransforms does). QueryScene and InstancedScene
        have no mesh queries; an InstanceWorld has overlapsMesh() / countOnMesh() / trianglesOnMesh()."""
        return self._mesh_query(other, poses, "bool", "psm_bvh_mesh_overlaps_dev", None, as_torch)

    def meshCount(self, other, poses, as_torch=False):
        """How many triangles of this hierarchy meet each triangle of `other` at each pose (psm_bvh_mesh_count_dev; not in the
        reference): uint32 [p, T], T = other.triangleCount, indexed by other's load-order triangle id (an int32 tensor with
        as_torch=True); a triangle other's build dropped counts 0. With other = self at the identity every leaf counts at
        least itself. Arguments and placement as meshOverlaps()."""
        return self._mesh_query(other, poses, "count", "psm_bvh_mesh_count_dev", None, as_torch)

    def meshTriangles(self, other, poses, k, as_torch=False):
        """Which triangles of this hierarchy meet each triangle of `other` at each pose (psm_bvh_mesh_triangles_dev; not in the
        reference): of the triangles meshCount() counts, the min(k, count) lowest ids, ascending. k: 1 .. QUERY_K_MAX. Returns
        QueryTriLists: tri [p, T, k] int32 (-1 past count) and count [p, T]. Arguments and placement as meshOverlaps()."""
        if not 1 <= _k(k, "psm_bvh_mesh_triangles_dev") <= QUERY_K_MAX:   # (refused here: no call is made)
            raise PsmError("psm_bvh_mesh_triangles_dev: k must be 1 .. %d" % QUERY_K_MAX)
        return self._mesh_query(other, poses, "tris", "psm_bvh_mesh_triangles_dev", int(k), as_torch)

    def _mesh_query(self, other, poses, out, name, k, as_torch):
        """one mesh query: the poses checked and packed [p, 12] on the host, the outputs [p] / [p, T] / [p, T, k] and [p, T]"""
        m12, p, t = _mesh_poses(other, poses, name)
        extra = () if k is None else (C.c_uint32(k),)
        fn = getattr(lib(), name)

        def call(*d_outs):
            self.ctx.check(fn(self._h, other._h, _p(m12), C.c_size_t(p), *extra, *map(C.c_void_p, d_outs)), name)

        res = _device_call(self.ctx, call, _mesh_outs(out, p, t, k, False), as_torch)
        if out == "tris":
            return QueryTriLists(*res)
        return _bool_view(res[0]) if out == "bool" else res[0]

    def meshClosest(self, other, poses, rmax=np.inf, as_torch=False):
        """The nearest triangle of this hierarchy to each triangle of `other` at each pose within rmax, its distance and the two
        nearest points (psm_bvh_mesh_closest_dev; not in the reference): each stored triangle of other is posed in float32 on
        the device, as meshCount() poses it, and answered bit for bit as triClosest() answers it. rmax: one scalar (+inf: no
        limit; NaN or negative: a miss everywhere). Returns QueryMeshHits over a [p, T, 8] buffer, T = other.triangleCount,
        indexed by other's load-order triangle id: u, v, dist, tri, s, t ([p, T] views; tri = -1, dist = +inf on a miss and for
        a triangle other's build dropped); .other is None. Arguments and placement as meshOverlaps()."""
        return self._mesh_dist_query(other, poses, rmax, "closest", "psm_bvh_mesh_closest_dev", as_torch)

    def meshWithin(self, other, poses, r, as_torch=False):
        """Whether some triangle of `other` comes within r of some triangle of this hierarchy at each pose
        (psm_bvh_mesh_within_dev; not in the reference): meshClearance(other, poses, r).tri >= 0, with every walk ended at its
        first such pair. A bool [p]. Arguments and placement as meshOverlaps()."""
        return self._mesh_dist_query(other, poses, r, "bool", "psm_bvh_mesh_within_dev", as_torch)

    def meshClearance(self, other, poses, rmax=np.inf, as_torch=False):
        """The one nearest pair of each pose (psm_bvh_mesh_clearance_dev; not in the reference): of meshClosest()'s records of
        a pose the one with the smallest dist, on an equal float32 dist the lowest triangle of other -- found inside the launch,
        the triangles of a pose sharing the best distance so far as their bound. Returns QueryMeshHits over a [p, 8] buffer:
        u, v, dist, tri, s, t and .other, the int32 id of other's triangle (tri = other = -1, dist = +inf where no pair is
        within rmax); .points() gives the two witness points. Arguments and placement as meshOverlaps()."""
        return self._mesh_dist_query(other, poses, rmax, "clearance", "psm_bvh_mesh_clearance_dev", as_torch)

    def _mesh_dist_query(self, other, poses, rmax, out, name, as_torch):
        """one mesh clearance query: the poses as _mesh_query packs them, rmax one float, the output [p, T, 8] / [p] / [p, 8]"""
        m12, p, t = _mesh_poses(other, poses, name)
        if np.ndim(rmax) != 0:
            raise ValueError("%s: rmax must be one scalar" % name)
        fn = getattr(lib(), name)

        def call(d_out):
            self.ctx.check(fn(self._h, other._h, _p(m12), C.c_size_t(p), C.c_float(rmax), C.c_void_p(d_out)), name)

        res, = _device_call(self.ctx, call, _mesh_dist_outs(out, p, t, False), as_torch)
        return _bool_view(res) if out == "bool" else QueryMeshHits(res, out == "clearance")

    def sweepSphere(self, origins, directions, radius, tmax=np.inf):
        """Where a sphere of `radius` that moves from each origin along its direction first touches a triangle within the distance
        tmax (psm_bvh_sweep_sphere_dev; not in the reference): origins, directions [n, 3] (any length; normalised inside, t is
        the distance along the unit direction), radius and tmax scalars or per-sweep [n]. Returns QueryHits: t = the distance the
        centre travels to the first contact (0: the sphere touches where it starts -- whenever within(origin, radius) says so,
        and for a sphere within rounding of its radius of a triangle it is moving into), tri the triangle, and u, v with the contact point = (v0 + u e1) + v e2 (tri = -1, t = +inf: no contact); the
        contact normal is (origin + t d - contact) / radius. A non-finite origin or direction, a zero direction, a radius that is
        negative, NaN or infinite and a negative or NaN tmax miss. numpy in: numpy out; torch device tensors in: torch tensors
        out on the same device, ordered against torch's current stream without synchronising (as intersect()). QueryScene
        and InstancedScene have no sweeps; InstanceWorld has its own (sphereCast / sphereCastOccluded: the sweep in world
        space)."""
        return self._query(origins, directions, radius, tmax, "hits", "psm_bvh_sweep_sphere_dev")

    def sweepOccluded(self, origins, directions, radius, tmax=np.inf):
        """Whether the swept sphere touches any triangle within tmax (psm_bvh_sweep_occluded_dev; not in the reference): the
        predicate isfinite(sweepSphere().t), the walk ending at the first contact found. A bool array / tensor. Arguments and
        placement as sweepSphere()."""
        return self._query(origins, directions, radius, tmax, "bool", "psm_bvh_sweep_occluded_dev")

    def _query(self, origins, directions, tmin, tmax, out, name=None, k=None):
        name = name or _RAY_QUERIES[out]
        extra = () if k is None else (C.c_uint32(_k(k, name)),)
        if type(origins).__module__.split(".")[0] == "torch":
            return _query_torch(self, origins, directions, tmin, tmax, out, name, *extra)
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        n = o.shape[0]
        if d.shape[0] != n:
            raise ValueError("origins and directions: %d against %d rays" % (n, d.shape[0]))
        rays = np.empty((n, 8), np.float32)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, tmin, d, tmax
        return self._launch_np(rays, out, name, *extra)

    def countHits(self, origins, directions, tmin=0.0, tmax=np.inf):
        """The number of triangles each ray hits inside [tmin, tmax] (psm_bvh_count_hits_dev; not in the reference): what occluded()
        asks "is there one?" about, counted. A uint32 array, or for torch tensors an int32 tensor on the same device (torch has
        no general uint32). Arguments and placement as intersect()."""
        return self._query(origins, directions, tmin, tmax, "count")

    def inside(self, points, samples=3):
        """Whether each point is inside the surface (psm_bvh_inside_dev; not in the reference): `samples` (1, 3 or 5) rays from
        the point along INSIDE_DIRECTIONS, each voting "inside" iff it crosses an odd number of triangles; the majority decides. A
        bool array / tensor. Right for a closed surface (a vote, because a ray within 1e-5 of a shared edge is counted by both of
        its triangles); for an open one merely deterministic. points and placement as closestPoint(); a packed [n, 4] array or
        tensor of (p, rmax) records is taken as it is (rmax is ignored)."""
        return self._point_query(points, np.inf, "bool", "psm_bvh_inside_dev", samples)

    def signedDistance(self, points, rmax=np.inf, samples=3):
        """closestPoint() with the sign of inside() (psm_bvh_signed_distance_dev; not in the reference): QueryHits whose t is the
        distance, negative inside (-0.0 for a point on the surface that the vote takes as inside). A point with no triangle within
        rmax stays a miss (tri = -1, t = +inf) and casts no rays: with a finite rmax, a narrow-band distance field."""
        return self._point_query(points, rmax, "hits", "psm_bvh_signed_distance_dev", samples)

    def closestPoint(self, points, rmax=np.inf):
        """Closest point on the hierarchy's triangles of every point within rmax (psm_bvh_closest_point_dev; not in the reference):
        points [n, 3], rmax a scalar or per-point [n]. numpy in: numpy out; torch device tensors in: torch tensors out on the same
        device, ordered against torch's current stream (as intersect()). Returns QueryHits: t = the distance, tri, and u, v with
        the point = (v0 + u e1) + v e2 of triangle tri (tri = -1, t = +inf when no triangle is within rmax)."""
        return self._point_query(points, rmax, "hits", "psm_bvh_closest_point_dev")

    def within(self, points, radius):
        """Whether some triangle is within `radius` (a scalar or per-point [n]) of each point (psm_bvh_within_dev; not in the
        reference): a bool array / tensor. Arguments and placement as closestPoint()."""
        return self._point_query(points, radius, "bool", "psm_bvh_within_dev")

    def _point_query(self, points, rmax, out, name, samples=None, k=None):
        """points [n, 3] with rmax, or (the inside queries only) [n, 4] records already packed; samples: the inside queries' extra
        argument, k: the k-best queries'"""
        extra = () if samples is None else (C.c_uint32(_samples(samples, name)),)
        if k is not None:
            extra = (C.c_uint32(_k(k, name)),)
        packed = samples is not None and getattr(points, "ndim", 0) == 2 and points.shape[1] == 4
        if type(points).__module__.split(".")[0] == "torch":
            import torch
            dev = points.device
            if dev.type != "cuda":
                raise ValueError("point queries: points must be a tensor on the context's device")
            if packed and points.dtype == torch.float32 and points.is_contiguous():
                return _launch_torch(self, points, out, name, *extra)
            p = points[:, 0:3] if packed else points.reshape(-1, 3)
            q = torch.empty((p.shape[0], 4), dtype=torch.float32, device=dev)
            q[:, 0:3] = p
            q[:, 3] = points[:, 3] if packed else torch.as_tensor(rmax, dtype=torch.float32, device=dev)
            return _launch_torch(self, q, out, name, *extra)
        if packed:
            return self._launch_np(np.ascontiguousarray(points, np.float32), out, name, *extra)
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        q = np.empty((p.shape[0], 4), np.float32)
        q[:, 0:3], q[:, 3] = p, rmax
        return self._launch_np(q, out, name, *extra)

    def _launch_np(self, packed, out, name, *extra):
        return _launch_np(self, packed, out, name, *extra)

    def _call(self, name, d_in, n, extra, d_out, d_geom):
        """the native call of one query launch (d_geom: a single hierarchy reports no geometry; the k-best queries' counts; a
        world's k-best queries: the pair (instances, counts))"""
        tail = () if d_geom is None else (C.c_void_p(d_geom),)
        self.ctx.check(getattr(lib(), name)(self._h, C.c_void_p(d_in), C.c_size_t(n), *extra, C.c_void_p(d_out), *tail), name)

    _scene = False   # (QueryScene: True -- a "hits" result then carries QueryHits.geom)

    def setBuildGraph(self, enable=True):
        """Replay rebuilds as one captured hipGraph from the second build of a triangle count on (default), or keep plain launches."""
        self.ctx.check(lib().psm_bvh_set_build_graph(self._h, C.c_int(1 if enable else 0)), "psm_bvh_set_build_graph")

    def stage(self, name, optimization=None):
        if name == "bounds":
            opt = None if optimization is None else np.ascontiguousarray(optimization, np.float64).reshape(16)
            rc = lib().psm_bvh_stage_bounds(self._h, _p(opt) if opt is not None else None)
        else:
            rc = getattr(lib(), "psm_bvh_stage_" + name)(self._h)
        self.ctx.check(rc, "psm_bvh_stage_" + name)

    def info(self):
        i = BvhInfo()
        self.ctx.check(lib().psm_bvh_get_info(self._h, C.byref(i)), "psm_bvh_get_info")
        return i

    def download(self, what, dtype, count):
        out = np.zeros(count, dtype)
        if count:
            self.ctx.check(lib().psm_bvh_download(self._h, C.c_int(what), _p(out), C.c_size_t(out.nbytes)),
                           "psm_bvh_download")
        return out

    def close(self):
        if self._h:
            lib().psm_bvh_destroy(self._h)
            self._h = C.c_void_p()


# a query's result by kind: bytes per query and the numpy type of the array returned ("hits": QueryHits over float32 [n, 4];
# "lists": QueryHitLists over float32 [n, k, 4] -- 16 bytes per slot, k the launch's extra argument -- and a count per query;
# "tris": QueryTriLists over int32 [n, k] -- 4 bytes per slot -- and a count per query)
# "trihits": QueryTriHits over float32 [n, 8] -- psm_tri_hit, 32 bytes per query
_QUERY_OUT = {"trihits": (32, np.float32), "hits": (16, np.float32), "bool": (1, np.bool_), "count": (4, np.uint32), "lists": (16, np.float32), "tris": (4, np.int32)}
_RAY_QUERIES = {"hits": "psm_bvh_intersect_dev", "bool": "psm_bvh_occluded_dev", "count": "psm_bvh_count_hits_dev"}


def _samples(samples, name):
    """the inside queries' sample count as the C ABI takes it (a uint32; which values are allowed is the library's to say)"""
    s = int(samples)
    if s != samples or not 0 <= s < 1 << 32:
        raise ValueError("%s: samples must be 1, 3 or 5" % name)
    return s


def _k(k, name):
    """the k-best queries' k as the C ABI takes it (a uint32; the library refuses 0 and k > QUERY_K_MAX)"""
    v = int(k)
    if v != k or not 0 <= v < 1 << 32:
        raise ValueError("%s: k must be 1 .. %d" % (name, QUERY_K_MAX))
    return v


GRID_DIM_MAX = 1 << 20   # psm_hip.h PSM_GRID_DIM_MAX


def _rmax(rmax):
    """a distance field's narrow band as a float; NaN or a negative one raises ValueError"""
    r = float(rmax)
    if not r >= 0.0:   # (NaN too)
        raise ValueError("distance field: rmax must be >= 0")
    return r


def _grid(origin, cell, dims):
    """a psm_grid from origin [3], cell (a scalar or [3]) and dims [3], refused here by the rules of psm_hip.h "voxel grids" (no
    call is made for an invalid grid: ValueError)"""
    o = np.asarray(origin, np.float64).reshape(-1)
    c = np.asarray(cell, np.float64).reshape(-1)
    d = np.asarray(dims).reshape(-1)
    if c.size == 1:
        c = np.repeat(c, 3)
    if o.size != 3 or c.size != 3 or d.size != 3:
        raise ValueError("voxel grid: origin and dims take 3 numbers, cell 1 or 3")
    with np.errstate(over="ignore"):
        o, c = o.astype(np.float32), c.astype(np.float32)
    if not np.isfinite(o).all():
        raise ValueError("voxel grid: origin is not finite")
    if not (np.isfinite(c) & (c > 0)).all():
        raise ValueError("voxel grid: cell must be finite and > 0")
    if any(int(x) != x or not 1 <= int(x) <= GRID_DIM_MAX for x in d.tolist()):
        raise ValueError("voxel grid: dims must be whole numbers in 1 .. 2^20")
    d = d.astype(np.int64)
    with np.errstate(over="ignore"):
        top = o + d.astype(np.float32) * c   # (the last voxel's hi: one float32 product, then one float32 sum)
    if not np.isfinite(top).all():
        raise ValueError("voxel grid: the last voxel's hi is not finite")
    nb = (d + 3) // 4
    if int(nb[0]) * int(nb[1]) * int(nb[2]) >= 1 << 31:
        raise ValueError("voxel grid: 2^31 bricks or more")
    g = Grid()
    g.origin[:], g.cell[:], g.dims[:] = o.tolist(), c.tolist(), [int(x) for x in d]
    return g


def voxel_boxes(origin, cell, dims):
    """The boxes of a grid's voxels, (lo, hi) float32 [nz * ny * nx, 3] with voxel (ix, iy, iz) in row (iz * ny + iy) * nx + ix:
    per axis k, lo_k = origin_k + float32(i_k) * cell_k and hi_k = origin_k + float32(i_k + 1) * cell_k, each one float32
    product and then one float32 sum (psm_hip.h "voxel grids"). hi of voxel i is lo of voxel i + 1 bit for bit. This is the
    public statement of the voxel box: voxelize() and voxelCounts() answer boxOverlaps() and boxCount() of these boxes."""
    g = _grid(origin, cell, dims)
    o, c = np.array(g.origin, np.float32), np.array(g.cell, np.float32)
    planes = [(o[k] + np.arange(g.dims[k] + 1, dtype=np.float32) * c[k]).astype(np.float32) for k in range(3)]
    iz, iy, ix = np.meshgrid(np.arange(g.dims[2]), np.arange(g.dims[1]), np.arange(g.dims[0]), indexing="ij")
    ix, iy, iz = ix.reshape(-1), iy.reshape(-1), iz.reshape(-1)
    lo = np.stack([planes[0][ix], planes[1][iy], planes[2][iz]], axis=1)
    hi = np.stack([planes[0][ix + 1], planes[1][iy + 1], planes[2][iz + 1]], axis=1)
    return lo, hi


def voxel_centres(origin, cell, dims):
    """The centres of a grid's voxels, float32 [nz * ny * nx, 3] in voxel_boxes()'s order: c_k = origin_k + (float32(i_k) + 0.5) *
    cell_k in float32: the points voxelize(solid=True) asks inside() about."""
    g = _grid(origin, cell, dims)
    o, c = np.array(g.origin, np.float32), np.array(g.cell, np.float32)
    mids = [(o[k] + (np.arange(g.dims[k], dtype=np.float32) + np.float32(0.5)) * c[k]).astype(np.float32) for k in range(3)]
    iz, iy, ix = np.meshgrid(np.arange(g.dims[2]), np.arange(g.dims[1]), np.arange(g.dims[0]), indexing="ij")
    return np.stack([mids[0][ix.reshape(-1)], mids[1][iy.reshape(-1)], mids[2][iz.reshape(-1)]], axis=1)


class VoxelGrid:
    """What TriangleHierarchy.voxelize returns. bricks: [nbz, nby, nbx], nb = ceil(dims / 4), one 64-bit word per 4 x 4 x 4 brick
    (a uint64 array; for torch an int64 tensor holding the same bits): bit (z & 3) * 16 + (y & 3) * 4 + (x & 3) of brick (x // 4,
    y // 4, z // 4) is voxel (x, y, z), and the bits of voxels outside dims are 0. dims = (nx, ny, nz), origin and cell as given
    (float32 values)."""

    def __init__(self, bricks, dims, origin, cell):
        self.bricks, self.dims, self.origin, self.cell = bricks, dims, origin, cell

    def dense(self):
        """bool [nz, ny, nx] (a numpy array, or a torch bool tensor on the bricks' device)"""
        nx, ny, nz = self.dims
        nbz, nby, nbx = self.bricks.shape
        if isinstance(self.bricks, np.ndarray):
            bits = (self.bricks[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
            cube = bits.astype(np.bool_).reshape(nbz, nby, nbx, 4, 4, 4).transpose(0, 3, 1, 4, 2, 5)
            return np.ascontiguousarray(cube.reshape(4 * nbz, 4 * nby, 4 * nbx)[:nz, :ny, :nx])
        import torch
        bits = (self.bricks[..., None] >> torch.arange(64, dtype=torch.int64, device=self.bricks.device)) & 1   # (bit 63: the sign's copies are masked off)
        cube = bits.to(torch.bool).reshape(nbz, nby, nbx, 4, 4, 4).permute(0, 3, 1, 4, 2, 5)
        return cube.reshape(4 * nbz, 4 * nby, 4 * nbx)[:nz, :ny, :nx].contiguous()

    def occupied(self):
        """the number of voxels set: the sum of the words' popcounts"""
        words = self.bricks if isinstance(self.bricks, np.ndarray) else self.bricks.cpu().numpy().view(np.uint64)
        return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum(dtype=np.int64))


class DistanceGrid:
    """What TriangleHierarchy.distanceField and InstanceWorld.distanceField return. dist: float32 [nz, ny, nx], the (signed)
    distance at each voxel centre, +inf where no triangle lies within rmax; tri: int32 [nz, ny, nx], the nearest triangle's id, -1
    where dist is +inf, or None when the ids were not asked for (numpy arrays, or torch tensors on the context's device). dims =
    (nx, ny, nz), origin and cell as given (float32 values). inst: for an InstanceWorld's field the int32 [nz, ny, nx] instance
    of each voxel's nearest triangle (tri is that instance's id), -1 where dist is +inf, None with tri; None for a single
    hierarchy's field."""

    def __init__(self, dist, tri, dims, origin, cell, inst=None):
        self.dist, self.tri, self.dims, self.origin, self.cell, self.inst = dist, tri, dims, origin, cell, inst


def _brick_shape(dims):
    """(nbz, nby, nbx) of a grid of dims = (nx, ny, nz)"""
    return tuple((int(d) + 3) // 4 for d in reversed(dims))


def _brick_scatter(ids, rows, shape, fill):
    """rows [n, ...] of the bricks ids into an array / tensor [nbz * nby * nbx, ...] of `fill`; an id at or above the brick
    count names no brick and is left out"""
    total = shape[0] * shape[1] * shape[2]
    if isinstance(rows, np.ndarray):
        at = np.asarray(ids).astype(np.int64)
        out = np.full((total,) + rows.shape[1:], fill, rows.dtype)
        out[at[at < total]] = rows[at < total]
        return out
    import torch
    at = ids.to(torch.int64) & 0xFFFFFFFF   # (an int32 tensor holds the uint32 bits)
    out = torch.full((total,) + tuple(rows.shape[1:]), fill, dtype=rows.dtype, device=rows.device)
    out[at[at < total]] = rows[at < total]
    return out


class _SparseGrid:
    def coords(self):
        """(bx, by, bz) of each listed brick, int64 [n, 3] (numpy, or a tensor on the ids' device)"""
        nbz, nby, nbx = _brick_shape(self.dims)
        if isinstance(self.ids, np.ndarray):
            b = self.ids.astype(np.int64)
            return np.stack([b % nbx, (b // nbx) % nby, b // (nbx * nby)], axis=1)
        import torch
        b = self.ids.to(torch.int64) & 0xFFFFFFFF
        return torch.stack([b % nbx, torch.div(b, nbx, rounding_mode="floor") % nby, torch.div(b, nbx * nby, rounding_mode="floor")], dim=1)

    def __len__(self):
        return int(self.ids.shape[0])


class SparseVoxelGrid(_SparseGrid):
    """What TriangleHierarchy.sparseVoxelize returns. ids: uint32 [n], the brick indices (bz * nby + by) * nbx + bx, ascending
    when the call listed them; words: uint64 [n], VoxelGrid's word of brick ids[i] (torch: int32 / int64 tensors holding the same
    bits). dims = (nx, ny, nz), origin and cell as given (float32 values). coords(): (bx, by, bz) per brick; dense(): the
    VoxelGrid with these words and 0 elsewhere."""

    def __init__(self, ids, words, dims, origin, cell):
        self.ids, self.words, self.dims, self.origin, self.cell = ids, words, dims, origin, cell

    def dense(self):
        shape = _brick_shape(self.dims)
        return VoxelGrid(_brick_scatter(self.ids, self.words, shape, 0).reshape(shape), self.dims, self.origin, self.cell)


class SparseDistanceGrid(_SparseGrid):
    """What TriangleHierarchy.sparseDistanceField returns. ids: uint32 [n] as SparseVoxelGrid's; dist: float32 [n, 4, 4, 4], axes
    (z, y, x) within the brick, the (signed) distance at each voxel centre of brick ids[i], +inf where no triangle lies within
    rmax and for a voxel outside dims; tri: int32 [n, 4, 4, 4], the nearest triangle, -1 where dist is +inf, or None when the ids
    were not asked for. coords(): (bx, by, bz) per brick; dense(): the DistanceGrid [nz, ny, nx] with these bricks and +inf / -1
    elsewhere."""

    def __init__(self, ids, dist, tri, dims, origin, cell):
        self.ids, self.dist, self.tri, self.dims, self.origin, self.cell = ids, dist, tri, dims, origin, cell

    def dense(self):
        nx, ny, nz = self.dims
        shape = _brick_shape(self.dims)

        def cube(rows, fill):
            c = _brick_scatter(self.ids, rows, shape, fill).reshape(shape + (4, 4, 4))
            c = c.transpose(0, 3, 1, 4, 2, 5) if isinstance(c, np.ndarray) else c.permute(0, 3, 1, 4, 2, 5)
            c = c.reshape(4 * shape[0], 4 * shape[1], 4 * shape[2])[:nz, :ny, :nx]
            return np.ascontiguousarray(c) if isinstance(c, np.ndarray) else c.contiguous()

        return DistanceGrid(cube(self.dist, np.inf), None if self.tri is None else cube(self.tri, -1), self.dims, self.origin, self.cell)


class QueryHitLists:
    """The rows of TriangleHierarchy.firstHits / .nearest and InstanceWorld.firstHits / .nearest: `buffer` [n, k, 4] float32 (numpy
    array or torch tensor) holds psm_hit records (u, v, t, tri); u, v, t and tri (int32) [n, k] are views of it. count [n]: the
    slots of a row that hold a record (uint32; an int32 tensor for torch), the rest are misses (tri = -1, t = +inf). geom: for an
    InstanceWorld's rows the int32 [n, k] array / tensor of each slot's instance (-1 in a miss slot; tri is that instance's id);
    None for a single hierarchy's."""

    def __init__(self, buffer, count, geom=None):
        self.buffer = buffer
        self.count = count
        self.geom = geom
        self.u, self.v, self.t = buffer[:, :, 0], buffer[:, :, 1], buffer[:, :, 2]
        if isinstance(buffer, np.ndarray):
            self.tri = buffer.view(np.int32)[:, :, 3]
        else:
            import torch
            self.tri = buffer.view(torch.int32)[:, :, 3]

    def __len__(self):
        return self.buffer.shape[0]


class QueryTriLists:
    """The rows of TriangleHierarchy.boxTriangles and .triTriangles: tri [n, k] int32 (numpy array or torch tensor), the lowest triangle ids that
    overlap the box (meet the query triangle), ascending, -1 in the slots past count; count [n] (uint32; an int32 tensor for torch). geom: for the rows of
    InstanceWorld.trianglesInBox the int32 [n, k] array / tensor of each slot's instance (-1 past count; tri is that instance's
    id; the rows ascend in (geom, tri)); None for a single hierarchy's."""

    def __init__(self, tri, count, geom=None):
        self.tri = tri
        self.count = count
        self.geom = geom

    def __len__(self):
        return self.tri.shape[0]


class QueryTriHits:
    """The records of TriangleHierarchy.triClosest and InstanceWorld.closestToTriangle: `buffer` [n, 8] float32 (numpy array or
    torch tensor) holds psm_tri_hit records (u, v, dist, tri, s, t, 0, 0); u, v, dist, tri (int32), s and t are views of it.
    (u, v) weigh e1, e2 of the stored triangle `tri`, (s, t) weigh b - a, c - a of the query triangle; a miss is tri = -1,
    dist = +inf. geom: for an InstanceWorld's records the int32 array / tensor of the winning instance's index (-1 on a miss, tri
    is that instance's id); None for a single hierarchy's. InstanceWorld.closestToMesh's records are [p, T, 8] with geom [p, T]:
    the views are on the last axis (points() and points_world() take the flat [n, 8] records)."""

    def __init__(self, buffer, geom=None):
        self.buffer = buffer
        self.geom = geom
        self.u, self.v, self.dist = buffer[..., 0], buffer[..., 1], buffer[..., 2]
        self.s, self.t = buffer[..., 4], buffer[..., 5]
        if isinstance(buffer, np.ndarray):
            self.tri = buffer.view(np.int32)[..., 3]
        else:
            import torch
            self.tri = buffer.view(torch.int32)[..., 3]

    def __len__(self):
        return self.buffer.shape[0]

    def points(self, mesh_tris, query_tris):
        """the two nearest points in world space, [n, 3] each: (v0 + u e1) + v e2 on the mesh's triangle `tri` (mesh_tris
        [T, 3, 3], the triangles as loaded) and (a + s (b - a)) + t (c - a) on the query triangle; a miss gives NaN rows"""
        u, v, s, t = self.u[:, None], self.v[:, None], self.s[:, None], self.t[:, None]
        ids = self.tri.clip(0) if isinstance(self.buffer, np.ndarray) else self.tri.clip(0).long()
        m = mesh_tris.reshape(-1, 3, 3)[ids]
        q = query_tris.reshape(-1, 3, 3)
        on_mesh = (m[:, 0] + u * (m[:, 1] - m[:, 0])) + v * (m[:, 2] - m[:, 0])
        on_query = (q[:, 0] + s * (q[:, 1] - q[:, 0])) + t * (q[:, 2] - q[:, 0])
        miss = (self.tri < 0)[:, None]
        return on_mesh + _nan_where(miss, on_mesh), on_query + _nan_where(miss, on_query)

    def points_world(self, world_tris_of_instances, query_tris):
        """points() for the records of InstanceWorld.closestToTriangle: world_tris_of_instances[j] holds instance j's triangles
        AS POSED, [T_j, 3, 3] in world space (its loaded triangles moved by its pose: R x + T per vertex); the point on the
        world is (v0' + u e1') + v e2' on triangle `tri` of instance `geom`. numpy arrays, [n, 3] each; a miss gives NaN rows"""
        if self.geom is None:
            raise ValueError("points_world(): the records of InstanceWorld.closestToTriangle have an instance; use points()")
        rec = self.buffer if isinstance(self.buffer, np.ndarray) else self.buffer.cpu().numpy()
        geom = self.geom if isinstance(self.geom, np.ndarray) else self.geom.cpu().numpy()
        tri = rec.view(np.int32)[:, 3]
        q = np.asarray(query_tris, np.float32).reshape(-1, 3, 3)
        m = np.full((rec.shape[0], 3, 3), np.nan, np.float32)
        for j in np.unique(geom[geom >= 0]):
            rows = geom == j
            m[rows] = np.asarray(world_tris_of_instances[j], np.float32).reshape(-1, 3, 3)[tri[rows]]
        u, v, s, t = (rec[:, k:k + 1] for k in (0, 1, 4, 5))
        on_world = (m[:, 0] + u * (m[:, 1] - m[:, 0])) + v * (m[:, 2] - m[:, 0])
        on_query = (q[:, 0] + s * (q[:, 1] - q[:, 0])) + t * (q[:, 2] - q[:, 0])
        on_query[tri < 0] = np.nan
        return on_world, on_query


class QueryMeshHits:
    """The records of TriangleHierarchy.meshClosest ([p, T, 8]) and .meshClearance ([p, 8]): `buffer`, float32 (numpy array or
    torch tensor), holds psm_tri_hit / psm_mesh_hit records; u, v, dist, tri (int32), s and t are views on its last axis.
    (u, v) weigh e1, e2 of this hierarchy's triangle `tri`, (s, t) weigh b - a, c - a of the posed triangle of the other mesh.
    other: for meshClearance the int32 view of slot 6, the other mesh's triangle (-1 on a miss); None for meshClosest, whose
    second index is that triangle. QueryTriHits stays what triClosest returns. geom: for InstanceWorld.clearanceToMesh's records
    the int32 array / tensor [p] of the winning instance (-1 on a miss; tri is that instance's id); None for a hierarchy's."""

    def __init__(self, buffer, per_pose=False, geom=None):
        self.buffer = buffer
        self.geom = geom
        self.u, self.v, self.dist = buffer[..., 0], buffer[..., 1], buffer[..., 2]
        self.s, self.t = buffer[..., 4], buffer[..., 5]
        if isinstance(buffer, np.ndarray):
            ints = buffer.view(np.int32)
        else:
            import torch
            ints = buffer.view(torch.int32)
        self.tri = ints[..., 3]
        self.other = ints[..., 6] if per_pose else None

    def __len__(self):
        return self.buffer.shape[0]

    def points(self, mesh_tris, other_tris, poses):
        """meshClearance's two witness points in this hierarchy's space, [p, 3] each: (v0 + u e1) + v e2 on this hierarchy's
        triangle `tri` (mesh_tris [T', 3, 3], the triangles as loaded) and (a + s (b - a)) + t (c - a) on the other mesh's
        triangle `other` (other_tris [T, 3, 3], as loaded) moved by its pose (poses [p, 3, 4] / [p, 4, 4]; float64 here, not
        the device's float32 image); a miss gives NaN rows. numpy arrays."""
        if self.other is None:
            raise ValueError("points(): the records of meshClearance have them; meshClosest's are per (pose, triangle)")
        rec = self.buffer if isinstance(self.buffer, np.ndarray) else self.buffer.cpu().numpy()
        ids = rec.view(np.int32)
        miss = ids[:, 3] < 0
        m = np.asarray(mesh_tris, np.float64).reshape(-1, 3, 3)[ids[:, 3].clip(0)] if len(rec) else np.zeros((0, 3, 3))
        o = np.asarray(other_tris, np.float64).reshape(-1, 3, 3)[ids[:, 6].clip(0)] if len(rec) else np.zeros((0, 3, 3))
        pm = np.asarray(poses, np.float64)
        pm = (pm[None] if pm.ndim == 2 else pm)[:, :3, :]
        o = np.einsum("pij,pkj->pki", pm[:, :, :3], o) + pm[:, None, :, 3]
        u, v, s, t = (rec[:, k:k + 1].astype(np.float64) for k in (0, 1, 4, 5))
        on_mesh = (m[:, 0] + u * (m[:, 1] - m[:, 0])) + v * (m[:, 2] - m[:, 0])
        on_other = (o[:, 0] + s * (o[:, 1] - o[:, 0])) + t * (o[:, 2] - o[:, 0])
        on_mesh[miss] = np.nan
        on_other[miss] = np.nan
        return on_mesh, on_other


    def points_world(self, world_tris_of_instances, other_tris, poses):
        """points() for the records of InstanceWorld.clearanceToMesh, in world space, [p, 3] each: the point on triangle `tri` of
        instance `geom` (world_tris_of_instances[j]: instance j's triangles AS POSED, as QueryTriHits.points_world takes them)
        and the point on the other mesh's triangle `other` moved by its pose (float32 here); a miss gives NaN rows"""
        if self.other is None or self.geom is None:
            raise ValueError("points_world(): the records of InstanceWorld.clearanceToMesh have an instance and a triangle of other")
        rec = self.buffer if isinstance(self.buffer, np.ndarray) else self.buffer.cpu().numpy()
        o = np.asarray(other_tris, np.float32).reshape(-1, 3, 3)[rec.view(np.int32)[:, 6].clip(0)] if len(rec) else np.zeros((0, 3, 3), np.float32)
        pm = np.asarray(poses, np.float32)
        pm = (pm[None] if pm.ndim == 2 else pm)[:, :3, :]
        posed = np.einsum("pij,pkj->pki", pm[:, :, :3], o) + pm[:, None, :, 3]
        return QueryTriHits(rec, self.geom).points_world(world_tris_of_instances, posed)


def _mesh_poses(other, poses, name):
    """the poses of a mesh query checked and packed [p, 12] float32 on the host; with them p and other's triangle count"""
    if not isinstance(other, TriangleHierarchy):
        raise TypeError("%s: other must be a TriangleHierarchy" % name)
    m = np.asarray(poses)
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3:
        raise ValueError("%s: poses must be one matrix or [p, 3, 4] / [p, 4, 4]" % name)
    p = m.shape[0]
    m12 = np.ascontiguousarray(np.stack([_pose(x, name) for x in m]).reshape(p, 12) if p else np.zeros((0, 12)), np.float32)
    return m12, p, int(other.triangleCount)


def _nan_where(mask, like):
    """an array / tensor shaped as `like`: NaN where mask, else 0"""
    if isinstance(like, np.ndarray):
        return np.where(mask, np.float32(np.nan), np.float32(0)) * np.ones_like(like)
    import torch
    return torch.where(mask, torch.full_like(like, float("nan")), torch.zeros_like(like))


class QueryHits:
    """Closest hits of TriangleHierarchy.intersect (closest points of .closestPoint and .signedDistance: t is the distance): `buffer` [n, 4] float32 (numpy array or torch tensor) holds psm_hit records
    (u, v, t, tri); t, u, v and tri (int32) are views of it. geom: for a QueryScene's results the int32 array / tensor of the
    winning geometry's index in the scene (-1 on a miss, tri is that geometry's id); None for a single hierarchy's."""

    def __init__(self, buffer, geom=None):
        self.buffer = buffer
        self.geom = geom
        self.u, self.v, self.t = buffer[:, 0], buffer[:, 1], buffer[:, 2]
        if isinstance(buffer, np.ndarray):
            self.tri = buffer.view(np.int32)[:, 3]
        else:
            import torch
            self.tri = buffer.view(torch.int32)[:, 3]

    def __len__(self):
        return self.buffer.shape[0]


def _launch_np(th, packed, out, name, *extra):
    """one query launch of `th` (a TriangleHierarchy or a QueryScene) over host records `packed` [n, k] float32: staged through
    device buffers, synchronises. out: the result's kind (_QUERY_OUT); extra: arguments between n and the output pointer"""
    ctx = th.ctx
    n = packed.shape[0]
    per, dtype = _QUERY_OUT[out]
    tris = out == "tris"     # (a box query's id rows: k slots per query and the counts, as the lists')
    lists = out == "lists"   # (k rows per query, and the counts travel where a scene's geometry indices do)
    k = extra[0].value if lists or tris else 1
    geom = (th._scene and out in ("hits", "trihits")) or lists or tris   # (a world's clearance records carry the instance too)
    hr, ho = ctx.buf_alloc(max(packed.nbytes, 32)), ctx.buf_alloc(max(per * k * n, 16))
    hg = ctx.buf_alloc(max(4 * n, 16)) if geom else None
    hi = ctx.buf_alloc(max(4 * k * n, 16)) if (lists or tris) and th._scene else None   # (a world's rows: the instance of every slot)
    try:
        if n:
            ctx.buf_upload(hr, packed)
        d_geom = ctx.buf_ptr(hg)[0] if geom else None
        th._call(name, ctx.buf_ptr(hr)[0], n, extra, ctx.buf_ptr(ho)[0], d_geom if hi is None else (ctx.buf_ptr(hi)[0], d_geom))
        if n == 0:
            ctx.sync()
            if lists:
                return QueryHitLists(np.zeros((0, k, 4), np.float32), np.zeros(0, np.uint32), None if hi is None else np.zeros((0, k), np.int32))
            if tris:
                return QueryTriLists(np.zeros((0, k), np.int32), np.zeros(0, np.uint32), None if hi is None else np.zeros((0, k), np.int32))
            if out == "hits":
                return QueryHits(np.zeros((0, 4), np.float32), np.zeros(0, np.int32) if geom else None)
            if out == "trihits":
                return QueryTriHits(np.zeros((0, 8), np.float32), np.zeros(0, np.int32) if geom else None)
            return np.zeros(0, dtype)
        if out == "bool":
            return ctx.buf_download(ho, np.uint8, n).view(np.bool_)
        if out == "count":
            return ctx.buf_download(ho, np.uint32, n)
        if out == "trihits":
            return QueryTriHits(ctx.buf_download(ho, np.float32, 8 * n).reshape(n, 8), ctx.buf_download(hg, np.int32, n) if geom else None)
        if tris:
            return QueryTriLists(ctx.buf_download(ho, np.int32, k * n).reshape(n, k), ctx.buf_download(hg, np.uint32, n),
                                 None if hi is None else ctx.buf_download(hi, np.int32, k * n).reshape(n, k))
        if lists:
            return QueryHitLists(ctx.buf_download(ho, np.float32, 4 * k * n).reshape(n, k, 4), ctx.buf_download(hg, np.uint32, n),
                                 None if hi is None else ctx.buf_download(hi, np.int32, k * n).reshape(n, k))
        return QueryHits(ctx.buf_download(ho, np.float32, 4 * n).reshape(n, 4), ctx.buf_download(hg, np.int32, n) if geom else None)
    finally:
        ctx.buf_free(hr)
        ctx.buf_free(ho)
        if geom:
            ctx.buf_free(hg)
        if hi is not None:
            ctx.buf_free(hi)


_hip_lib = None


def _hip():
    """The HIP runtime libpsm_hip.so runs on (loaded once per process; torch's streams and events are its handles). torch's own
    cross-stream waits reject a stream it did not create (ExternalStream), so the two waits of _query_torch are made here."""
    global _hip_lib
    if _hip_lib is None:
        lib()
        _hip_lib = C.CDLL("libamdhip64.so.7", mode=C.RTLD_GLOBAL)
    return _hip_lib


def _hip_check(rc, what):
    if rc != 0:
        raise PsmError("%s failed (%d)" % (what, rc))


def _query_torch(th, origins, directions, tmin, tmax, out, name, *extra):
    """TriangleHierarchy.intersect / occluded on torch device tensors: rays packed on torch's current stream, the kernel on the
    context's stream, the two ordered by events when they differ -- no host synchronisation."""
    import torch
    dev = origins.device
    if dev.type != "cuda" or directions.device != dev:
        raise ValueError("%s: origins and directions must be tensors on the context's device"
                         % ("sweepSphere / sweepOccluded" if "sweep" in name else "intersect / occluded"))
    o = origins.reshape(-1, 3)
    d = directions.reshape(-1, 3)
    n = o.shape[0]
    if d.shape[0] != n:
        raise ValueError("origins and directions: %d against %d rays" % (n, d.shape[0]))
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    rays[:, 0:3] = o
    rays[:, 3] = torch.as_tensor(tmin, dtype=torch.float32, device=dev)
    rays[:, 4:7] = d
    rays[:, 7] = torch.as_tensor(tmax, dtype=torch.float32, device=dev)
    return _launch_torch(th, rays, out, name, *extra)


def _torch_ordered(ctx, dev, call):
    """call() -- launches on the context's stream -- between what torch's current stream of `dev` has queued and what it queues
    next: the two streams ordered by events when they differ, no host synchronisation."""
    import torch
    cur = torch.cuda.current_stream(dev)
    mine = ctx.stream or 0   # (NULL: the device's null stream, torch's default stream)
    other = mine != cur.cuda_stream
    if other:   # the context's stream waits for the packing (torch's event, HIP's wait: no host synchronisation)
        ev_in = torch.cuda.Event()
        ev_in.record(cur)
        _hip_check(_hip().hipStreamWaitEvent(C.c_void_p(mine), C.c_void_p(ev_in.cuda_event), C.c_uint(0)), "hipStreamWaitEvent")
    call()
    if other:   # ... and torch's stream for the kernel: every later use of the outputs, and of the inputs' memory, comes after it
        hip, ev = _hip(), C.c_void_p()
        _hip_check(hip.hipEventCreateWithFlags(C.byref(ev), C.c_uint(2)), "hipEventCreateWithFlags")   # hipEventDisableTiming
        _hip_check(hip.hipEventRecord(ev, C.c_void_p(mine)), "hipEventRecord")
        _hip_check(hip.hipStreamWaitEvent(C.c_void_p(cur.cuda_stream), ev, C.c_uint(0)), "hipStreamWaitEvent")
        _hip_check(hip.hipEventDestroy(ev), "hipEventDestroy")


_TORCH_OF = {np.uint8: "uint8", np.int32: "int32", np.uint32: "int32", np.uint64: "int64", np.float32: "float32"}   # (torch has no general uint32 / uint64)


def _device_call(ctx, call, outs, as_torch):
    """One native call that writes device outputs, outs a list of (shape, numpy dtype): call(*pointers), one per output in
    order. as_torch: the outputs are torch tensors on the context's device and the call runs under _torch_ordered; else they are
    staged in the context's buffers, read back (an empty one is not) and freed. Returns the tensors / arrays in order."""
    if as_torch:
        import torch
        dev = torch.device("cuda", ctx.device)
        res = [torch.empty(shape, dtype=getattr(torch, _TORCH_OF[dtype]), device=dev) for shape, dtype in outs]
        _torch_ordered(ctx, dev, lambda: call(*[r.data_ptr() for r in res]))
        return res
    bufs = []
    try:
        for shape, dtype in outs:
            bufs.append(ctx.buf_alloc(max(int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize, 16)))
        call(*[ctx.buf_ptr(h)[0] for h in bufs])
        res = []
        for h, (shape, dtype) in zip(bufs, outs):
            n = int(np.prod(shape, dtype=np.int64))
            res.append((ctx.buf_download(h, dtype, n) if n else np.zeros(0, dtype)).reshape(shape))
        return res
    finally:
        for h in bufs:
            ctx.buf_free(h)


def _voxel_call(ctx, handle, prefix, what, g, dtype, as_torch, samples=None, fresh=None):
    """One voxel grid call of a hierarchy ("psm_grid_") or a world ("psm_grid_world_"), what: surface, solid (with samples),
    counts or instances. g: the Grid (_grid()'s: an invalid one has raised ValueError before); fresh(name): the owner's check
    before the library sees the handle. uint64: the bricks as a VoxelGrid; else the dense [nz, ny, nx] array / tensor."""
    name = prefix + what + "_dev"
    extra = () if samples is None else (C.c_uint32(_samples(samples, name)),)
    if fresh:
        fresh(name)
    fn = getattr(lib(), name)
    words = dtype is np.uint64
    shape = tuple((int(d) + 3) // 4 if words else int(d) for d in reversed(g.dims))

    def call(d_out):
        ctx.check(fn(handle, C.byref(g), *extra, C.c_void_p(d_out)), name)

    out = _device_call(ctx, call, [(shape, dtype)], as_torch)[0]
    return VoxelGrid(out, tuple(g.dims), tuple(g.origin), tuple(g.cell)) if words else out


def _distance_call(ctx, handle, prefix, g, r, signed, samples, nearest, as_torch, inst=False, fresh=None):
    """One distance-field call of a hierarchy or a world (prefix, g and fresh as _voxel_call's; r: _rmax()'s): dist, with nearest
    tri and, where the call has an instance output, inst behind it; an output not asked for is passed as NULL. Returns DistanceGrid."""
    name = prefix + ("signed_distance_dev" if signed else "distance_dev")
    extra = (C.c_float(r), C.c_uint32(_samples(samples, name))) if signed else (C.c_float(r),)
    if fresh:
        fresh(name)
    fn = getattr(lib(), name)
    shape = (g.dims[2], g.dims[1], g.dims[0])
    ids = 2 if inst else 1   # (the outputs behind dist)

    def call(*ptrs):
        ptrs += (None,) * (1 + ids - len(ptrs))
        ctx.check(fn(handle, C.byref(g), *extra, *[C.c_void_p(p) for p in ptrs]), name)

    outs = _device_call(ctx, call, [(shape, np.float32)] + ([(shape, np.int32)] * ids if nearest else []), as_torch)
    outs += [None] * (3 - len(outs))
    return DistanceGrid(outs[0], outs[1], tuple(g.dims), tuple(g.origin), tuple(g.cell), outs[2])


def _sparse_call(ctx, handle, g, r, signed, samples, nearest, bricks, as_torch):
    """One sparse grid call of a hierarchy: r None -- the surface (SparseVoxelGrid) --, else the distance field with band r
    (_rmax()'s), signed with samples, tri stored iff nearest (SparseDistanceGrid). bricks None: the count (the one
    synchronisation), then the list into an exact-size array and the fill, in one _device_call; bricks given: the fill alone."""
    surface = r is None
    lister = "psm_grid_sparse_surface_bricks_dev" if surface else "psm_grid_sparse_distance_bricks_dev"
    filler = "psm_grid_sparse_surface_dev" if surface else ("psm_grid_sparse_signed_distance_dev" if signed else "psm_grid_sparse_distance_dev")
    band = () if surface else (C.c_float(r),)
    extra = band + ((C.c_uint32(_samples(samples, filler)),) if signed and not surface else ())
    list_fn, fill_fn = getattr(lib(), lister), getattr(lib(), filler)
    dims, origin, cell = tuple(g.dims), tuple(g.origin), tuple(g.cell)

    def result(ids, outs):
        n = ids.shape[0]
        if surface:
            return SparseVoxelGrid(ids, outs[0], dims, origin, cell)
        return SparseDistanceGrid(ids, outs[0].reshape(n, 4, 4, 4), outs[1].reshape(n, 4, 4, 4) if nearest else None, dims, origin, cell)

    def fills(n):
        return [((n,), np.uint64)] if surface else [((n, 64), np.float32)] + ([((n, 64), np.int32)] if nearest else [])

    def fill(p_ids, n, ptrs):
        if n:   # (an empty list asks nothing, and an empty array may have no address)
            ptrs = tuple(ptrs) + (None,) * ((1 if surface else 2) - len(ptrs))
            ctx.check(fill_fn(handle, C.byref(g), *extra, C.c_void_p(p_ids), C.c_uint32(n), *[C.c_void_p(p) for p in ptrs]), filler)

    if bricks is None:
        def count(p_count):
            ctx.check(list_fn(handle, C.byref(g), *band, C.c_uint32(0), None, C.c_void_p(p_count)), lister)

        n = int(_device_call(ctx, count, [((1,), np.uint32)], False)[0][0])

        def call(p_ids, p_count, *ptrs):
            ctx.check(list_fn(handle, C.byref(g), *band, C.c_uint32(n), C.c_void_p(p_ids) if n else None, C.c_void_p(p_count)), lister)
            fill(p_ids, n, ptrs)

        outs = _device_call(ctx, call, [((n,), np.uint32), ((1,), np.uint32)] + fills(n), as_torch)
        return result(outs[0], outs[2:])
    if type(bricks).__module__.split(".")[0] == "torch":
        import torch
        if bricks.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
            raise ValueError("sparse grid: bricks must hold uint32 brick indices")
        ids = bricks.reshape(-1).contiguous() if as_torch else bricks.detach().cpu().numpy().view(np.uint32).reshape(-1)
    else:
        ids = np.ascontiguousarray(bricks)
        if ids.dtype != np.uint32:
            if ids.size and (not np.issubdtype(ids.dtype, np.integer) or ids.min() < 0 or ids.max() >= 1 << 32):
                raise ValueError("sparse grid: bricks must hold uint32 brick indices")
            ids = ids.astype(np.uint32)
        ids = ids.reshape(-1)
    n = int(ids.shape[0])
    if n >= 1 << 32:
        raise ValueError("sparse grid: 2^32 bricks or more")
    if as_torch:
        import torch
        dev = torch.device("cuda", ctx.device)
        if isinstance(ids, np.ndarray):
            ids = torch.from_numpy(ids.view(np.int32)).to(dev)
        elif ids.device != dev:
            raise ValueError("sparse grid: bricks must be a tensor on the context's device")
        return result(ids, _device_call(ctx, lambda *ptrs: fill(ids.data_ptr(), n, ptrs), fills(n), True))
    h = ctx.buf_alloc(max(4 * n, 16))
    try:
        if n:
            ctx.buf_upload(h, ids)
        return result(ids, _device_call(ctx, lambda *ptrs: fill(ctx.buf_ptr(h)[0], n, ptrs), fills(n), False))
    finally:
        ctx.buf_free(h)


def _bool_view(flags):
    """a uint8 array / tensor of 0 / 1 as bools, the same memory"""
    if isinstance(flags, np.ndarray):
        return flags.view(np.bool_)
    import torch
    return flags.view(torch.bool)


def _mesh_outs(out, p, t, k, world):
    """the output spec of a mesh query: the flags [p], the counts [p, T], or the rows [p, T, k] (a world's twice: the
    instances) and the counts"""
    if out == "bool":
        return [((p,), np.uint8)]
    if out == "count":
        return [((p, t), np.uint32)]
    return [((p, t, k), np.int32)] * (2 if world else 1) + [((p, t), np.uint32)]


def _mesh_dist_outs(out, p, t, world):
    """the output spec of a mesh clearance query: the flags [p], or the records [p, T, 8] / [p, 8] and a world's instances"""
    if out == "bool":
        return [((p,), np.uint8)]
    shape = (p, t, 8) if out == "closest" else (p, 8)
    return [(shape, np.float32)] + ([(shape[:-1], np.int32)] if world else [])


def _mesh_skip(world, skip, name):
    """a world's skip argument as the library takes it: -1 for None, else an instance index (refused here: no call is made)"""
    if skip is None:
        return -1
    s = int(skip)
    if s != skip or isinstance(skip, bool) or not 0 <= s < len(world.hierarchies):
        raise PsmError("%s: skip must be None or an instance index 0 .. %d" % (name, len(world.hierarchies) - 1))
    return s


def _launch_torch(th, packed, kind, name, *extra):
    """One query launch over device records `packed` (made on torch's current stream) on the context's stream: the two streams
    ordered by events when they differ -- no host synchronisation. kind: the result's (_QUERY_OUT): QueryHits, a bool or an int32
    count per query; extra: arguments between n and the output pointer."""
    import torch
    dev = packed.device
    n = packed.shape[0]
    lists, tris = kind == "lists", kind == "tris"
    shape, dtype = {"trihits": ((n, 8), torch.float32), "hits": ((n, 4), torch.float32), "bool": ((n,), torch.uint8), "count": ((n,), torch.int32),
                    "lists": ((n, extra[0].value if lists else 1, 4), torch.float32),
                    "tris": ((n, extra[0].value if tris else 1), torch.int32)}[kind]
    out = torch.empty(shape, dtype=dtype, device=dev)
    geom = torch.empty((n,), dtype=torch.int32, device=dev) if (th._scene and kind in ("hits", "trihits")) or lists or tris else None
    inst = torch.empty(shape[:2], dtype=torch.int32, device=dev) if (lists or tris) and th._scene else None   # (a world's rows)
    d_geom = None if geom is None else geom.data_ptr()
    _torch_ordered(th.ctx, dev, lambda: th._call(name, packed.data_ptr(), n, extra, out.data_ptr(),
                                                 d_geom if inst is None else (inst.data_ptr(), d_geom)))
    if lists:
        return QueryHitLists(out, geom, inst)
    if tris:
        return QueryTriLists(out, geom, inst)
    if kind == "trihits":
        return QueryTriHits(out, geom)
    return QueryHits(out, geom) if kind == "hits" else (out.view(torch.bool) if kind == "bool" else out)


class QueryScene:
    """The queries of TriangleHierarchy over several hierarchies at once (psm_scene_*_dev; not in the reference): an ordered list
    of 1 .. SCENE_MAX_GEOMETRIES built hierarchies of one context, e.g. a static set and the objects that move -- each rebuilt or
    refitted on its own, none merged. A candidate is (geom, tri): geom the index in the list, tri that hierarchy's triangle id.
    Closest hit / closest point: the smallest value over the scene, on a tie the lowest (geom, tri), and QueryHits.geom says
    which geometry; occluded / within: the OR; countHits: the sum; inside: parity over the crossings of ALL geometries (a closed
    surface split over several hierarchies is one surface). Arguments, numpy / torch placement and stream ordering of every
    method are those of the TriangleHierarchy method of the same name. The scene keeps references to its hierarchies and reads
    their handles at every call: a hierarchy that was rebuilt, refitted or reallocated is used as it then is."""
    _scene = True

    def __init__(self, ctx, hierarchies):
        self.ctx = ctx
        self.hierarchies = list(hierarchies)
        if not 1 <= len(self.hierarchies) <= SCENE_MAX_GEOMETRIES:
            raise ValueError("QueryScene: %d hierarchies (1 .. %d)" % (len(self.hierarchies), SCENE_MAX_GEOMETRIES))

    def _call(self, name, d_in, n, extra, d_out, d_geom):
        name = name.replace("psm_bvh_", "psm_scene_")
        g = len(self.hierarchies)
        handles = (C.c_void_p * g)(*[th._h for th in self.hierarchies])
        tail = () if d_geom is None else (C.c_void_p(d_geom),)
        self.ctx.check(getattr(lib(), name)(handles, C.c_uint32(g), C.c_void_p(d_in), C.c_size_t(n), *extra, C.c_void_p(d_out), *tail), name)

    def _launch_np(self, packed, out, name, *extra):
        return _launch_np(self, packed, out, name, *extra)

    _query = TriangleHierarchy._query
    _point_query = TriangleHierarchy._point_query

    def intersect(self, origins, directions, tmin=0.0, tmax=np.inf):
        """Closest hit of every ray over the scene (psm_scene_intersect_dev): QueryHits with geom."""
        return self._query(origins, directions, tmin, tmax, "hits")

    def occluded(self, origins, directions, tmin=0.0, tmax=np.inf):
        """Any hit inside [tmin, tmax] in any geometry (psm_scene_occluded_dev): bool."""
        return self._query(origins, directions, tmin, tmax, "bool")

    def countHits(self, origins, directions, tmin=0.0, tmax=np.inf):
        """Hits inside [tmin, tmax] summed over the geometries (psm_scene_count_hits_dev)."""
        return self._query(origins, directions, tmin, tmax, "count")

    def closestPoint(self, points, rmax=np.inf):
        """Closest point over the scene within rmax (psm_scene_closest_point_dev): QueryHits with geom."""
        return self._point_query(points, rmax, "hits", "psm_bvh_closest_point_dev")

    def within(self, points, radius):
        """Whether some triangle of some geometry is within radius (psm_scene_within_dev): bool."""
        return self._point_query(points, radius, "bool", "psm_bvh_within_dev")

    def inside(self, points, samples=3):
        """Inside / outside by the parity of each ray's crossings over ALL geometries, then the vote (psm_scene_inside_dev)."""
        return self._point_query(points, np.inf, "bool", "psm_bvh_inside_dev", samples)

    def signedDistance(self, points, rmax=np.inf, samples=3):
        """closestPoint() over the scene with the sign of inside() over the scene (psm_scene_signed_distance_dev)."""
        return self._point_query(points, rmax, "hits", "psm_bvh_signed_distance_dev", samples)


INSTANCE_ORTHONORMAL_TOL = 1e-5   # psm_hip.h: the largest entry of R^T R - 1 a pose may have


def _pose(matrix, what):
    """a pose as psm_instance takes it: float32 [3, 4] from a 3 x 4 or a 4 x 4 (last row 0 0 0 1) world-from-object matrix,
    checked as the library checks it (finite; R^T R within INSTANCE_ORTHONORMAL_TOL of the identity, in double)"""
    m = np.asarray(matrix)
    if m.shape not in ((3, 4), (4, 4)):
        raise ValueError("%s: a transform must be 3 x 4 or 4 x 4, not %s" % (what, "x".join(str(k) for k in m.shape) or "a scalar"))
    m = m.astype(np.float32)
    if not np.isfinite(m).all():
        raise ValueError("%s: a transform has a non-finite entry" % what)
    if m.shape == (4, 4) and not np.array_equal(m[3], [0, 0, 0, 1]):
        raise ValueError("%s: the last row of a 4 x 4 transform must be 0 0 0 1" % what)
    r = m[:3, :3].astype(np.float64)
    if np.abs(r.T @ r - np.eye(3)).max() > INSTANCE_ORTHONORMAL_TOL:
        raise ValueError("%s: a transform must be rigid (a rotation or reflection and a translation: no scale, no shear)" % what)
    return np.ascontiguousarray(m[:3])


class InstancedScene(QueryScene):
    """QueryScene with a pose per entry (psm_instances_*_dev; not in the reference): an ordered list of 1 .. SCENE_MAX_GEOMETRIES
    instances (TriangleHierarchy, matrix), the matrix a rigid world-from-object transform, 3 x 4 [R | T] or 4 x 4 with the last
    row 0 0 0 1. The same hierarchy may stand at many poses. A query is moved into each instance's object space and answered
    there; the answers combine as QueryScene's. Moving a body is setTransform(): nothing is rebuilt, the next call reads the new
    matrix. QueryHits.geom is the index of the winning INSTANCE; u, v, t, tri are that instance's object-space values (the point
    of triangle tri at (u, v), mapped through transforms()[geom], is the world point). Methods, arguments and numpy / torch
    placement: QueryScene's."""

    def __init__(self, ctx, instances):
        pairs = list(instances)
        super().__init__(ctx, [th for th, _ in pairs])
        self._poses = np.stack([_pose(m, "InstancedScene") for _, m in pairs])

    def setTransform(self, i, matrix):
        """Place instance i anew: the next query reads it (no rebuild, no upload)."""
        self._poses[range(len(self.hierarchies))[i]] = _pose(matrix, "InstancedScene.setTransform")

    def transforms(self):
        """The poses, float32 [instances, 3, 4] (a copy)."""
        return self._poses.copy()

    def _call(self, name, d_in, n, extra, d_out, d_geom):
        name = name.replace("psm_bvh_", "psm_instances_")
        g = len(self.hierarchies)
        insts = (Instance * g)()
        for k, th in enumerate(self.hierarchies):
            insts[k].bvh = th._h.value if isinstance(th._h, C.c_void_p) else th._h
            insts[k].world_from_object[:] = self._poses[k].reshape(12).tolist()
        tail = () if d_geom is None else (C.c_void_p(d_geom),)
        self.ctx.check(getattr(lib(), name)(insts, C.c_uint32(g), C.c_void_p(d_in), C.c_size_t(n), *extra, C.c_void_p(d_out), *tail), name)


class InstanceWorld(QueryScene):
    """InstancedScene without its limit of 32 and without its cost per instance (psm_world_*; not in the reference): up to
    WORLD_MAX_INSTANCES instances (TriangleHierarchy, matrix) in a table on the device under a tree over their world-space boxes.
    A query walks the tree and enters only the instances it can reach; the answers are exactly those an InstancedScene over the
    same ordered list would give if it could be that long (ties: the lowest (instance, triangle)). Moving bodies is
    setTransform() / setTransforms(): boxes and tree are redone on the device, no hierarchy is rebuilt. The world records its
    hierarchies as they are when set: after a member was rebuilt, reloaded or reallocated the next query raises PsmError until
    setInstances() is called again; after a member was REFITTED call refresh(). Methods, arguments and numpy / torch placement:
    QueryScene's; QueryHits.geom is the index of the winning instance. A world also has the k-best queries, firstHits() and
    nearest(), the box queries overlapsBox(), countInBox() and trianglesInBox() over world-space boxes, the sphere sweeps
    sphereCast() and sphereCastOccluded() along world-space lines, and the triangle queries overlapsTriangle(),
    countOnTriangle() and trianglesOnTriangle() on world-space triangles, and the mesh queries overlapsMesh(), countOnMesh()
    and trianglesOnMesh() of another hierarchy at world poses, and the clearance queries closestToTriangle() and
    withinOfTriangle() on world-space triangles, and mesh clearance closestToMesh(), withinOfMesh() and clearanceToMesh() of
    another hierarchy at world poses, and the grids voxelize(), voxelCounts(), voxelInstances() and distanceField() over a
    world-space grid, which the flat lists (QueryScene, InstancedScene) have not."""

    def __init__(self, ctx, entries, capacity=None):
        self.ctx = ctx
        pairs = list(entries)
        cap = max(len(pairs), 1) if capacity is None else int(capacity)
        self._w = C.c_void_p(lib().psm_world_create(ctx._h, C.c_uint32(cap)))
        if not self._w:
            raise PsmError("psm_world_create: %s" % lib().psm_last_error(ctx._h).decode())
        self.hierarchies, self._poses, self._handles = [], np.zeros((0, 3, 4), np.float32), []
        try:
            self.setInstances(pairs)
        except Exception:
            self.close()
            raise

    def setInstances(self, entries):
        """Set the whole list anew (psm_world_set_instances): table, boxes and tree; an empty list empties the world."""
        pairs = list(entries)
        poses = np.stack([_pose(m, "InstanceWorld") for _, m in pairs]) if pairs else np.zeros((0, 3, 4), np.float32)
        handles = [th._h.value if isinstance(th._h, C.c_void_p) else th._h for th, _ in pairs]
        insts = np.zeros(len(pairs), INSTANCE_DT)
        insts["bvh"] = [h or 0 for h in handles]
        insts["world_from_object"] = poses.reshape(-1, 12)
        self.hierarchies, self._poses, self._handles = [], np.zeros((0, 3, 4), np.float32), []   # (a refused list leaves what the library leaves)
        self.ctx.check(lib().psm_world_set_instances(self._w, _p(insts), C.c_uint32(len(pairs))), "psm_world_set_instances")
        self.hierarchies, self._poses, self._handles = [th for th, _ in pairs], poses, handles

    def __len__(self):
        return int(lib().psm_world_count(self._w))

    def setTransform(self, i, matrix):
        """Place instance i anew (psm_world_set_transforms): no hierarchy is rebuilt."""
        i = range(len(self.hierarchies))[i]
        self.setTransforms(i, [matrix])

    def setTransforms(self, first, matrices):
        """Place instances first .. first + len(matrices) - 1 anew."""
        ms = np.stack([_pose(m, "InstanceWorld.setTransforms") for m in matrices]) if len(matrices) else np.zeros((0, 3, 4), np.float32)
        if first < 0 or first + ms.shape[0] > len(self.hierarchies):
            raise IndexError("InstanceWorld.setTransforms: instances %d .. %d of %d" % (first, first + ms.shape[0], len(self.hierarchies)))
        self._fresh("psm_world_set_transforms")
        self.ctx.check(lib().psm_world_set_transforms(self._w, C.c_uint32(first), C.c_uint32(ms.shape[0]), _p(np.ascontiguousarray(ms))),
                       "psm_world_set_transforms")
        self._poses[first:first + ms.shape[0]] = ms

    def refresh(self):
        """After a member hierarchy was refitted: the boxes and the tree are redone from the triangles as they now are."""
        self.setTransforms(0, self._poses)

    def transforms(self):
        """The poses, float32 [instances, 3, 4] (a copy)."""
        return self._poses.copy()

    def _fresh(self, name):
        """a hierarchy whose handle is no longer the one recorded was reallocated: the library must not be given the old one"""
        for k, (th, h) in enumerate(zip(self.hierarchies, self._handles)):
            if (th._h.value if isinstance(th._h, C.c_void_p) else th._h) != h:
                raise PsmError("%s: instance %d's hierarchy was reallocated after the instances were set (set the instances again)" % (name, k))

    def firstHits(self, origins, directions, k, tmin=0.0, tmax=np.inf):
        """The first k hits of every ray over the whole world, in order (psm_world_first_hits_dev): of the candidates countHits()
        counts, the min(k, count) smallest in (t, instance, tri) -- bit-equal t (coincident instances, coincident triangles, a
        shared edge) are all listed, the lowest instance first. k: 1 .. QUERY_K_MAX. Returns QueryHitLists: u, v, t, tri and geom
        (the slot's instance) [n, k], each record the instance's object-space values (slot 0 and geom[:, 0] are intersect()'s
        record and geom; the slots past count are misses: tri = -1, t = +inf, geom = -1) and count [n]. Arguments and placement
        as intersect()."""
        return self._query(origins, directions, tmin, tmax, "lists", "psm_bvh_first_hits_dev", k)

    def nearest(self, points, k, rmax=np.inf):
        """The k nearest triangles of every point within rmax over the whole world (psm_world_nearest_dev): the min(k, count)
        smallest in (d2, instance, tri), d2 each instance's own squared distance to its moved point. k: 1 .. QUERY_K_MAX. Returns
        QueryHitLists with geom: t = the distance, u, v as closestPoint()'s (slot 0 and geom[:, 0] are closestPoint()'s record
        and geom). Arguments and placement as closestPoint()."""
        return self._point_query(points, rmax, "lists", "psm_bvh_nearest_dev", k=k)

    def overlapsBox(self, lo, hi):
        """Whether some triangle of some instance overlaps each axis-aligned WORLD box [lo, hi] (psm_world_box_overlaps_dev): lo,
        hi [n, 3]. The box stays in world space; each candidate triangle is posed forward in float32 (v0' = R v0 + T, e1' = R e1,
        e2' = R e2) and judged by boxOverlaps()'s test (psm_hip.h "box queries over a world"). Closed; a point is a box; a box with
        a non-finite number or lo > hi overlaps nothing. A bool array / tensor; numpy / torch placement as intersect()."""
        return self._box_query(lo, hi, "bool", "psm_bvh_box_overlaps_dev")

    def countInBox(self, lo, hi):
        """The number of (instance, triangle) pairs that overlap each world box, summed over the instances
        (psm_world_box_count_dev). A uint32 array, or an int32 tensor for torch tensors. Arguments as overlapsBox()."""
        return self._box_query(lo, hi, "count", "psm_bvh_box_count_dev")

    def trianglesInBox(self, lo, hi, k):
        """Which triangles of which instances overlap each world box (psm_world_box_triangles_dev): of the pairs countInBox()
        counts, the min(k, count) lowest in (instance, tri), ascending -- coincident instances list a shared triangle once per
        instance, the lowest instance first. k: 1 .. QUERY_K_MAX. Returns QueryTriLists: tri and geom (the slot's instance)
        [n, k] int32, -1 in both past count, and count [n]. Arguments as overlapsBox()."""
        if not 1 <= _k(k, "psm_world_box_triangles_dev") <= QUERY_K_MAX:   # (refused here: no call is made)
            raise PsmError("psm_world_box_triangles_dev: k must be 1 .. %d" % QUERY_K_MAX)
        return self._box_query(lo, hi, "tris", "psm_bvh_box_triangles_dev", k)

    _box_query = TriangleHierarchy._box_query

    def sphereCast(self, origins, directions, radius, tmax=np.inf):
        """Where a sphere of `radius` that moves from each WORLD origin along its world direction first touches a triangle of
        some instance within the distance tmax (psm_world_sweep_sphere_dev): origins, directions [n, 3] (any length; normalised
        inside), radius and tmax scalars or per-sweep [n]. The sweep is moved into each instance as a ray is and judged there by
        TriangleHierarchy.sweepSphere()'s test, so the answer is exactly the brute force over the ordered instance list: the
        smallest t, on a bit-equal t the lowest (instance, tri). Returns QueryHits with geom: the winning instance's index and
        its object-space u, v, t, tri (geom = tri = -1, t = +inf: no contact); t = 0 whenever within(origin, radius) holds.
        Invalid sweeps miss, as sweepSphere()'s. numpy / torch placement as intersect()."""
        return self._query(origins, directions, radius, tmax, "hits", "psm_bvh_sweep_sphere_dev")

    def sphereCastOccluded(self, origins, directions, radius, tmax=np.inf):
        """Whether the swept sphere touches any triangle of any instance within tmax (psm_world_sweep_occluded_dev): the
        predicate isfinite(sphereCast().t), the walk ending at the first contact found. A bool array / tensor. Arguments and
        placement as sphereCast()."""
        return self._query(origins, directions, radius, tmax, "bool", "psm_bvh_sweep_occluded_dev")

    def overlapsTriangle(self, tris):
        """Whether some triangle of some instance meets each WORLD triangle (psm_world_tri_overlaps_dev): tris [n, 3, 3] or
        [n, 9], the vertices a, b, c of each. The query stays in world space; each candidate triangle is posed forward in float32
        (v0' = R v0 + T, e1' = R e1, e2' = R e2) and judged by triOverlaps()'s test (psm_hip.h "triangle queries over a world").
        Closed; a segment or a point is a valid query; one with a non-finite number meets nothing. A bool array / tensor; numpy /
        torch placement as intersect()."""
        return self._tri_query(tris, "bool", "psm_bvh_tri_overlaps_dev")

    def countOnTriangle(self, tris):
        """The number of (instance, triangle) pairs that meet each world triangle, summed over the instances
        (psm_world_tri_count_dev). A uint32 array, or an int32 tensor for torch tensors. Arguments as overlapsTriangle()."""
        return self._tri_query(tris, "count", "psm_bvh_tri_count_dev")

    def trianglesOnTriangle(self, tris, k):
        """Which triangles of which instances meet each world triangle (psm_world_tri_triangles_dev): of the pairs
        countOnTriangle() counts, the min(k, count) lowest in (instance, tri), ascending -- coincident instances list a shared
        triangle once per instance, the lowest instance first. k: 1 .. QUERY_K_MAX. Returns QueryTriLists: tri and geom (the
        slot's instance) [n, k] int32, -1 in both past count, and count [n]. Arguments as overlapsTriangle()."""
        if not 1 <= _k(k, "psm_world_tri_triangles_dev") <= QUERY_K_MAX:   # (refused here: no call is made)
            raise PsmError("psm_world_tri_triangles_dev: k must be 1 .. %d" % QUERY_K_MAX)
        return self._tri_query(tris, "tris", "psm_bvh_tri_triangles_dev", k)

    _tri_query = TriangleHierarchy._tri_query

    def closestToTriangle(self, tris, rmax=np.inf):
        """The nearest (instance, triangle) pair of the world to each WORLD triangle within rmax, its distance and the two
        nearest points (psm_world_tri_closest_dev): tris [n, 3, 3] or [n, 9], rmax a scalar or [n] (+inf: no limit; NaN or
        negative: a miss). The query stays in world space; each candidate triangle is posed forward in float32 (v0' = R v0 + T,
        e1' = R e1, e2' = R e2) and judged by triClosest()'s test (psm_hip.h "clearance queries over a world"), so dist == 0
        exactly where overlapsTriangle() counts the pair. The smallest float32 squared distance wins, on a bit-equal one the
        lowest (instance, tri). Returns QueryTriHits with geom, the winning instance (geom = tri = -1, dist = +inf on a miss);
        (u, v) weigh the stored triangle's edges, which are weights of the posed triangle as well: the point on the world is
        (v0' + u e1') + v e2' (QueryTriHits.points_world). numpy / torch placement as triClosest()."""
        return self._tri_dist_query(tris, rmax, "trihits", "psm_bvh_tri_closest_dev")

    def withinOfTriangle(self, tris, r):
        """Whether some triangle of some instance is within r of each world triangle (psm_world_tri_within_dev): the predicate
        closestToTriangle(tris, r).tri >= 0, with the walk ended at the first such pair. A bool array / tensor. Arguments and
        placement as closestToTriangle()."""
        return self._tri_dist_query(tris, r, "bool", "psm_bvh_tri_within_dev")

    _tri_dist_query = TriangleHierarchy._tri_dist_query

    def overlapsMesh(self, other, poses, skip=None, as_torch=False):
        """Whether `other`, a built TriangleHierarchy of this context (it may be a member of the world), meets some triangle of
        some instance at each pose (psm_world_mesh_overlaps_dev; not in the reference). poses: one matrix or [p, 3, 4] /
        [p, 4, 4], each a rigid [R | T] that takes a point of other's object space into WORLD space, checked as an instance's
        pose is: a non-rigid one raises before any call. The query triangles are other's stored leaves posed in float32 on the
        device (psm_hip.h "mesh queries over a world"); each is answered bit for bit as overlapsTriangle() answers it. skip: an
        instance index that is left out (the answer is that of the list without it, the other indices kept: "body i at a new
        pose against all the others" is skip=i with other = its hierarchy), None for none. A numpy bool [p]; with as_torch=True a
        torch bool tensor on the context's device, the launch ordered against torch's current stream by events (the call itself
        waits once for its pose upload, as setTransforms() does, and cannot be captured into a graph)."""
        return self._mesh_query(other, poses, skip, "bool", "psm_world_mesh_overlaps_dev", None, as_torch)

    def countOnMesh(self, other, poses, skip=None, as_torch=False):
        """How many (instance, triangle) pairs of the world meet each triangle of `other` at each pose
        (psm_world_mesh_count_dev; not in the reference): uint32 [p, T], T = other.triangleCount, indexed by other's load-order
        triangle id (an int32 tensor with as_torch=True); a triangle other's build dropped counts 0. Arguments and placement
        as overlapsMesh()."""
        return self._mesh_query(other, poses, skip, "count", "psm_world_mesh_count_dev", None, as_torch)

    def trianglesOnMesh(self, other, poses, k, skip=None, as_torch=False):
        """Which triangles of which instances meet each triangle of `other` at each pose (psm_world_mesh_triangles_dev; not in
        the reference): of the pairs countOnMesh() counts, the min(k, count) lowest in (instance, tri), ascending. k: 1 ..
        QUERY_K_MAX. Returns QueryTriLists: tri and geom (the slot's instance) [p, T, k] int32, -1 in both past count, and count
        [p, T]. Arguments and placement as overlapsMesh()."""
        if not 1 <= _k(k, "psm_world_mesh_triangles_dev") <= QUERY_K_MAX:   # (refused here: no call is made)
            raise PsmError("psm_world_mesh_triangles_dev: k must be 1 .. %d" % QUERY_K_MAX)
        return self._mesh_query(other, poses, skip, "tris", "psm_world_mesh_triangles_dev", int(k), as_torch)

    def _mesh_query(self, other, poses, skip, out, name, k, as_torch):
        """one mesh query of the world (TriangleHierarchy._mesh_query's shape): the poses and skip checked on the host, the
        poses packed [p, 12], the outputs [p] / [p, T] / [p, T, k] twice and [p, T]"""
        m12, p, t = _mesh_poses(other, poses, name)
        s = _mesh_skip(self, skip, name)
        self._fresh(name)
        extra = () if k is None else (C.c_uint32(k),)
        fn = getattr(lib(), name)

        def call(*d_outs):
            self.ctx.check(fn(self._w, other._h, _p(m12), C.c_size_t(p), C.c_int32(s), *extra, *map(C.c_void_p, d_outs)), name)

        res = _device_call(self.ctx, call, _mesh_outs(out, p, t, k, True), as_torch)
        if out == "tris":
            ids, inst, cnt = res
            return QueryTriLists(ids, cnt, inst)
        return _bool_view(res[0]) if out == "bool" else res[0]

    def closestToMesh(self, other, poses, rmax=np.inf, skip=None, as_torch=False):
        """The nearest (instance, triangle) pair of the world to each triangle of `other` at each pose within rmax
        (psm_world_mesh_closest_dev; not in the reference): each stored triangle of other is posed in float32 on the device, as
        countOnMesh() poses it, and answered bit for bit as closestToTriangle() answers it. rmax: one scalar (+inf: no limit; NaN
        or negative: a miss everywhere). Returns QueryTriHits over a [p, T, 8] buffer with geom [p, T], T = other.triangleCount,
        indexed by other's load-order triangle id (tri = geom = -1, dist = +inf on a miss and for a triangle other's build
        dropped). skip, the poses and the placement as overlapsMesh()."""
        return self._mesh_dist_query(other, poses, rmax, skip, "closest", "psm_world_mesh_closest_dev", as_torch)

    def withinOfMesh(self, other, poses, r, skip=None, as_torch=False):
        """Whether some triangle of `other` comes within r of some triangle of some instance at each pose
        (psm_world_mesh_within_dev; not in the reference): clearanceToMesh(other, poses, r, skip).tri >= 0, with every walk ended
        at its first such pair. A bool [p]. Arguments and placement as closestToMesh()."""
        return self._mesh_dist_query(other, poses, r, skip, "bool", "psm_world_mesh_within_dev", as_torch)

    def clearanceToMesh(self, other, poses, rmax=np.inf, skip=None, as_torch=False):
        """The one nearest pair of each pose (psm_world_mesh_clearance_dev; not in the reference): of closestToMesh()'s records
        of a pose the one with the smallest dist, on an equal float32 dist the lowest triangle of other -- found inside the
        launch, the triangles of a pose sharing the best distance so far as their bound. Returns QueryMeshHits over a [p, 8]
        buffer with geom [p]: u, v, dist, tri, s, t, .other (other's triangle) and .geom (the instance; tri = other = geom = -1,
        dist = +inf where no pair is within rmax); .points_world() gives the two witness points. Arguments and placement as
        closestToMesh()."""
        return self._mesh_dist_query(other, poses, rmax, skip, "clearance", "psm_world_mesh_clearance_dev", as_torch)

    def _mesh_dist_query(self, other, poses, rmax, skip, out, name, as_torch):
        """one mesh clearance query of the world: poses and skip as _mesh_query checks and packs them, rmax one float, the
        outputs [p, T, 8] and [p, T] / [p] / [p, 8] and [p]"""
        m12, p, t = _mesh_poses(other, poses, name)
        if np.ndim(rmax) != 0:
            raise ValueError("%s: rmax must be one scalar" % name)
        s = _mesh_skip(self, skip, name)
        self._fresh(name)
        fn = getattr(lib(), name)

        def call(*d_outs):
            self.ctx.check(fn(self._w, other._h, _p(m12), C.c_size_t(p), C.c_int32(s), C.c_float(rmax), *map(C.c_void_p, d_outs)), name)

        res = _device_call(self.ctx, call, _mesh_dist_outs(out, p, t, True), as_torch)
        if out == "bool":
            return _bool_view(res[0])
        return QueryTriHits(*res) if out == "closest" else QueryMeshHits(res[0], True, res[1])

    def voxelize(self, origin, cell, dims, solid=False, samples=3, as_torch=False):
        """The voxels of a regular WORLD grid that a posed triangle of some instance overlaps (psm_grid_world_surface_dev; not in
        the reference), or with solid=True those and the voxels whose centre inside() takes as inside with `samples` (1, 3 or 5)
        rays (psm_grid_world_solid_dev). The grid, its voxel boxes (voxel_boxes()) and the VoxelGrid returned are
        TriangleHierarchy.voxelize()'s; a voxel's bit is bit for bit what overlapsBox() answers for its box: one call, no box
        records. An invalid grid raises ValueError before any call. Not covered: the skip of one instance, sparse output,
        oriented grids, graph capture of solid (the signed-distance grid of a world is distanceField())."""
        g = _grid(origin, cell, dims)
        return _voxel_call(self.ctx, self._w, "psm_grid_world_", "solid" if solid else "surface", g, np.uint64, as_torch,
                           samples if solid else None, self._fresh)

    def voxelCounts(self, origin, cell, dims, as_torch=False):
        """How many (instance, triangle) pairs overlap each voxel of a regular world grid (psm_grid_world_counts_dev; not in the
        reference): uint32 [nz, ny, nx] (an int32 tensor with as_torch=True), each entry what countInBox() answers for the voxel's
        box. Arguments and placement as voxelize()."""
        g = _grid(origin, cell, dims)
        return _voxel_call(self.ctx, self._w, "psm_grid_world_", "counts", g, np.uint32, as_torch, fresh=self._fresh)

    def voxelInstances(self, origin, cell, dims, as_torch=False):
        """Which body owns each voxel of a regular world grid (psm_grid_world_instances_dev; not in the reference): int32 [nz, ny,
        nx], the lowest instance index that has a triangle overlapping the voxel -- trianglesInBox(lo, hi, 1).geom[:, 0] of the
        voxel's box --, -1 where voxelCounts() is 0: a labelled occupancy map. Arguments and placement as voxelize()."""
        g = _grid(origin, cell, dims)
        return _voxel_call(self.ctx, self._w, "psm_grid_world_", "instances", g, np.int32, as_torch, fresh=self._fresh)

    def distanceField(self, origin, cell, dims, rmax=np.inf, signed=False, samples=3, nearest=True, as_torch=False):
        """The distance from every voxel centre of a regular WORLD grid to the nearest posed triangle of any instance
        (psm_grid_world_distance_dev; not in the reference), or with signed=True that distance with the sign of inside(centre,
        samples) over all instances (psm_grid_world_signed_distance_dev): a planner's clearance map or a narrow-band level set
        over bodies that each move by a matrix per step, in one call. Arguments, the centres (voxel_centres()) and rmax are
        TriangleHierarchy.distanceField()'s. Every voxel is bit for bit what closestPoint() / signedDistance() of the world
        answer for its centre with the same rmax and samples (t, tri and the instance; -0.0 can occur in a signed field); on a
        bit-equal squared distance the lexicographically lowest (instance, triangle) wins. Returns DistanceGrid with dist float32,
        tri and inst int32, each [nz, ny, nx] (tri and inst None with nearest=False); a miss holds +inf, -1, -1; with
        as_torch=True torch tensors on the context's device, ordered against torch's current stream by events. An invalid grid
        and a NaN or negative rmax raise ValueError before any call. Not covered: the skip of one instance, a per-voxel rmax,
        sparse output, graph capture of the signed call."""
        g, r = _grid(origin, cell, dims), _rmax(rmax)
        return _distance_call(self.ctx, self._w, "psm_grid_world_", g, r, signed, samples, nearest, as_torch,
                              inst=True, fresh=self._fresh)

    def _call(self, name, d_in, n, extra, d_out, d_geom):
        name = name.replace("psm_bvh_", "psm_world_")
        self._fresh(name)
        if isinstance(d_geom, tuple):   # (the k-best queries: the instances [n, k], then the counts [n])
            tail = tuple(C.c_void_p(p) for p in d_geom)
        else:
            tail = () if d_geom is None else (C.c_void_p(d_geom),)
        self.ctx.check(getattr(lib(), name)(self._w, C.c_void_p(d_in), C.c_size_t(n), *extra, C.c_void_p(d_out), *tail), name)

    def close(self):
        if self._w:
            lib().psm_world_destroy(self._w)
            self._w = C.c_void_p()


class TextureSet:
    """psm::TextureSet (Include/Prismarine/TextureSet.{hpp,inl}): slot table of material textures. A texture
    is an RGBA8 image, uint8 [h,w,4], row 0 = v 0 (GL order); slot 0 means "none" (TextureSet.inl:7-12)."""

    def __init__(self):
        self.textures = [None]
        self.freedomTextures = []
        self.revision = 1

    def loadTexture(self, image):
        """TextureSet.inl:73-86: reuse a freed slot, else append; returns the slot index materials refer to."""
        img = np.ascontiguousarray(image, np.uint8)
        if img.ndim != 3 or img.shape[2] != 4:
            raise ValueError("texture must be uint8 [h,w,4]")
        if self.freedomTextures:
            idx = self.freedomTextures.pop()
            self.textures[idx] = img
        else:
            idx = len(self.textures)
            self.textures.append(img)
        self.revision += 1
        return idx

    def freeTexture(self, idx):
        self.freedomTextures.append(idx)
        self.textures[idx] = None
        self.revision += 1

    def clearGlTextures(self):
        for i in range(1, len(self.textures)):
            self.freeTexture(i)

    def loadToVGA(self):
        pass  # uploaded by Pipeline.applyMaterials


class MaterialSet:
    """psm::MaterialSet (Include/Prismarine/MaterialSet.hpp:28-41): a host-side material array."""

    def __init__(self):
        self.submats = []
        self.loadOffset = 0
        self.texset = None

    def setTextureSet(self, txs):
        self.texset = txs

    def addSubmat(self, m):
        self.submats.append(m)
        return len(self.submats) - 1

    def setSumbat(self, i, m):
        while len(self.submats) <= i:
            self.submats.append(dict(self.submats[-1]) if self.submats else m)
        self.submats[i] = m

    def clearSubmats(self):
        self.submats = []

    def getMaterialCount(self):
        return len(self.submats)

    def setLoadingOffset(self, off):
        self.loadOffset = off

    def loadToVGA(self):
        pass  # uploaded by Pipeline.applyMaterials


class Pipeline:
    """psm::Pipeline (Include/Prismarine/Pipeline.hpp:84-137)."""

    def __init__(self, ctx, seed=1):
        from . import scenes as _sc
        self._sc = _sc
        self.ctx = ctx
        self._h = C.c_void_p()
        ctx.check(lib().psm_rt_create(ctx._h, C.byref(self._h)), "psm_rt_create")
        self.width = self.height = self.displayWidth = self.displayHeight = 256  # Pipeline.hpp:87-90
        self.raycountCache = 0
        self._rand_state = seed & 0xFFFFFFFF
        self._mat_sig = None
        self._tex_sig = None
        self.resizeBuffers(256, 256)
        self.resize(256, 256)

    # host rand() of Pipeline.inl:282,426 made explicit: the MSVC CRT LCG, seedable
    def setSeed(self, seed):
        self._rand_state = seed & 0xFFFFFFFF

    def _rand(self):
        self._rand_state = (self._rand_state * 214013 + 2531011) & 0xFFFFFFFF
        return (self._rand_state >> 16) & 0x7FFF

    def resizeBuffers(self, w, h):
        self.width, self.height = w, h
        self.ctx.check(lib().psm_rt_resize_buffers(self._h, C.c_uint32(w), C.c_uint32(h)), "psm_rt_resize_buffers")

    def resize(self, w, h):
        self.displayWidth, self.displayHeight = w, h
        self.ctx.check(lib().psm_rt_resize(self._h, C.c_uint32(w), C.c_uint32(h)), "psm_rt_resize")

    def setTile(self, y0, y1):
        self.ctx.check(lib().psm_rt_set_tile(self._h, C.c_uint32(y0), C.c_uint32(y1)), "psm_rt_set_tile")

    def setTileInterleaved(self, rank, world, weights=None):
        """8-row bands dealt to the ranks: round-robin, or weights[r] bands of every period of sum(weights) for rank r
        (psm_rt_set_tile_weighted; dist.band_pattern is the same dealing in Python)."""
        wv = None if weights is None else (C.c_uint32 * world)(*[int(v) for v in weights])
        self.ctx.check(lib().psm_rt_set_tile_weighted(self._h, C.c_uint32(rank), C.c_uint32(world), wv),
                       "psm_rt_set_tile_weighted")

    def tile_texels(self):
        n = C.c_uint32()
        self.ctx.check(lib().psm_rt_tile_texels(self._h, C.byref(n)), "psm_rt_tile_texels")
        return n.value

    def pack_texels_dev(self, dev_ptr):
        self.ctx.check(lib().psm_rt_pack_texels_dev(self._h, C.c_void_p(dev_ptr)), "psm_rt_pack_texels_dev")

    def unpack_tiles_dev(self, world, skip_rank, dev_ptr, stride_floats):
        """all the other ranks' gathered tiles (dense, stride_floats apart) into this image in one launch"""
        self.ctx.check(lib().psm_rt_unpack_tiles_dev(self._h, C.c_uint32(world), C.c_uint32(skip_rank), C.c_void_p(dev_ptr),
                                                     C.c_size_t(stride_floats)), "psm_rt_unpack_tiles_dev")

    def unpack_texels_dev(self, interleaved, a, b, dev_ptr):
        self.ctx.check(lib().psm_rt_unpack_texels_dev(self._h, C.c_int(int(interleaved)), C.c_uint32(a), C.c_uint32(b),
                                                      C.c_void_p(dev_ptr)), "psm_rt_unpack_texels_dev")

    def ray_count_dev(self, dev_ptr):
        self.ctx.check(lib().psm_rt_ray_count_dev(self._h, C.c_void_p(dev_ptr)), "psm_rt_ray_count_dev")

    def set_ray_count(self, n):
        self.ctx.check(lib().psm_rt_set_ray_count(self._h, C.c_int32(n)), "psm_rt_set_ray_count")
        self.raycountCache = n

    def setLights(self, lights):
        lights = np.ascontiguousarray(lights, LIGHT_DT)
        self.ctx.check(lib().psm_rt_set_lights(self._h, _p(lights), C.c_uint32(lights.shape[0])), "psm_rt_set_lights")

    def setSky(self, rgb):
        a = np.asarray(list(rgb)[:3] + [1.0], np.float32)
        self.ctx.check(lib().psm_rt_set_sky(self._h, _p(a)), "psm_rt_set_sky")

    def setSkybox(self, image):
        """setSkybox(GLuint) (Pipeline.hpp:93): here the equirect image itself, uint8 [h,w,4] RGBA (None =
        constant sky colour). Sampled as public/environment.glsl:23-26 does (GL_LINEAR, clamp to edge)."""
        if image is None:
            self.ctx.check(lib().psm_rt_set_skybox(self._h, None, C.c_uint32(0), C.c_uint32(0)), "psm_rt_set_skybox")
            return
        img = np.ascontiguousarray(image, np.uint8)
        self.ctx.check(lib().psm_rt_set_skybox(self._h, _p(img), C.c_uint32(img.shape[1]), C.c_uint32(img.shape[0])),
                       "psm_rt_set_skybox")

    def clearSampler(self):
        self.ctx.check(lib().psm_rt_clear_sampler(self._h), "psm_rt_clear_sampler")

    def switchMode(self):
        """Pipeline.inl:128-132: clear, then toggle the 360-degree camera (camera.comp:48-59)."""
        self.raycountCache = 0
        self.clearSampler()
        self.enable360 = 0 if getattr(self, "enable360", 0) else 1
        self.ctx.check(lib().psm_rt_set_camera_mode(self._h, C.c_int(self.enable360)), "psm_rt_set_camera_mode")

    def camera_matrices(self, cam_inv, proj_inv, time=None):
        t = self._rand() if time is None else time
        ci = np.ascontiguousarray(cam_inv, np.float32).reshape(16)
        pi = np.ascontiguousarray(proj_inv, np.float32).reshape(16)
        self.ctx.check(lib().psm_rt_camera(self._h, _p(ci), _p(pi), C.c_uint32(t)), "psm_rt_camera")
        self._reload()

    def camera(self, eye, view):
        ci, pi = self._sc.camera_matrices(eye, view, self.displayWidth, self.displayHeight)
        self.camera_matrices(ci, pi)

    def _reload(self):
        n = C.c_int32()
        self.ctx.check(lib().psm_rt_ray_count(self._h, C.byref(n)), "psm_rt_ray_count")
        self.raycountCache = n.value

    def getRayCount(self):
        return self.raycountCache if self.raycountCache >= 32 else 0  # Pipeline.inl:459-461

    def setTraverseMode(self, mode):
        """Tuning knob (psm_rt_set_traverse_mode): which kernel schedule intersection() runs as -- "auto", "whole",
        "phased", "adaptive" or a TRAVERSE_* value. Results never depend on it."""
        m = TRAVERSE_MODES[mode] if isinstance(mode, str) else int(mode)
        self.ctx.check(lib().psm_rt_set_traverse_mode(self._h, C.c_int(m)), "psm_rt_set_traverse_mode")

    def setTraversePhases(self, caps, min_rays=1 << 20):
        """psm_rt_set_traverse_phases: wave-step caps of the launches an intersection() is cut into (selects "phased")."""
        arr = (C.c_uint32 * max(len(caps), 1))(*caps)
        self.ctx.check(lib().psm_rt_set_traverse_phases(self._h, arr, C.c_uint32(len(caps)), C.c_uint32(min_rays)),
                       "psm_rt_set_traverse_phases")

    def setTraverseAdaptive(self, min_live=12, min_steps=8, final_rays=65536, max_launches=4, min_rays=1 << 19):
        """psm_rt_set_traverse_adaptive: parameters of the "adaptive" schedule (does not select it)."""
        self.ctx.check(lib().psm_rt_set_traverse_adaptive(self._h, C.c_uint32(min_live), C.c_uint32(min_steps),
                                                          C.c_uint32(final_rays), C.c_uint32(max_launches),
                                                          C.c_uint32(min_rays)), "psm_rt_set_traverse_adaptive")

    def setTraverseSolo(self, solo_max=1):
        """psm_rt_set_traverse_solo: a traversal wave left with at most solo_max rays (0..4) walks them one at a time with all its
        lanes on one ray; 0 switches the gear off. Results never depend on it."""
        self.ctx.check(lib().psm_rt_set_traverse_solo(self._h, C.c_uint32(solo_max)), "psm_rt_set_traverse_solo")

    def resetHits(self):
        """Forget the hit chains of the current queue (ray.hit = -1): the next intersection() starts afresh."""
        self.ctx.check(lib().psm_rt_reset_hits(self._h), "psm_rt_reset_hits")

    def intersection(self, obj, clearDepth=0, force=False):
        """force=True skips the local >=32 rule (tile-sharded frames decide on the global count).
        Called with several hierarchies before shade(), the hits chain across them (multi-BVH,
        directTraverse.comp:219-249,335-346); download_hits() then reports tri | object_sequence << 27."""
        if obj is None or obj.triangleCount <= 0:
            return 0
        if (self.raycountCache if force else self.getRayCount()) <= 0:
            return 0
        self._obj = obj
        self.ctx.check(lib().psm_rt_traverse(self._h, obj._h), "psm_rt_traverse")
        return 1

    def applyMaterials(self, mat):
        sig = (id(mat), len(mat.submats), mat.loadOffset)
        if sig != self._mat_sig:
            arr = self._sc.materials_array(mat.submats)
            self.ctx.check(lib().psm_rt_set_materials(self._h, _p(arr), C.c_uint32(arr.shape[0]),
                                                      C.c_int32(mat.loadOffset)), "psm_rt_set_materials")
            self._mat_sig = sig
        ts = mat.texset
        if ts is not None and (id(ts), ts.revision) != self._tex_sig:
            for i in range(1, 32):
                img = ts.textures[i] if i < len(ts.textures) else None
                if img is None:
                    self.ctx.check(lib().psm_rt_set_texture(self._h, C.c_uint32(i), None, C.c_uint32(0), C.c_uint32(0)),
                                   "psm_rt_set_texture")
                else:
                    self.ctx.check(lib().psm_rt_set_texture(self._h, C.c_uint32(i), _p(img), C.c_uint32(img.shape[1]),
                                                            C.c_uint32(img.shape[0])), "psm_rt_set_texture")
            self._tex_sig = (id(ts), ts.revision)

    def shade(self, time=None, force=False, reload=True):
        """reload=False leaves raycountCache stale: the caller learns the count elsewhere (ray_count_dev +
        an all-gather) and reports it with set_ray_count()."""
        if not force and self.getRayCount() <= 0:
            return
        t = self._rand() if time is None else time  # drawn every round so sharded ranks stay in step
        if self.raycountCache <= 0:
            return
        self.ctx.check(lib().psm_rt_shade(self._h, self._obj._h, C.c_uint32(t)), "psm_rt_shade")
        if reload:
            self._reload()

    def reclaim(self):
        pass  # Pipeline.inl:361-369 is a no-op

    def sample(self):
        self.ctx.check(lib().psm_rt_sample(self._h), "psm_rt_sample")

    def render(self):
        pass  # display quad: out of scope (render.vert/frag)

    def snapHdr(self, raw=False):
        out = np.zeros((self.displayHeight, self.displayWidth, 4), np.float32)
        self.ctx.check(lib().psm_rt_snap(self._h, _p(out), C.c_int(int(raw))), "psm_rt_snap")
        return out

    def snapRawHdr(self):
        return self.snapHdr(True)

    # parity / debug access
    def download_rays(self):
        n = self.raycountCache
        out = np.zeros(max(n, 1), RAY_DT)
        cnt = C.c_uint32()
        self.ctx.check(lib().psm_rt_download_rays(self._h, _p(out), C.c_uint32(n), C.byref(cnt)), "psm_rt_download_rays")
        return out[:n]

    def upload_rays(self, rays):
        rays = np.ascontiguousarray(rays, RAY_DT)
        self.ctx.check(lib().psm_rt_upload_rays(self._h, _p(rays), C.c_uint32(rays.shape[0])), "psm_rt_upload_rays")
        self.raycountCache = rays.shape[0]

    def download_hits(self, n):
        hits = np.zeros((max(n, 1), 8), HIT_DT)
        counts = np.zeros(max(n, 1), np.int32)
        self.ctx.check(lib().psm_rt_download_hits(self._h, _p(hits), _p(counts), C.c_uint32(n)), "psm_rt_download_hits")
        return hits[:n], counts[:n]

    def download_texels(self):
        wh = self.width * self.height
        s = np.zeros((wh, 4), np.float32)
        c = np.zeros((wh, 2), np.float32)
        f = np.zeros(wh, np.int32)
        self.ctx.check(lib().psm_rt_download_texels(self._h, _p(s), _p(c), _p(f)), "psm_rt_download_texels")
        return s, c, f

    def get_texels_dev(self, y0, y1, dev_ptr):
        self.ctx.check(lib().psm_rt_get_texels_dev(self._h, C.c_uint32(y0), C.c_uint32(y1), C.c_void_p(dev_ptr)),
                       "psm_rt_get_texels_dev")

    def set_texels_dev(self, y0, y1, dev_ptr):
        self.ctx.check(lib().psm_rt_set_texels_dev(self._h, C.c_uint32(y0), C.c_uint32(y1), C.c_void_p(dev_ptr)),
                       "psm_rt_set_texels_dev")

    def close(self):
        if self._h:
            lib().psm_rt_destroy(self._h)
            self._h = C.c_void_p()


def write_pfm(path, image):
    """Save an HDR snapshot (snapHdr(); the app writes EXR on key L, Application.hpp:324-343) as a PFM file: 'PF', width height,
    scale -1.0 (little endian), RGB float32, rows BOTTOM TO TOP -- which is the order snapHdr() returns them in: row 0 of the
    sampler's image is the picture's bottom row (camera.comp:61: texel row 0 is NDC y = -1; the reference's HdrImage and FreeImage's
    scanlines are bottom-up alike), so the rows are written as they come."""
    img = np.ascontiguousarray(image[..., :3], np.float32)
    with open(path, "wb") as f:
        f.write(("PF\n%d %d\n-1.0\n" % (img.shape[1], img.shape[0])).encode())
        f.write(img.astype("<f4").tobytes())


def read_pfm(path):
    """The image of a PFM file in snapHdr()'s row order (row 0 = the picture's bottom row)."""
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4").reshape(h, w, 3)
    return data.copy()


def write_exr(path, image):
    """Save an HDR snapshot as the app does on key L (PathTracerApplication::saveHdr, Application.hpp:324-343: FreeImage FIT_RGBAF ->
    FIF_EXR, EXR_FLOAT): an OpenEXR scan-line file, channels A B G R as 32-bit floats, one scan line per chunk, NO_COMPRESSION
    (the app asks FreeImage for PIZ; which lossless compression a file uses is invisible to its readers). The app copies row r of
    snapHdr()'s image into FreeImage scan line r, which FreeImage counts from the BOTTOM: the file's first (top) scan line is the
    image's last row. `image`: [h, w, 3 or 4] float; a missing alpha is written as 1."""
    import struct
    img = np.asarray(image, np.float32)
    h, w = img.shape[:2]
    rgba = np.ones((h, w, 4), np.float32)
    rgba[..., :img.shape[2]] = img[..., :4]

    def attr(name, typ, payload):
        return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(payload)) + payload
    chlist = b"".join(n + b"\0" + struct.pack("<iB3xii", 2, 0, 1, 1) for n in (b"A", b"B", b"G", b"R")) + b"\0"   # 2 = FLOAT
    box = struct.pack("<iiii", 0, 0, w - 1, h - 1)
    header = (struct.pack("<ii", 20000630, 2) + attr("channels", "chlist", chlist) + attr("compression", "compression", b"\0") +
              attr("dataWindow", "box2i", box) + attr("displayWindow", "box2i", box) + attr("lineOrder", "lineOrder", b"\0") +
              attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0)) +
              attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0")
    line_bytes = 4 * w * 4
    first = len(header) + 8 * h
    with open(path, "wb") as f:
        f.write(header)
        f.write(np.arange(h, dtype="<u8").__mul__(8 + line_bytes).__add__(first).astype("<u8").tobytes())   # offset table
        for y in range(h):
            row = rgba[h - 1 - y]                                   # top scan line first
            f.write(struct.pack("<ii", y, line_bytes))
            f.write(np.ascontiguousarray(row[:, [3, 2, 1, 0]].T, "<f4").tobytes())   # channel by channel: A, B, G, R


def read_exr(path):
    """The image of an uncompressed 32-bit-float scan-line OpenEXR file (what write_exr writes; any channel set), in snapHdr()'s
    row order: [h, w, 4] RGBA, a channel the file lacks reads 0 (alpha: 1)."""
    import struct
    data = open(path, "rb").read()
    magic, version = struct.unpack_from("<ii", data, 0)
    assert magic == 20000630 and (version & 0xFF) == 2 and not (version & 0x200), "not a scan-line OpenEXR 2 file"
    pos, attrs = 8, {}
    while data[pos] != 0:
        e = data.index(b"\0", pos); name = data[pos:e].decode(); pos = e + 1
        e = data.index(b"\0", pos); typ = data[pos:e].decode(); pos = e + 1
        (size,) = struct.unpack_from("<i", data, pos); pos += 4
        attrs[name] = (typ, data[pos:pos + size]); pos += size
    pos += 1
    assert attrs["compression"][1] == b"\0" and attrs["lineOrder"][1] == b"\0", "only uncompressed, increasing-y files"
    x0, y0, x1, y1 = struct.unpack("<iiii", attrs["dataWindow"][1])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    chans, cp, cl = [], 0, attrs["channels"][1]
    while cl[cp] != 0:
        e = cl.index(b"\0", cp); nm = cl[cp:e].decode(); cp = e + 1
        ptype, = struct.unpack_from("<i", cl, cp); cp += 16
        assert ptype == 2, "only 32-bit float channels"
        chans.append(nm)
    out = np.zeros((h, w, 4), np.float32)
    out[..., 3] = 1.0
    offs = np.frombuffer(data, "<u8", h, pos)
    for y in range(h):
        o = int(offs[y])
        yy, nbytes = struct.unpack_from("<ii", data, o)
        assert nbytes == 4 * w * len(chans)
        line = np.frombuffer(data, "<f4", w * len(chans), o + 8).reshape(len(chans), w)
        for k, nm in enumerate(chans):
            if nm in "RGBA":
                out[h - 1 - (yy - y0), :, "RGBA".index(nm)] = line[k]
    return out


def sharded_rounds(rays, intersector, materials, depth=16):
    """The bounce loop of Viewer.cpp:304-310 for one tile of a sharded frame, as a generator: yields
    the local ray count and is sent the GLOBAL count (sum over tiles), so the reference's
    `getRayCount() < 32 -> stop` rule (Pipeline.inl:459-461) is applied to the whole frame and the
    sharded image equals the unsharded one."""
    rays.applyMaterials(materials)
    for _ in range(depth):
        total = yield rays.raycountCache
        if total < 32:
            break
        rays.intersection(intersector, force=True)
        rays.shade(force=True)
        rays.reclaim()


class LaneResult(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("rays", C.c_uint64)]


class FrameBatch:
    """Several frames in flight on one GPU (psm_lanes_render): `lanes` independent copies of
    GltfViewer::process() (Viewer.cpp:296-312), each on its own context / HIP stream with its own
    TriangleHierarchy and Pipeline, so one frame's traversal tail overlaps the other frames' kernels.
    lanes[0].rays is the accumulating Pipeline: after a batch the lanes are folded into it in frame order
    (psm_rt_sample_from), which gives the image the same frames rendered one after another would give.

    rand(): the accumulating stream (setSeed) hands every frame one draw; that draw seeds the frame's own
    CRT-rand() stand-in, from which its camera() and shade() calls draw (Pipeline.inl:282,426)."""

    class Lane:
        def __init__(self, ctx, th, rays):
            self.ctx, self.th, self.rays = ctx, th, rays

    def __init__(self, lanes, width, height, device=0, seed=1, streams=None, display=None, master_stream=None):
        self.n = lanes
        self.lanes = []
        for s in range(lanes):
            ctx = Context(device, stream=None if streams is None else streams[s])
            th = TriangleHierarchy(ctx)
            rt = Pipeline(ctx, seed=seed)
            rt.resizeBuffers(width, height)
            rt.resize(*(display or (width, height)))
            self.lanes.append(FrameBatch.Lane(ctx, th, rt))
        # the accumulating Pipeline only samples: it has its own context so that folding a finished frame
        # never queues behind a lane's tracing kernels
        self.master_ctx = Context(device, stream=master_stream)
        self.master = Pipeline(self.master_ctx, seed=seed)
        self.master.resizeBuffers(width, height)
        self.master.resize(*(display or (width, height)))
        self.width, self.height = width, height
        self.frames_rendered = 0

    def pipelines(self):
        """every Pipeline that traces"""
        for ln in self.lanes:
            yield ln.rays

    # -- scene: every lane holds the same scene ------------------------------------------------------
    def allocate(self, n):
        for ln in self.lanes:
            ln.th.allocate(n)

    def loadTriangles(self, tris, normals=None, mats=None, texcoords=None):
        for ln in self.lanes:
            ln.th.loadTriangles(tris, normals, mats, texcoords)

    def loadMesh(self, mesh):
        for ln in self.lanes:
            ln.th.loadMesh(mesh)

    def clearTribuffer(self):
        for ln in self.lanes:
            ln.th.clearTribuffer()

    def each(self, fn):
        """Apply a setter to every lane's Pipeline: batch.each(lambda r: r.setSkybox(img))."""
        for r in self.pipelines():
            fn(r)

    def applyMaterials(self, materials):
        for r in self.pipelines():
            r.applyMaterials(materials)

    def setSeed(self, seed):
        self.master.setSeed(seed)

    # -- frames -----------------------------------------------------------------------------------------
    def frame_seeds(self, frames):
        return [self.master._rand() for _ in range(frames)]

    def trace(self, cam_inv, proj_inv, seeds, depth=16, rebuild=True, optimization=None, fold=True):
        """len(seeds) frames, up to `lanes` in flight. fold=True: sample() each into the accumulating Pipeline in
        frame order. fold=False (len(seeds) <= lanes): frame f stays in lane f for the caller to fold.
        Returns per-frame (rounds, rays)."""
        k = len(seeds)
        if k == 0:
            return []
        n = min(self.n, k)
        rts = (C.c_void_p * n)(*[ln.rays._h for ln in self.lanes[:n]])
        bvhs = (C.c_void_p * n)(*[ln.th._h for ln in self.lanes[:n]])
        sd = (C.c_uint32 * k)(*[v & 0xFFFFFFFF for v in seeds])
        res = (LaneResult * k)()
        ci = np.ascontiguousarray(cam_inv, np.float32).reshape(16)
        pi = np.ascontiguousarray(proj_inv, np.float32).reshape(16)
        opt = None if optimization is None else np.ascontiguousarray(optimization, np.float64).reshape(16)
        rc = lib().psm_lanes_render(rts, bvhs, C.c_uint32(n), _p(ci), _p(pi), sd, C.c_uint32(k), C.c_uint32(depth),
                                    C.c_int(int(rebuild)), _p(opt) if opt is not None else None,
                                    self.master._h if fold else None, res)
        self.lanes[0].ctx.check(rc, "psm_lanes_render")
        for ln in self.lanes[:n]:
            ln.th._dirty = False
            ln.rays._obj = ln.th
        return [(res[f].rounds, res[f].rays) for f in range(k)]

    def fold(self, k):
        """sample() for frames left in lanes 0..k-1 by trace(fold=False), in frame order."""
        for ln in self.lanes[:k]:
            self.master.ctx.check(lib().psm_rt_sample_from(self.master._h, ln.rays._h), "psm_rt_sample_from")

    # -- tile-sharded frames: lanes run free until their LOCAL count parks them (dist.run_batch_sharded) ----
    def run_sharded(self, seeds=None, cam_inv=None, proj_inv=None, force_until=None, depth=16, rebuild=True):
        """seeds given: begin len(seeds) frames (frame f on lane f) and run them until every lane is parked.
        seeds None: resume the parked frames, lane s at least up to round force_until[s].
        Returns (rounds, local_counts) per lane."""
        if seeds is not None:
            k = len(seeds)
            self._k = k
            self._rts = (C.c_void_p * k)(*[ln.rays._h for ln in self.lanes[:k]])
            self._bvhs = (C.c_void_p * k)(*[ln.th._h for ln in self.lanes[:k]])
            self._state = (C.c_uint32 * k)(*[v & 0xFFFFFFFF for v in seeds])
            self._rounds = (C.c_uint32 * k)()
            self._cam = (np.ascontiguousarray(cam_inv, np.float32).reshape(16), np.ascontiguousarray(proj_inv, np.float32).reshape(16))
        k = self._k
        fu = (C.c_uint32 * k)(*([0] * k if force_until is None else [int(v) for v in force_until]))
        counts = (C.c_int32 * k)()
        rc = lib().psm_lanes_run_sharded(self._rts, self._bvhs, C.c_uint32(k), _p(self._cam[0]), _p(self._cam[1]), self._state,
                                         self._rounds, fu, C.c_uint32(depth), C.c_int(int(seeds is not None)),
                                         C.c_int(int(rebuild)), None, counts)
        self.lanes[0].ctx.check(rc, "psm_lanes_run_sharded")
        if seeds is not None:
            for ln in self.lanes[:k]:
                ln.th._dirty = False
                ln.rays._obj = ln.th
        return list(self._rounds), list(counts)

    def render_batch_sharded(self, native, seeds, cam_inv, proj_inv, depth=16, rebuild=True):
        """len(seeds) tile-sharded frames in flight, start to finish, in the C ABI (psm_dist_render_batch): rounds,
        the (round, count) exchanges, one tile gather per frame and, on rank 0, the fold in frame order."""
        k = len(seeds)
        rts = (C.c_void_p * k)(*[ln.rays._h for ln in self.lanes[:k]])
        bvhs = (C.c_void_p * k)(*[ln.th._h for ln in self.lanes[:k]])
        sd = (C.c_uint32 * k)(*[v & 0xFFFFFFFF for v in seeds])
        rounds = (C.c_uint32 * k)()
        ci = np.ascontiguousarray(cam_inv, np.float32).reshape(16)
        pi = np.ascontiguousarray(proj_inv, np.float32).reshape(16)
        rc = lib().psm_dist_render_batch(native._h, rts, bvhs, C.c_uint32(k), _p(ci), _p(pi), sd, C.c_uint32(depth), C.c_int(int(rebuild)),
                                         None, self.master._h, rounds)
        self.lanes[0].ctx.check(rc, "psm_dist_render_batch")
        for ln in self.lanes[:k]:
            ln.th._dirty = False
            ln.rays._obj = ln.th
        return list(rounds)

    def render_frames_sharded(self, native, seeds, cam_inv, proj_inv, depth=16, rebuild=True, lanes=None):
        """len(seeds) tile-sharded frames with all lanes (or the first `lanes` of them) in flight and no drain between batches
        (psm_dist_render_frames)."""
        k, n = len(seeds), (self.n if lanes is None else max(1, min(int(lanes), self.n)))
        rts = (C.c_void_p * n)(*[ln.rays._h for ln in self.lanes[:n]])
        bvhs = (C.c_void_p * n)(*[ln.th._h for ln in self.lanes[:n]])
        sd = (C.c_uint32 * max(k, 1))(*[v & 0xFFFFFFFF for v in seeds])
        rounds = (C.c_uint32 * max(k, 1))()
        ci = np.ascontiguousarray(cam_inv, np.float32).reshape(16)
        pi = np.ascontiguousarray(proj_inv, np.float32).reshape(16)
        rc = lib().psm_dist_render_frames(native._h, rts, bvhs, C.c_uint32(n), _p(ci), _p(pi), sd, C.c_uint32(k), C.c_uint32(depth),
                                          C.c_int(int(rebuild)), None, self.master._h, rounds)
        self.lanes[0].ctx.check(rc, "psm_dist_render_frames")
        for ln in self.lanes[:n]:
            ln.th._dirty = False
            ln.rays._obj = ln.th
        return list(rounds)[:k]

    def fold_one(self, lane):
        self.master.ctx.check(lib().psm_rt_sample_from(self.master._h, lane.rays._h), "psm_rt_sample_from")

    def render(self, frames, eye, view, depth=16, rebuild=True):
        """`frames` x process() with `lanes` frames in flight; returns per-frame (rounds, rays)."""
        sc = self.master._sc
        ci, pi = sc.camera_matrices(eye, view, self.master.displayWidth, self.master.displayHeight)
        out = self.trace(ci, pi, self.frame_seeds(frames), depth, rebuild)
        self.frames_rendered += frames
        return out

    def snapHdr(self, raw=False):
        return self.master.snapHdr(raw)

    def clearSampler(self):
        self.master.clearSampler()

    def contexts(self):
        for ln in self.lanes:
            yield ln.ctx

    def sync(self):
        for c in self.contexts():
            c.sync()
        self.master_ctx.sync()

    def close(self):
        for ln in self.lanes:
            ln.rays.close()
            ln.th.close()
        for ln in self.lanes:
            ln.ctx.close()
        self.lanes = []
        self.master.close()
        self.master_ctx.close()


def render_frame(rays, intersector, materials, eye, view, depth=16):
    """GltfViewer::process(), Source/Examples/Viewer.cpp:296-312 (minus display)."""
    materials.loadToVGA()
    intersector.markDirty()
    intersector.build()
    rays.camera(eye, view)
    rounds = 0
    for _ in range(depth):
        if rays.getRayCount() <= 0:
            break
        rays.intersection(intersector)
        rays.applyMaterials(materials)
        rays.shade()
        rays.reclaim()
        rounds += 1
    rays.sample()
    rays.render()
    return rounds
